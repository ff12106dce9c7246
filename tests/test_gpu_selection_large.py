"""Selection queries at 2 x 10^8 docs against numpy on the synthetic values (pinot_amd/synth.py): ORDER BY m DESC LIMIT 10 over the whole
segment, LIMIT 1000 behind config 3's filter, and an adversarial column that rises with docId under ORDER BY ... DESC, so that every new doc
beats the threshold of the streaming top-K.  Its time is recorded, with no target."""
import time

import numpy as np
import pytest

from pinot_amd import synth
from pinot_amd.executor import NativeSegment
from pinot_amd.segment import build_column

pytestmark = pytest.mark.gpu
DOCS = 200_000_000
WHERE = "WHERE c_inv1 IN (0,1,2,3) AND c_inv2 IN (0,1) AND r_int BETWEEN 250000 AND 749999"


def _values(name):
    return synth.values_numpy(synth.GPU_BENCH[name], synth.SEED_BASE ^ 0, DOCS)


def _top_desc(vals, k):
    part = np.partition(vals, len(vals) - k)[len(vals) - k:]
    return sorted(part.tolist(), reverse=True)


def test_top_k_at_scale(gpu_api, record_property):
    host = synth.generate_segment(DOCS, segment_index=0, columns=synth.CFG3_COLUMNS)
    rise = np.arange(DOCS, dtype=np.int32)
    rise[[0, 1]] = [1, 0]   # not sorted (a sorted first ORDER BY column is the linear operators'), yet every later doc beats the ones before
    host.columns["rise"] = build_column("rise", rise, "INT", dictionary=False)
    g = NativeSegment(gpu_api, host)
    try:
        m = _values("m")
        g1 = _values("g1")
        # the whole segment: the ten largest m, each row's g1 that of a doc holding its m
        rb = g.execute("SELECT m, g1 FROM gpuBench ORDER BY m DESC LIMIT 10")
        rows = rb.selection_rows
        assert [r[0] for r in rows] == _top_desc(m, 10)
        for mv, gv in rows:
            assert gv in set(g1[m == mv].tolist())
        assert rb.stats.num_docs_scanned == DOCS and rb.stats.kernel.decode() == "pg_select_topk_lds"
        # config 3's filter: the 1000 largest m among the matches
        match = np.isin(_values("c_inv1"), [0, 1, 2, 3]) & np.isin(_values("c_inv2"), [0, 1])
        r_int = _values("r_int")
        match &= (r_int >= 250000) & (r_int <= 749999)
        rb = g.execute(f"SELECT m, r_int FROM gpuBench {WHERE} ORDER BY m DESC LIMIT 1000")
        assert [r[0] for r in rb.selection_rows] == _top_desc(m[match], 1000)
        assert rb.stats.num_docs_scanned == int(match.sum())
        assert all(250000 <= r[1] <= 749999 for r in rb.selection_rows)
        # adversarial: every doc beats the threshold the docs before it set
        t0 = time.perf_counter()
        rb = g.execute("SELECT rise, g1 FROM gpuBench ORDER BY rise DESC LIMIT 1000")
        wall_ms = (time.perf_counter() - t0) * 1e3
        assert [r[0] for r in rb.selection_rows] == list(range(DOCS - 1, DOCS - 1001, -1))
        assert [r[1] for r in rb.selection_rows] == g1[DOCS - 1000:][::-1].tolist()
        record_property("adversarial_device_ms", rb.stats.device_ms_total)
        record_property("adversarial_wall_ms", wall_ms)
        print(f"adversarial ORDER BY rise DESC LIMIT 1000 at {DOCS} docs: device {rb.stats.device_ms_total:.3f} ms, wall {wall_ms:.1f} ms")
    finally:
        g.destroy()
