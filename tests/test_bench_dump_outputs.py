"""bench.py --dump-outputs without a GPU: the writer's arrays against the rows of the same result (the CPU oracle's block stands in for the
timed step's), groups in key order, float64 only, and the size limit met by a seeded sample that is the same on every call."""
import os

import numpy as np
import pytest

import bench
from pinot_amd import synth
from pinot_amd.executor import NativeSegment


@pytest.fixture(scope="module")
def blocks(oracle_api):
    host = synth.generate_segment(20_000, columns=list(synth.CFG5_COLUMNS) + list(synth.CFG3_COLUMNS))
    seg = NativeSegment(oracle_api, host)
    out = {q: seg.execute(sql) for q, sql in (("cfg3", synth.QUERY_CFG3), ("cfg5", synth.QUERY_CFG5), ("cfg2", synth.QUERY_CFG2))}
    yield out
    seg.destroy()


def load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_arrays_equal_the_rows_in_key_order(blocks, tmp_path):
    b = blocks["cfg3"]
    bench.dump_outputs(b, str(tmp_path))
    got = load(str(tmp_path))
    assert sorted(got) == ["agg0_sum_m", "agg1_max_m", "group_keys", "stats"]
    assert all(a.dtype == np.float64 for a in got.values())
    rows = b.rows()
    keys = sorted(rows)
    assert got["group_keys"].tolist() == [list(k) for k in keys]
    assert got["agg0_sum_m"].tolist() == [rows[k][0] for k in keys]
    assert got["agg1_max_m"].tolist() == [rows[k][1] for k in keys]
    assert got["stats"].tolist() == [b.stats.num_docs_scanned, b.stats.num_entries_scanned_in_filter, b.stats.num_entries_scanned_post_filter,
                                     b.stats.num_total_docs, b.stats.num_groups_limit_reached]


def test_no_group_by(blocks, tmp_path):
    b = blocks["cfg2"]
    bench.dump_outputs(b, str(tmp_path))
    got = load(str(tmp_path))
    assert sorted(got) == ["agg0_count_star", "stats"]
    assert got["agg0_count_star"].tolist() == [b.aggregation_result()[0]]


def test_size_limit_takes_the_same_sample_every_time(blocks, tmp_path):
    b = blocks["cfg5"]
    bench.dump_outputs(b, str(tmp_path / "full"))
    full = load(str(tmp_path / "full"))
    assert full["agg1_distinctcounthll_u"].shape == (b.num_groups, 256)
    limit = 1 << 20
    for d in ("a", "b"):
        bench.dump_outputs(b, str(tmp_path / d), limit_bytes=limit)
        assert sum(os.path.getsize(os.path.join(tmp_path, d, f)) for f in os.listdir(tmp_path / d)) <= limit
    a, c = load(str(tmp_path / "a")), load(str(tmp_path / "b"))
    assert sorted(a) == sorted(full)
    assert all(np.array_equal(a[k], c[k]) for k in a)
    n = len(a["group_keys"])
    assert 0 < n < b.num_groups
    # the sample is a subset of the groups, still in key order, with each group's own results
    pos = {tuple(k): i for i, k in enumerate(full["group_keys"].tolist())}
    idx = [pos[tuple(k)] for k in a["group_keys"].tolist()]
    assert idx == sorted(idx)
    assert all(np.array_equal(a[k], full[k][idx]) for k in a if k != "stats")


def test_full_is_an_option():
    """`--full` exists (what it gates needs a GPU: tests/test_gpu_bench_contract.py); checked on the parser's own help, before anything is imported."""
    import subprocess
    import sys
    out = subprocess.run([sys.executable, bench.__file__, "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "--full" in out.stdout.split("options:")[0], out.stdout[:500]
