"""MODE against the twin the parent commit can already run on the same segment and shape — PERCENTILE(col, 50) with
PG_QUERY_FLAG_FINAL_PERCENTILE: the same counting pass, so the difference is the selection —, alternated in one process (dev tool, not a
test), in the manner of tools/prof_histogram.py and DESIGN 4.10's protocol.

gpuBench at 2 x 10^8 docs by default.  No ratio is fixed in advance.  The shapes:
  * wide     MODE(m_d) without GROUP BY: one row of 2^20 counters (pg_pctl_hbm), the case DESIGN 4.5 (d) calls a latency chain
  * g7       MODE(v100) GROUP BY g7: 7 rows of 100 counters (pg_pctl_lds), one wavefront per row
  * sort     MODE(v100) WHERE g7 = 3 with PG_PCTL_HBM_MAX_BYTES=4: the sort tier (pg_pctl_sort) over a seventh of the docs
each as final value (PG_QUERY_FLAG_FINAL_MODE), as final AVG, and as intermediate map, next to its twin.
Then pg_mode_select's switch: the wide shape by PG_MODE_SPLIT_IDS, from 64 ids per wavefront share to the whole row in one wavefront.

Which number comes from where: device time is the library's HIP-event total (pg_exec_stats.device_ms_total) and the counting path's own
events (device_ms_aggregate: counting pass, selection, runs / ties and their copies), medians of --reps alternated runs with the profiler
off, with their spread; wall time last."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401,E402  (initialises the ROCm runtime as bench.py does)
from pinot_amd import capi, synth  # noqa: E402
from pinot_amd.executor import NativeSegment  # noqa: E402
from pinot_amd.query import parse_sql  # noqa: E402
from pinot_amd.segment import HostSegment, build_column  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=200_000_000)
ap.add_argument("--reps", type=int, default=7)
args = ap.parse_args()
n = args.docs

api = capi.gpu_api()
api.call("init", 0)
seg = NativeSegment(api, HostSegment("prof_mode", n))
seg.add_column(synth.generate_segment(n, columns=["m_d"]).columns["m_d"], keep_host_buffers=False)
print("# column m_d registered: dictionary INT, 2^20 values", flush=True)
seg.add_column(build_column("v100", (np.arange(n, dtype=np.int64) * 37 % 1009 % 100).astype(np.int32), "INT"), keep_host_buffers=False)
seg.add_column(build_column("g7", (np.arange(n, dtype=np.int32) * 5 + 3) % 7, "INT"), keep_host_buffers=False)
print("# columns v100 (100 values) and g7 (7 values) registered: dictionary INT", flush=True)

FINAL = capi.QUERY_FLAG_FINAL_MODE | capi.QUERY_FLAG_FINAL_PERCENTILE
SHAPES = {   # name: (FROM ... tail, column, knobs)
    "wide": ("FROM gpuBench", "m_d", "", {}),
    "g7": ("FROM gpuBench GROUP BY g7 LIMIT 100000", "v100", "g7, ", {}),
    "sort": ("FROM gpuBench WHERE g7 = 3", "v100", "", {"PG_PCTL_HBM_MAX_BYTES": "4"}),
}
QUERIES = {}   # name: (sql, flags, knobs)
for shape, (tail, col, keys, knobs) in SHAPES.items():
    QUERIES[f"{shape}_mode_final"] = (f"SELECT {keys}MODE({col}) {tail}", FINAL, knobs)
    QUERIES[f"{shape}_mode_avg_final"] = (f"SELECT {keys}MODE({col}, 'AVG') {tail}", FINAL, knobs)
    QUERIES[f"{shape}_mode_map"] = (f"SELECT {keys}MODE({col}) {tail}", 0, knobs)
    QUERIES[f"{shape}_twin_final"] = (f"SELECT {keys}PERCENTILE({col}, 50) {tail}", FINAL, knobs)
    QUERIES[f"{shape}_twin_runs"] = (f"SELECT {keys}PERCENTILE({col}, 50) {tail}", 0, knobs)


def set_knobs(knobs):
    for k in ("PG_PCTL_HBM_MAX_BYTES", "PG_MODE_SPLIT_IDS"):
        os.environ.pop(k, None)
    os.environ.update(knobs)
    api.call("options_reload")


def run(name):
    sql, flags, knobs = QUERIES[name]
    qc = parse_sql(sql)
    qc.flags |= flags
    qc.num_groups_limit = 2_000_000_000
    t0 = time.perf_counter()
    rb = seg.execute(qc, profile=True)
    return rb, (time.perf_counter() - t0) * 1e3


names, skipped = list(QUERIES), {}
for shape in SHAPES:   # one setting of the knobs at a time; within it the twins alternate
    group = [q for q in names if q.startswith(shape + "_")]
    set_knobs(SHAPES[shape][3])
    for q in list(group):
        try:
            run(q)   # warm-up: plans, code objects
            run(q)
        except capi.NativeError as e:   # a refusal is a result of the measurement too
            skipped[q] = e.message
            group.remove(q)
        print(f"# warmed up {q}", flush=True)
    dev = {q: [] for q in group}
    agg = {q: [] for q in group}
    wall = {q: [] for q in group}
    last = {}
    for _ in range(args.reps):
        for q in group:
            rb, ms = run(q)
            dev[q].append(rb.stats.device_ms_total)
            agg[q].append(rb.stats.device_ms_aggregate)
            wall[q].append(ms)
            last[q] = rb
    med = {}
    for q in group:
        st = last[q].stats
        med[q] = (statistics.median(dev[q]), statistics.median(agg[q]))
        print(f"{q:22s} device_ms {med[q][0]:9.3f} (min {min(dev[q]):.3f}, max {max(dev[q]):.3f})  counting_path_ms {med[q][1]:9.3f} (min {min(agg[q]):.3f}, max {max(agg[q]):.3f})  "
              f"wall_ms {statistics.median(wall[q]):9.3f}  groups {last[q].num_groups:4d}  kernel {st.kernel.decode():14s} docs_scanned {st.num_docs_scanned:11d}  query: {QUERIES[q][0]}")
    for q, t in ((f"{shape}_mode_final", f"{shape}_twin_final"), (f"{shape}_mode_avg_final", f"{shape}_twin_final"), (f"{shape}_mode_map", f"{shape}_twin_runs")):
        if q in med and t in med and med[t][0] > 0 and med[t][1] > 0:
            print(f"ratio {q} / {t}: device time {med[q][0] / med[t][0]:.3f}, counting path {med[q][1] / med[t][1]:.3f}")
for q, why in skipped.items():
    print(f"{q:22s} refused: {why}")

# ---- pg_mode_select's switch: ids per wavefront share over the one wide row --------------------------------------------------------------------
SPLITS = (64, 256, 1024, 4096, 16384, 65536, 1 << 20)
print("# wide_mode_final counting_path_ms by PG_MODE_SPLIT_IDS (2^20: one wavefront walks the row alone); the twin's rank selection for comparison")
table = {s: [] for s in SPLITS}
twin = []
for _ in range(args.reps):
    for s in SPLITS:   # alternated over the settings as well
        set_knobs({"PG_MODE_SPLIT_IDS": str(s)})
        table[s].append(run("wide_mode_final")[0].stats.device_ms_aggregate)
    twin.append(run("wide_twin_final")[0].stats.device_ms_aggregate)
set_knobs({})
print("  ".join(f"{s}: {statistics.median(table[s]):.3f} (min {min(table[s]):.3f})" for s in SPLITS) + f"  twin: {statistics.median(twin):.3f} (min {min(twin):.3f})")
seg.destroy()
