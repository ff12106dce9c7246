"""Selection queries against their MAX twins on one synthetic segment, alternated in one process (dev tool, not a test).

Device time is the library's HIP-event total (pg_exec_stats.device_ms_total: the filter plus the selection stages); the fraction of 8 TB/s
comes from pg_exec_stats.algorithmic_bytes.  Prints one line per query (median of --reps alternated runs) and the ratios the selection work is
judged by:
  (a) config 3's filter, SELECT m, g1, u ... ORDER BY m DESC LIMIT 10 against SELECT MAX(m) behind the same filter (target: at most 1.3x);
  (b) no filter, SELECT m, g1 ... ORDER BY m_d DESC LIMIT 100 (a dictionary key) against SELECT MAX(m_d) (target: at most 1.3x);
  (c) (a) with LIMIT 100000: the sort tier over every match (reported only; without the filter its 10^9 pairs exceed the work-area budget);
  (d) SELECT * LIMIT 10, without a filter (no kernel over the segment) and behind config 3's filter (the filter still runs whole).
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401,E402  (initialises the ROCm runtime as bench.py does)
from pinot_amd import capi, synth  # noqa: E402
from pinot_amd.executor import NativeSegment  # noqa: E402
from pinot_amd.query import parse_sql  # noqa: E402
from pinot_amd.segment import HostSegment  # noqa: E402

WHERE = "WHERE c_inv1 IN (0,1,2,3) AND c_inv2 IN (0,1) AND r_int BETWEEN 250000 AND 749999"
QUERIES = {
    "a_topk_cfg3": f"SELECT m, g1, u FROM gpuBench {WHERE} ORDER BY m DESC LIMIT 10",
    "a_max_twin": f"SELECT MAX(m) FROM gpuBench {WHERE}",
    "b_topk_dict_key": "SELECT m, g1 FROM gpuBench ORDER BY m_d DESC LIMIT 100",
    "b_max_twin": "SELECT MAX(m_d) FROM gpuBench",
    "c_sort_tier": f"SELECT m, g1, u FROM gpuBench {WHERE} ORDER BY m DESC LIMIT 100000",
    "d_star_limit10": "SELECT * FROM gpuBench LIMIT 10",
    "d_star_limit10_cfg3": f"SELECT * FROM gpuBench {WHERE} LIMIT 10",
}

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=1_000_000_000)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--only", default="", help="comma-separated query names")
args = ap.parse_args()

api = capi.gpu_api()
api.call("init", 0)
seg = NativeSegment(api, HostSegment("prof_selection", args.docs))
for name in ["c_inv1", "c_inv2", "r_int", "g1", "m", "m_d", "u"]:
    one = synth.generate_segment(args.docs, columns=[name])
    seg.add_column(one.columns[name], keep_host_buffers=False)

names = [n for n in QUERIES if not args.only or n in args.only.split(",")]
qcs = {n: parse_sql(QUERIES[n]) for n in names}
for n in names:
    seg.execute(qcs[n], profile=True)   # warm-up: plans, work areas
dev = {n: [] for n in names}
wall = {n: [] for n in names}
last = {}
for _ in range(args.reps):
    for n in names:   # alternated: the twins see the same clocks and caches
        t0 = time.perf_counter()
        rb = seg.execute(qcs[n], profile=True)
        wall[n].append((time.perf_counter() - t0) * 1e3)
        dev[n].append(rb.stats.device_ms_total)
        last[n] = rb

print(f"# prof_selection: {args.docs} docs, {args.reps} alternated reps, medians")
med = {}
for n in names:
    st = last[n].stats
    med[n] = statistics.median(dev[n])
    frac = st.algorithmic_bytes / (med[n] * 1e-3) / 8e12 if med[n] > 0 else 0.0
    print(f"{n:22s} device_ms {med[n]:8.3f}  wall_ms {statistics.median(wall[n]):8.3f}  rows {last[n].num_groups:6d}  "
          f"kernel {st.kernel.decode():20s} docs_scanned {st.num_docs_scanned:11d}  algorithmic_bytes {st.algorithmic_bytes:12d}  "
          f"frac_of_8TBps {frac:.3f}  query: {QUERIES[n]}")
for a, b, target in (("a_topk_cfg3", "a_max_twin", "<= 1.3"), ("b_topk_dict_key", "b_max_twin", "<= 1.3")):
    if a in med and b in med and med[b] > 0:
        print(f"ratio {a} / {b} device time: {med[a] / med[b]:.3f} (target {target})")
    elif a in med and b in med:   # MAX over a dictionary column without a filter: NonScanBasedAggregationOperator, no kernel
        print(f"ratio {a} / {b}: n/a, the twin runs no kernel ({last[b].stats.kernel.decode() or 'answered from the dictionary'})")
seg.destroy()
