"""SELECT DISTINCT against its GROUP BY / ORDER BY twins on one synthetic segment, alternated in one process (dev tool, not a test).

Device time is the library's HIP-event total (pg_exec_stats.device_ms_total: the filter plus the DISTINCT stages); the fraction of
8 TB/s comes from pg_exec_stats.algorithmic_bytes.  Prints one line per query (median of --reps alternated runs) and the ratios the
DISTINCT work is judged by:
  * config 3's filter, DISTINCT g1, g2 ORDER BY g1, g2 LIMIT 10000 against GROUP BY g1, g2 with COUNT(*) (target: no slower);
  * DISTINCT g1, g2 LIMIT 100 against its ORDER BY twin (target: at most 5 % of its device time);
  * the HBM tier, DISTINCT u, g2 ORDER BY u DESC LIMIT 100 (no target).
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
    "distinct_cfg3_ordered": f"SELECT DISTINCT g1, g2 FROM gpuBench {WHERE} ORDER BY g1, g2 LIMIT 10000",
    "groupby_cfg3_twin": f"SELECT g1, g2, COUNT(*) FROM gpuBench {WHERE} GROUP BY g1, g2 ORDER BY g1, g2 LIMIT 10000",
    "distinct_limit100": "SELECT DISTINCT g1, g2 FROM gpuBench LIMIT 100",
    "distinct_limit100_ordered_twin": "SELECT DISTINCT g1, g2 FROM gpuBench ORDER BY g1, g2 LIMIT 100",
    "distinct_hbm_tier": "SELECT DISTINCT u, g2 FROM gpuBench ORDER BY u DESC LIMIT 100",
}

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=1_000_000_000)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--only", default="", help="comma-separated query names (e.g. for a rocprofv3 --pmc run of one kernel)")
args = ap.parse_args()

api = capi.gpu_api()
api.call("init", 0)
seg = NativeSegment(api, HostSegment("prof_distinct", args.docs))
for name in ["c_inv1", "c_inv2", "r_int", "g1", "g2", "u"]:
    one = synth.generate_segment(args.docs, columns=[name])
    seg.add_column(one.columns[name], keep_host_buffers=False)

names = [n for n in QUERIES if not args.only or n in args.only.split(",")]
qcs = {n: parse_sql(QUERIES[n]) for n in names}
for n in names:
    if "groupby" in n:
        qcs[n].num_groups_limit = 2_000_000_000
    seg.execute(qcs[n], profile=True)   # warm-up: plans, virtual work areas
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

print(f"# prof_distinct: {args.docs} docs, {args.reps} alternated reps, medians")
med = {}
for n in names:
    st = last[n].stats
    med[n] = statistics.median(dev[n])
    frac = st.algorithmic_bytes / (med[n] * 1e-3) / 8e12 if med[n] > 0 else 0.0
    print(f"{n:34s} device_ms {med[n]:8.3f}  wall_ms {statistics.median(wall[n]):8.3f}  rows {last[n].num_groups:6d}  "
          f"kernel {st.kernel.decode():24s} docs_scanned {st.num_docs_scanned:11d}  algorithmic_bytes {st.algorithmic_bytes:12d}  "
          f"frac_of_8TBps {frac:.3f}  query: {QUERIES[n]}")
if "distinct_cfg3_ordered" in med and "groupby_cfg3_twin" in med:
    print(f"ratio distinct_cfg3_ordered / groupby_cfg3_twin device time: {med['distinct_cfg3_ordered'] / med['groupby_cfg3_twin']:.3f} (target <= 1)")
if "distinct_limit100" in med and "distinct_limit100_ordered_twin" in med:
    print(f"ratio distinct_limit100 / ordered twin device time: {med['distinct_limit100'] / med['distinct_limit100_ordered_twin']:.3f} (target <= 0.05)")
seg.destroy()
