"""Exact PERCENTILE against its DISTINCTCOUNT twins on one synthetic segment, alternated in one process (dev tool, not a test).

The twin of every query has DISTINCTCOUNT of the same column in place of the percentile(s): it streams the same bytes and sets a bit where
the percentile pass adds to a counter.  Device time is the library's HIP-event total (pg_exec_stats.device_ms_total — for a percentile
query: the ordinary part, the filter pass and the percentile passes); the fraction of 8 TB/s comes from pg_exec_stats.algorithmic_bytes.
Prints one line per query (median of --reps alternated runs) and the ratio of every percentile query to its twin:
  * PERCENTILE(m_d, 95), no filter, no GROUP BY;
  * config 3's filter, GROUP BY g1, g2, one percentile;
  * the same with three percentiles (one counting pass: they share the column).
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
    "pctl_plain": "SELECT PERCENTILE(m_d, 95) FROM gpuBench",
    "pctl_plain_twin": "SELECT DISTINCTCOUNT(m_d) FROM gpuBench",
    "pctl_cfg3_groupby": f"SELECT g1, g2, COUNT(*), PERCENTILE(m_d, 95) FROM gpuBench {WHERE} GROUP BY g1, g2 LIMIT 100000",
    "pctl_cfg3_groupby_3p": f"SELECT g1, g2, COUNT(*), PERCENTILE(m_d, 50), PERCENTILE(m_d, 95), PERCENTILE(m_d, 99) FROM gpuBench {WHERE} GROUP BY g1, g2 LIMIT 100000",
    "pctl_cfg3_groupby_twin": f"SELECT g1, g2, COUNT(*), DISTINCTCOUNT(m_d) FROM gpuBench {WHERE} GROUP BY g1, g2 LIMIT 100000",
}
TWIN = {"pctl_plain": "pctl_plain_twin", "pctl_cfg3_groupby": "pctl_cfg3_groupby_twin", "pctl_cfg3_groupby_3p": "pctl_cfg3_groupby_twin"}

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=1_000_000_000)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--final", action="store_true", help="PG_QUERY_FLAG_FINAL_PERCENTILE / _FINAL_DISTINCT: only final values cross PCIe")
ap.add_argument("--only", default="", help="comma-separated query names (e.g. for a rocprofv3 run of one kernel)")
args = ap.parse_args()

api = capi.gpu_api()
api.call("init", 0)
seg = NativeSegment(api, HostSegment("prof_percentile", args.docs))
for name in ["c_inv1", "c_inv2", "r_int", "g1", "g2", "m_d"]:
    one = synth.generate_segment(args.docs, columns=[name])
    seg.add_column(one.columns[name], keep_host_buffers=False)

names = [n for n in QUERIES if not args.only or n in args.only.split(",")]
qcs = {n: parse_sql(QUERIES[n]) for n in names}
skipped = {}
for n in list(names):
    qcs[n].num_groups_limit = 2_000_000_000
    if args.final:
        qcs[n].flags |= capi.QUERY_FLAG_FINAL_PERCENTILE | capi.QUERY_FLAG_FINAL_DISTINCT
    try:
        seg.execute(qcs[n], profile=True)   # warm-up: plans, virtual dictionaries
    except capi.NativeError as e:          # a refusal is a result of the measurement too
        skipped[n] = e.message
        names.remove(n)
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

print(f"# prof_percentile: {args.docs} docs, {args.reps} alternated reps, medians{', final values' if args.final else ''}")
med = {}
for n in names:
    st = last[n].stats
    med[n] = statistics.median(dev[n])
    frac = st.algorithmic_bytes / (med[n] * 1e-3) / 8e12 if med[n] > 0 else 0.0
    print(f"{n:24s} device_ms {med[n]:9.3f}  wall_ms {statistics.median(wall[n]):9.3f}  groups {last[n].num_groups:6d}  "
          f"kernel {st.kernel.decode():24s} docs_scanned {st.num_docs_scanned:11d}  algorithmic_bytes {st.algorithmic_bytes:12d}  "
          f"frac_of_8TBps {frac:.3f}  query: {QUERIES[n]}")
for n, why in skipped.items():
    print(f"{n:24s} refused: {why}")
for n, t in TWIN.items():
    if n in med and t in med and med[t] > 0:
        print(f"ratio {n} / {t} device time: {med[n] / med[t]:.3f}; wall time: {statistics.median(wall[n]) / statistics.median(wall[t]):.3f}")
seg.destroy()
