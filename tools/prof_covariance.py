"""COVAR_POP against its twin on the existing kernels, alternated in one process (dev tool, not a test), in the manner of
tools/prof_variance.py and DESIGN 4.8's protocol.

gpuBench at 2 x 10^8 docs by default.  The twin of every query is `SUM(m), SUM(r_int), SUM(m * r_int), COUNT(*)` of the same shape: it
produces the same four numbers through the ordinary part plus the expression pass, where the covariance takes the ordinary
part (COUNT(*)) plus ONE fused pass.  m and r_int are raw INT columns: two integer slots, five product limbs and the count per doc.
Three shapes:
  * COVAR_POP(m, r_int), no filter, no GROUP BY      (pg_covar_reg)
  * COVAR_POP(m, r_int) GROUP BY g1                  (pg_covar_lds: 100 groups x 8 slots)
  * config 3's filter, GROUP BY g1                   (pg_covar_lds behind the filter's match words)
No ratio is fixed in advance; the expectation is that the fused pass is no slower than the twin.

Which number comes from where, and the order to read them in:
  1. kernel time: a kernel trace in a run of its own —
         rocprofv3 --kernel-trace --stats -d DIR -- python tools/prof_covariance.py --reps 3
     (pg_covar_reg / pg_covar_lds by their stable names; pg_covar_reg_wide for more than one pair); tracing slows the host, so nothing else is read from that run;
  2. device time: the library's HIP-event total (pg_exec_stats.device_ms_total: the ordinary part, the filter pass and the accumulation
     pass), median of --reps alternated runs with the profiler off, with its spread;
  3. the ratio to the twin, from the same alternated runs;
  4. the fraction of 8 TB/s: pg_exec_stats.algorithmic_bytes over the device time — a whole-query rate, not a kernel's share of peak;
  5. wall time last: it includes the host's planning and the joins.
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
COVAR = "COVAR_POP(m, r_int)"
TWIN_AGGS = "SUM(m), SUM(r_int), SUM(m * r_int), COUNT(*)"
QUERIES = {
    "covar_plain": f"SELECT {COVAR} FROM gpuBench",
    "covar_plain_twin": f"SELECT {TWIN_AGGS} FROM gpuBench",
    "covar_g1": f"SELECT g1, {COVAR} FROM gpuBench GROUP BY g1 LIMIT 100000",
    "covar_g1_twin": f"SELECT g1, {TWIN_AGGS} FROM gpuBench GROUP BY g1 LIMIT 100000",
    "covar_cfg3_g1": f"SELECT g1, {COVAR} FROM gpuBench {WHERE} GROUP BY g1 LIMIT 100000",
    "covar_cfg3_g1_twin": f"SELECT g1, {TWIN_AGGS} FROM gpuBench {WHERE} GROUP BY g1 LIMIT 100000",
}
TWIN = {n: n + "_twin" for n in QUERIES if not n.endswith("_twin")}

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=200_000_000)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--only", default="", help="comma-separated query names (e.g. for a rocprofv3 run of one kernel)")
args = ap.parse_args()

api = capi.gpu_api()
api.call("init", 0)
seg = NativeSegment(api, HostSegment("prof_covariance", args.docs))
for name in ["c_inv1", "c_inv2", "r_int", "g1", "m"]:
    one = synth.generate_segment(args.docs, columns=[name])
    seg.add_column(one.columns[name], keep_host_buffers=False)
    print(f"# column {name} registered", flush=True)

names = [n for n in QUERIES if not args.only or n in args.only.split(",")]
qcs = {n: parse_sql(QUERIES[n]) for n in names}
skipped, first = {}, {}
for n in list(names):
    qcs[n].num_groups_limit = 2_000_000_000
    try:
        t0 = time.perf_counter()
        seg.execute(qcs[n], profile=True)   # warm-up: plans, code objects, the expression's bounds pass
        seg.execute(qcs[n], profile=True)
        first[n] = (time.perf_counter() - t0) * 1e3
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

print(f"# prof_covariance: {args.docs} docs, {args.reps} alternated reps, medians")
med = {}
for n in names:
    st = last[n].stats
    med[n] = statistics.median(dev[n])
    frac = st.algorithmic_bytes / (med[n] * 1e-3) / 8e12 if med[n] > 0 else 0.0
    print(f"{n:20s} device_ms {med[n]:9.3f}  (min {min(dev[n]):.3f}, max {max(dev[n]):.3f})  aggregate_ms {st.device_ms_aggregate:9.3f}  wall_ms {statistics.median(wall[n]):9.3f}  "
          f"warm_up_wall_ms {first[n]:9.3f}  groups {last[n].num_groups:6d}  kernel {st.kernel.decode():24s} docs_scanned {st.num_docs_scanned:11d}  "
          f"algorithmic_bytes {st.algorithmic_bytes:12d}  frac_of_8TBps {frac:.3f}  query: {QUERIES[n]}")
for n, why in skipped.items():
    print(f"{n:20s} refused: {why}")
# the two results of a pair hold the same four numbers where both windows hold every digit: checked on the last run
for n, t in TWIN.items():
    if n in last and t in last:
        a, b = last[n].rows() if qcs[n].group_by else {(): last[n].aggregation_result()}, last[t].rows() if qcs[t].group_by else {(): last[t].aggregation_result()}
        same = all(tuple(a[k][0]) == (b[k][0], b[k][1], b[k][2], b[k][3]) for k in a) and set(a) == set(b)
        print(f"tuple of {n} equals the four results of {t}: {same}")
for n, t in TWIN.items():
    if n in med and t in med and med[t] > 0:
        print(f"ratio {n} / {t} device time: {med[n] / med[t]:.3f}; wall time: {statistics.median(wall[n]) / statistics.median(wall[t]):.3f}")
seg.destroy()
