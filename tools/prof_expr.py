"""Aggregations over an arithmetic expression against their plain-SUM twins on one synthetic segment, alternated in one process (dev tool,
not a test).

The twin of every query has plain SUMs over the expression's operand columns in place of the SUM over the expression: it streams the same
bytes through the existing kernels.  Device time is the library's HIP-event total (pg_exec_stats.device_ms_total — for an expression query:
the ordinary part, the filter pass and the accumulation pass; the bounds pass runs once per segment and expression, in the warm-up, and is
reported on its own line); the fraction of 8 TB/s comes from pg_exec_stats.algorithmic_bytes.  Prints one line per query (median of --reps
alternated runs) and the ratio of every expression query to its twin:
  * SUM(m * r_int), no filter, no GROUP BY;
  * config 3's filter, GROUP BY g1;
  * config 3's filter, GROUP BY g1, g2.
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
    "expr_plain": "SELECT SUM(m * r_int) FROM gpuBench",
    "expr_plain_twin": "SELECT SUM(m), SUM(r_int) FROM gpuBench",
    "expr_cfg3_g1": f"SELECT g1, SUM(m * r_int) FROM gpuBench {WHERE} GROUP BY g1 LIMIT 100000",
    "expr_cfg3_g1_twin": f"SELECT g1, SUM(m), SUM(r_int) FROM gpuBench {WHERE} GROUP BY g1 LIMIT 100000",
    "expr_cfg3_g1g2": f"SELECT g1, g2, SUM(m * r_int) FROM gpuBench {WHERE} GROUP BY g1, g2 LIMIT 100000",
    "expr_cfg3_g1g2_twin": f"SELECT g1, g2, SUM(m), SUM(r_int) FROM gpuBench {WHERE} GROUP BY g1, g2 LIMIT 100000",
}
TWIN = {n: n + "_twin" for n in QUERIES if not n.endswith("_twin")}

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=1_000_000_000)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--only", default="", help="comma-separated query names (e.g. for a rocprofv3 run of one kernel)")
args = ap.parse_args()

api = capi.gpu_api()
api.call("init", 0)
seg = NativeSegment(api, HostSegment("prof_expr", args.docs))
for name in ["c_inv1", "c_inv2", "r_int", "g1", "g2", "m"]:
    one = synth.generate_segment(args.docs, columns=[name])
    seg.add_column(one.columns[name], keep_host_buffers=False)
    print(f"# column {name} registered", flush=True)

names = [n for n in QUERIES if not args.only or n in args.only.split(",")]
qcs = {n: parse_sql(QUERIES[n]) for n in names}
skipped = {}
first = {}
for n in list(names):
    qcs[n].num_groups_limit = 2_000_000_000
    try:
        t0 = time.perf_counter()
        seg.execute(qcs[n], profile=True)   # warm-up: plans, virtual dictionaries, the bounds pass of the expression
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

print(f"# prof_expr: {args.docs} docs, {args.reps} alternated reps, medians")
med = {}
for n in names:
    st = last[n].stats
    med[n] = statistics.median(dev[n])
    frac = st.algorithmic_bytes / (med[n] * 1e-3) / 8e12 if med[n] > 0 else 0.0
    print(f"{n:20s} device_ms {med[n]:9.3f}  wall_ms {statistics.median(wall[n]):9.3f}  first_run_wall_ms {first[n]:9.3f}  groups {last[n].num_groups:6d}  "
          f"kernel {st.kernel.decode():24s} docs_scanned {st.num_docs_scanned:11d}  algorithmic_bytes {st.algorithmic_bytes:12d}  "
          f"frac_of_8TBps {frac:.3f}  query: {QUERIES[n]}")
for n, why in skipped.items():
    print(f"{n:20s} refused: {why}")
for n, t in TWIN.items():
    if n in med and t in med and med[t] > 0:
        print(f"ratio {n} / {t} device time: {med[n] / med[t]:.3f}; wall time: {statistics.median(wall[n]) / statistics.median(wall[t]):.3f}")
seg.destroy()
