"""KURTOSIS against its twin STDDEV_POP on one synthetic segment, alternated in one process (dev tool, not a test), in the manner of
tools/prof_variance.py and DESIGN 4.10's protocol.

gpuBench at 2 x 10^8 docs by default.  The twin of every query is `STDDEV_POP(m)` of the same shape: it streams the same bytes through
pg_var_* with 4 slot updates per doc on the integer path (m is a raw INT column) against 11 here, so a multiple is expected, not parity;
no ratio is fixed in advance.  Three shapes:
  * KURTOSIS(m), no filter, no GROUP BY      (pg_moment_reg)
  * KURTOSIS(m) GROUP BY g1                  (pg_moment_lds: 100 groups x 11 slots)
  * config 3's filter, GROUP BY g1           (pg_moment_lds behind the filter's match words)
and, with --double, the same over a raw DOUBLE copy of m (the double path: 1 + 4 + 6 + 9 + 12 slots, against the twin's 1 + 4 + 6).

Which number comes from where, and the order to read them in:
  1. kernel time: a kernel trace in a run of its own —
         rocprofv3 --kernel-trace --stats -d DIR -- python tools/prof_moments.py --reps 3
     (pg_moment_reg / pg_moment_lds and pg_var_reg / pg_var_lds by their stable names); tracing slows the host, so nothing else is read
     from that run;
  2. device time: the library's HIP-event total (pg_exec_stats.device_ms_total: the ordinary part, the filter pass and the accumulation
     pass), median of --reps alternated runs with the profiler off, with its spread;
  3. the ratio to the twin, from the same alternated runs;
  4. the fraction of 8 TB/s: pg_exec_stats.algorithmic_bytes over the device time — a whole-query rate, not a kernel's share of peak;
  5. wall time last: it includes the host's planning, the wide-integer finalisation and the joins.
"""
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
from pinot_amd.segment import HostSegment, build_column, decode_column  # noqa: E402

WHERE = "WHERE c_inv1 IN (0,1,2,3) AND c_inv2 IN (0,1) AND r_int BETWEEN 250000 AND 749999"


def queries(col):
    return {
        f"m4_plain({col})": f"SELECT KURTOSIS({col}) FROM gpuBench",
        f"m4_plain({col})_twin": f"SELECT STDDEV_POP({col}) FROM gpuBench",
        f"m4_g1({col})": f"SELECT g1, KURTOSIS({col}) FROM gpuBench GROUP BY g1 LIMIT 100000",
        f"m4_g1({col})_twin": f"SELECT g1, STDDEV_POP({col}) FROM gpuBench GROUP BY g1 LIMIT 100000",
        f"m4_cfg3_g1({col})": f"SELECT g1, KURTOSIS({col}) FROM gpuBench {WHERE} GROUP BY g1 LIMIT 100000",
        f"m4_cfg3_g1({col})_twin": f"SELECT g1, STDDEV_POP({col}) FROM gpuBench {WHERE} GROUP BY g1 LIMIT 100000",
    }


ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=200_000_000)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--double", action="store_true", help="also over m_f64, a raw DOUBLE copy of m (the double path)")
ap.add_argument("--only", default="", help="comma-separated query names (e.g. for a rocprofv3 run of one kernel)")
args = ap.parse_args()

api = capi.gpu_api()
api.call("init", 0)
seg = NativeSegment(api, HostSegment("prof_moments", args.docs))
QUERIES = queries("m")
for name in ["c_inv1", "c_inv2", "r_int", "g1", "m"]:
    one = synth.generate_segment(args.docs, columns=[name])
    if name == "m" and args.double:
        seg.add_column(build_column("m_f64", decode_column(one.columns[name], args.docs).astype(np.float64), "DOUBLE", dictionary=False), keep_host_buffers=False)
        QUERIES.update(queries("m_f64"))
        print("# column m_f64 registered: raw DOUBLE", flush=True)
    seg.add_column(one.columns[name], keep_host_buffers=False)
    print(f"# column {name} registered", flush=True)
TWIN = {n: n + "_twin" for n in QUERIES if not n.endswith("_twin")}

names = [n for n in QUERIES if not args.only or n in args.only.split(",")]
qcs = {n: parse_sql(QUERIES[n]) for n in names}
skipped, first = {}, {}
for n in list(names):
    qcs[n].num_groups_limit = 2_000_000_000
    try:
        t0 = time.perf_counter()
        seg.execute(qcs[n], profile=True)   # warm-up: plans, code objects
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

print(f"# prof_moments: {args.docs} docs, {args.reps} alternated reps, medians")
med = {}
for n in names:
    st = last[n].stats
    med[n] = statistics.median(dev[n])
    frac = st.algorithmic_bytes / (med[n] * 1e-3) / 8e12 if med[n] > 0 else 0.0
    print(f"{n:28s} device_ms {med[n]:9.3f}  (min {min(dev[n]):.3f}, max {max(dev[n]):.3f})  aggregate_ms {st.device_ms_aggregate:9.3f}  wall_ms {statistics.median(wall[n]):9.3f}  "
          f"warm_up_wall_ms {first[n]:9.3f}  groups {last[n].num_groups:6d}  kernel {st.kernel.decode():24s} docs_scanned {st.num_docs_scanned:11d}  "
          f"algorithmic_bytes {st.algorithmic_bytes:12d}  frac_of_8TBps {frac:.3f}  query: {QUERIES[n]}")
for n, why in skipped.items():
    print(f"{n:28s} refused: {why}")
for n, t in TWIN.items():
    if n in med and t in med and med[t] > 0:
        print(f"ratio {n} / {t} device time: {med[n] / med[t]:.3f}; wall time: {statistics.median(wall[n]) / statistics.median(wall[t]):.3f}")
seg.destroy()
