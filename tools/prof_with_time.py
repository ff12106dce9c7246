"""LASTWITHTIME against its twin MAX(ts) + COUNT on one synthetic segment, alternated in one process (dev tool, not a test), in the manner of
tools/prof_variance.py and DESIGN 4.10's protocol.

gpuBench at 2 x 10^8 docs by default, with an event-time column added: ts, raw LONG, epoch milliseconds over about eleven days (packed
mode, pg_with_time.h).  The twin of every query is `MAX(ts), COUNT(*)` of the same shape: it streams the same bytes through the existing
kernels with the same number of atomics, so near parity is expected — an expectation, not a bar.  Three shapes:
  * LASTWITHTIME(m, ts, 'INT'), no filter, no GROUP BY      (pg_wt_reg)
  * LASTWITHTIME(m, ts, 'INT') GROUP BY g1                  (pg_wt_lds: 100 groups x 1 slot)
  * config 3's filter, GROUP BY g1                          (pg_wt_lds behind the filter's match words)
and, with --wide, the same over ts_wide, a raw LONG column that spans the whole LONG range (wide mode: two passes' worth expected).

Which number comes from where, and the order to read them in:
  1. kernel time: a kernel trace in a run of its own —
         rocprofv3 --kernel-trace --stats -d DIR -- python tools/prof_with_time.py --reps 3
     (pg_wt_reg / pg_wt_lds / pg_wt_gather by their stable names); tracing slows the host, so nothing else is read from that run;
  2. device time: the library's HIP-event total (pg_exec_stats.device_ms_total: the ordinary part, the filter pass and the arg-max
     passes with their gather), median of --reps alternated runs with the profiler off, with its spread;
  3. the ratio to the twin, from the same alternated runs;
  4. the fraction of 8 TB/s: pg_exec_stats.algorithmic_bytes over the device time — a whole-query rate, not a kernel's share of peak;
  5. wall time last: it includes the host's planning and the joins.
The lines go to stdout; kept as profiles/with_time_prof.txt they are what DESIGN 4.11 quotes.
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
from pinot_amd.segment import HostSegment, build_column  # noqa: E402

WHERE = "WHERE c_inv1 IN (0,1,2,3) AND c_inv2 IN (0,1) AND r_int BETWEEN 250000 AND 749999"


def queries(t):
    return {
        f"wt_plain({t})": f"SELECT LASTWITHTIME(m, {t}, 'INT') FROM gpuBench",
        f"wt_plain({t})_twin": f"SELECT MAX({t}), COUNT(*) FROM gpuBench",
        f"wt_g1({t})": f"SELECT g1, LASTWITHTIME(m, {t}, 'INT') FROM gpuBench GROUP BY g1 LIMIT 100000",
        f"wt_g1({t})_twin": f"SELECT g1, MAX({t}), COUNT(*) FROM gpuBench GROUP BY g1 LIMIT 100000",
        f"wt_cfg3_g1({t})": f"SELECT g1, LASTWITHTIME(m, {t}, 'INT') FROM gpuBench {WHERE} GROUP BY g1 LIMIT 100000",
        f"wt_cfg3_g1({t})_twin": f"SELECT g1, MAX({t}), COUNT(*) FROM gpuBench {WHERE} GROUP BY g1 LIMIT 100000",
    }


ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=200_000_000)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--wide", action="store_true", help="also over ts_wide, a raw LONG time column spanning the whole LONG range (wide mode)")
ap.add_argument("--only", default="", help="comma-separated query names (e.g. for a rocprofv3 run of one kernel)")
args = ap.parse_args()

api = capi.gpu_api()
api.call("init", 0)
seg = NativeSegment(api, HostSegment("prof_with_time", args.docs))
QUERIES = queries("ts")
for name in ["c_inv1", "c_inv2", "r_int", "g1", "m"]:
    seg.add_column(synth.generate_segment(args.docs, columns=[name]).columns[name], keep_host_buffers=False)
    print(f"# column {name} registered", flush=True)
rng = np.random.default_rng(7)
ts = 1_700_000_000_000 + rng.integers(0, 10**9, args.docs, dtype=np.int64)   # events out of order over about eleven days, ties included
seg.add_column(build_column("ts", ts, "LONG", dictionary=False), keep_host_buffers=False)
print("# column ts registered: raw LONG", flush=True)
if args.wide:
    wide = rng.integers(-2**63, 2**63 - 1, args.docs, dtype=np.int64)
    seg.add_column(build_column("ts_wide", wide, "LONG", dictionary=False), keep_host_buffers=False)
    QUERIES.update(queries("ts_wide"))
    print("# column ts_wide registered: raw LONG over the whole range", flush=True)
    del wide
del ts
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

print(f"# prof_with_time: {args.docs} docs, {args.reps} alternated reps, medians")
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
