"""SUM(CASE WHEN s > k THEN m ELSE 0 END) against its two twins on one synthetic segment, alternated in one process (dev tool, not a test),
in the manner of tools/prof_mode.py and tools/prof_expr.py:
  * the expression twin  SUM(m * r_int): the same side pass (pg_expr_reg / pg_expr_lds), the same number of operand columns, one
                         multiplication where the CASE has a comparison and a select;
  * the filter twin      SUM(m) WHERE r_int > k: what FilteredAggregationsTest holds the CASE equal to, through the fast-path kernels.
The condition column is r_int (raw INT, uniform over [0, 10^6)), k its median; no GROUP BY and GROUP BY g1.  No ratio is fixed in advance:
the expression pass is known to run well off its fast-path twins, and closing that gap is not this tool's subject.

Device time is the library's HIP-event total (pg_exec_stats.device_ms_total), medians of --reps alternated runs with their spread; the bounds
pass of an expression runs once per segment and text, in the warm-up."""
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

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=1_000_000_000)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--k", type=int, default=499_999)
args = ap.parse_args()

CASE = f"SUM(CASE WHEN r_int > {args.k} THEN m ELSE 0 END)"
QUERIES = {}
for shape, keys, tail in (("plain", "", ""), ("g1", "g1, ", " GROUP BY g1 LIMIT 100000")):
    QUERIES[f"{shape}_case"] = f"SELECT {keys}{CASE} FROM gpuBench{tail}"
    QUERIES[f"{shape}_expr_twin"] = f"SELECT {keys}SUM(m * r_int) FROM gpuBench{tail}"
    QUERIES[f"{shape}_filter_twin"] = f"SELECT {keys}SUM(m) FROM gpuBench WHERE r_int > {args.k}{tail}"

api = capi.gpu_api()
api.call("init", 0)
seg = NativeSegment(api, HostSegment("prof_case", args.docs))
for name in ["r_int", "g1", "m"]:
    seg.add_column(synth.generate_segment(args.docs, columns=[name]).columns[name], keep_host_buffers=False)
    print(f"# column {name} registered", flush=True)

qcs = {n: parse_sql(q) for n, q in QUERIES.items()}
names, skipped, first = list(QUERIES), {}, {}
for n in list(names):
    qcs[n].num_groups_limit = 2_000_000_000
    try:
        t0 = time.perf_counter()
        seg.execute(qcs[n], profile=True)   # warm-up: plans, code objects, the bounds pass of an expression
        first[n] = (time.perf_counter() - t0) * 1e3
        seg.execute(qcs[n], profile=True)
    except capi.NativeError as e:          # a refusal is a result of the measurement too
        skipped[n] = e.message
        names.remove(n)
    print(f"# warmed up {n}", flush=True)
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

print(f"# prof_case: {args.docs} docs, {args.reps} alternated reps, medians")
med = {}
for n in names:
    st = last[n].stats
    med[n] = statistics.median(dev[n])
    print(f"{n:18s} device_ms {med[n]:9.3f} (min {min(dev[n]):.3f}, max {max(dev[n]):.3f})  wall_ms {statistics.median(wall[n]):9.3f}  first_run_wall_ms {first[n]:9.3f}  "
          f"groups {last[n].num_groups:6d}  kernel {st.kernel.decode():22s} docs_scanned {st.num_docs_scanned:11d}  query: {QUERIES[n]}")
for n, why in skipped.items():
    print(f"{n:18s} refused: {why}")
for shape in ("plain", "g1"):
    c = f"{shape}_case"
    for t in (f"{shape}_expr_twin", f"{shape}_filter_twin"):
        if c in med and t in med and med[t] > 0:
            print(f"ratio {c} / {t} device time: {med[c] / med[t]:.3f}")
if "plain_case" in last and "plain_filter_twin" in last:   # the two are the same query: the same sum
    print(f"# plain_case = {last['plain_case'].aggregation_result()[0]!r}, plain_filter_twin = {last['plain_filter_twin'].aggregation_result()[0]!r}")
seg.destroy()
