"""GROUP BY over arithmetic expressions on one synthetic segment (dev tool, not a test), in the manner of tools/prof_expr_filter.py.

The twins of `m - r_int` and `m * r_int` are stored raw DOUBLE columns holding the same values (`k_sub*`, `k_mul*`): grouping by them runs
code this feature does not touch (ensure_virtual_dictionary over a stored column, the same group-by kernels).  gpuBench at 2 x 10^8 docs by
default: the virtual dictionary's sort works in 24 B/doc.

Two measurements:
  (a) the first-use build.  pg_query_supported over `GROUP BY <key>` builds the key's virtual dictionary and compiles the plan without running
      it: wall time of the first call minus the median of its cached repetitions.  An expression's column is cached per text, so its
      repetitions are the spellings of the same work (minus / sub; times / mult in either operand order); a stored column's virtual
      dictionary is built once per column, so the twin is registered --twin-copies times under different names.  The kernels' own times
      come from a kernel trace of a --build-only run, in a run of its own —
          rocprofv3 --kernel-trace -f csv -d DIR -- python tools/prof_expr_keys.py --build-only
          python tools/kernel_trace_medians.py DIR
      (pg_expr_keys against pg_vdict_keys_kernel; the sort, unique, id and pack kernels are the same code on both sides).
  (b) the steady-state query: config 3's filter with GROUP BY m - r_int against the same query grouped by the twin, alternated in one
      process, medians of --reps runs, device time from pg_exec_stats, the kernel's name from the same place.
"""
import argparse
import dataclasses
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401,E402  (initialises the ROCm runtime as bench.py does)
from pinot_amd import capi, synth  # noqa: E402
from pinot_amd.executor import NativeSegment  # noqa: E402
from pinot_amd.query import CQuery, parse_sql  # noqa: E402
from pinot_amd.segment import HostSegment, build_column, decode_column  # noqa: E402

CFG3 = "c_inv1 IN (0,1,2,3) AND c_inv2 IN (0,1) AND r_int BETWEEN 250000 AND 749999"

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=200_000_000)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--twin-copies", type=int, default=3)
ap.add_argument("--build-only", action="store_true", help="(a) alone: the run to put under a kernel trace")
args = ap.parse_args()

api = capi.gpu_api()
api.call("init", 0)
seg = NativeSegment(api, HostSegment("prof_expr_keys", args.docs))
values = {}
for name in (["r_int", "m"] if args.build_only else ["c_inv1", "c_inv2", "r_int", "m"]):
    one = synth.generate_segment(args.docs, columns=[name])
    if name in ("r_int", "m"):
        values[name] = decode_column(one.columns[name], args.docs).astype(np.float64)
    seg.add_column(one.columns[name], keep_host_buffers=False)
    print(f"# column {name} registered", flush=True)
for twin, v in (("k_sub", values["m"] - values["r_int"]), ("k_mul", values["m"] * values["r_int"])):
    col = build_column(twin, v, "DOUBLE", dictionary=False)
    for i in range(args.twin_copies):
        seg.add_column(dataclasses.replace(col, name=f"{twin}{i}"), keep_host_buffers=True)
    col.forward_index = None
    print(f"# twin {twin}0..{args.twin_copies - 1} registered: raw DOUBLE", flush=True)
values.clear()


def wall_ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def supported(key):
    qc = parse_sql(f"SELECT {key}, COUNT(*) FROM gpuBench GROUP BY {key} LIMIT 10")
    qc.num_groups_limit = 2_000_000_000
    cq = CQuery(qc)
    return lambda: api.call("query_supported", seg.handle, cq.ptr())


print(f"# prof_expr_keys: {args.docs} docs, {args.reps} repetitions, medians")
# ---- (a) the first-use build -------------------------------------------------------------------------------------------------------------------------
build = {}
for label, keys in (("m - r_int", ["m - r_int", "sub(m, r_int)"]), ("twin of m - r_int", [f"k_sub{i}" for i in range(args.twin_copies)]),
                    ("m * r_int", ["m * r_int", "mult(m, r_int)", "r_int * m", "mult(r_int, m)"]), ("twin of m * r_int", [f"k_mul{i}" for i in range(args.twin_copies)])):
    first, cached = [], []
    for key in keys:
        call = supported(key)
        t_first, _ = wall_ms(call)          # builds the key's virtual dictionary (key pass, sort, unique, ids, pack) and compiles the plan
        t_again = statistics.median(wall_ms(call)[0] for _ in range(3))
        first.append(t_first)
        cached.append(t_again)
    build[label] = statistics.median(a - b for a, b in zip(first, cached))
    print(f"(a) {label:18s} first_call_wall_ms {statistics.median(first):9.3f}  cached_call_wall_ms {statistics.median(cached):9.3f}  "
          f"difference_ms {build[label]:9.3f}  ({len(keys)} builds; min {min(a - b for a, b in zip(first, cached)):.3f}, max {max(a - b for a, b in zip(first, cached)):.3f})")
for e in ("m - r_int", "m * r_int"):
    print(f"(a) build of {e} / build of its twin: {build[e] / build['twin of ' + e]:.3f}")
print(f"(a) device bytes of the segment after the builds: {seg.device_bytes()}")
if args.build_only:
    seg.destroy()
    sys.exit(0)

# ---- (b) the steady-state query ------------------------------------------------------------------------------------------------------------------------
variants = {"group_by_expression": "m - r_int", "group_by_twin": "k_sub0"}
qcs = {}
for n, key in variants.items():
    qcs[n] = parse_sql(f"SELECT {key}, COUNT(*), SUM(m) FROM gpuBench WHERE {CFG3} GROUP BY {key} LIMIT 100000")
    qcs[n].num_groups_limit = 2_000_000_000
    seg.execute(qcs[n], profile=True)
    seg.execute(qcs[n], profile=True)
dev = {n: [] for n in variants}
wall = {n: [] for n in variants}
last = {}
for _ in range(args.reps):
    for n in variants:   # alternated: the variants see the same clocks and caches
        w, rb = wall_ms(lambda: seg.execute(qcs[n], profile=True))
        wall[n].append(w)
        dev[n].append(rb.stats.device_ms_total)
        last[n] = rb
for n in variants:
    st = last[n].stats
    print(f"(b) {n:20s} device_ms {statistics.median(dev[n]):9.3f}  (min {min(dev[n]):.3f}, max {max(dev[n]):.3f})  wall_ms {statistics.median(wall[n]):9.3f}  "
          f"kernel {st.kernel.decode():24s} groups {last[n].num_groups:9d}  docs_scanned {st.num_docs_scanned:11d}  entries_post_filter {st.num_entries_scanned_post_filter:11d}")
print(f"(b) expression / twin: {statistics.median(dev['group_by_expression']) / statistics.median(dev['group_by_twin']):.3f}")
seg.destroy()
