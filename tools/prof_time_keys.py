"""GROUP BY over time-bucket transforms on one synthetic segment (dev tool, not a test), in the manner of tools/prof_expr_keys.py.

gpuBench at 2 x 10^8 docs by default with a raw LONG millisecond column `ts_ms` added (2001-08-22T03:04:05.321Z + r_int minutes + m
milliseconds: about 1.9 years of instants).  The twin of each text is a stored raw LONG column holding the same values: grouping by it runs
code this feature does not touch (ensure_virtual_dictionary over a stored column, the same group-by kernels).

Two measurements per text:
  (a) the first-use build.  pg_query_supported over `GROUP BY <key>` builds the key's virtual dictionary and compiles the plan without running
      it: wall time of the first call minus the median of its cached repetitions.  A time key's column is cached per text, so its repetitions
      are other texts of the same work (a default argument spelled out, a unit name in another case); the twin is registered --twin-copies
      times under different names.  The kernels' own times come from a kernel trace of a --build-only run, in a run of its own —
          rocprofv3 --kernel-trace -f csv -d DIR -- python tools/prof_time_keys.py --build-only
          python tools/kernel_trace_medians.py DIR
      (pg_time_keys against pg_vdict_keys_kernel; the sort, unique, id and pack kernels are the same code on both sides).
  (b) the steady-state query: config 3's filter with GROUP BY <text>, COUNT(*), SUM(m) against the same query grouped by the twin, alternated
      in one process, medians of --reps runs, device time from pg_exec_stats, the kernel's name from the same place.
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
BASE_MS = 998449445321


def trunc_div(x, d):
    return np.where(x < 0, -((-x) // d), x // d)


def month_floor(x):
    return x.astype("datetime64[ms]").astype("datetime64[M]").astype("datetime64[ms]").astype(np.int64)


# label: (spellings of the same work, the values in numpy)
KEYS = {
    "toepochhours": (["toEpochHours(ts_ms)", "timeConvert(ts_ms,'MILLISECONDS','HOURS')", "timeConvert(ts_ms,'milliseconds','hours')"],
                     lambda x: trunc_div(x, 3_600_000)),
    "datetrunc day": (["dateTrunc('day', ts_ms)", "dateTrunc('DAY', ts_ms)", "dateTrunc('day', ts_ms, 'MILLISECONDS')"], lambda x: x // 86_400_000 * 86_400_000),
    "datetrunc month": (["dateTrunc('month', ts_ms)", "dateTrunc('MONTH', ts_ms)", "dateTrunc('month', ts_ms, 'MILLISECONDS')"], month_floor),
    "datetimeconvert 15 min": (["dateTimeConvert(ts_ms,'1:MILLISECONDS:EPOCH','1:MILLISECONDS:EPOCH','15:MINUTES')",
                                "dateTimeConvert(ts_ms,'EPOCH|MILLISECONDS','1:MILLISECONDS:EPOCH','15:MINUTES')",
                                "dateTimeConvert(ts_ms,'1:MILLISECONDS:EPOCH','EPOCH|MILLISECONDS','MINUTES|15')"], lambda x: trunc_div(x, 900_000) * 900_000),
}

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=200_000_000)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--twin-copies", type=int, default=2)
ap.add_argument("--build-only", action="store_true", help="(a) alone: the run to put under a kernel trace")
args = ap.parse_args()

api = capi.gpu_api()
api.call("init", 0)
seg = NativeSegment(api, HostSegment("prof_time_keys", args.docs))
values = {}
for name in (["r_int", "m"] if args.build_only else ["c_inv1", "c_inv2", "r_int", "m"]):
    one = synth.generate_segment(args.docs, columns=[name])
    if name in ("r_int", "m"):
        values[name] = decode_column(one.columns[name], args.docs).astype(np.int64)
    if not (args.build_only and name == "r_int"):
        seg.add_column(one.columns[name], keep_host_buffers=False)
    print(f"# column {name} registered", flush=True)
ts = BASE_MS + values["r_int"] * 60_000 + values["m"]
values.clear()
seg.add_column(build_column("ts_ms", ts, "LONG", dictionary=False), keep_host_buffers=False)
print("# column ts_ms registered: raw LONG", flush=True)
twin_of = {}
for i, (label, (_, fn)) in enumerate(KEYS.items()):
    col = build_column(f"k{i}_", fn(ts).astype(np.int64), "LONG", dictionary=False)
    for c in range(args.twin_copies):
        seg.add_column(dataclasses.replace(col, name=f"k{i}_{c}"), keep_host_buffers=True)
    col.forward_index = None
    twin_of[label] = [f"k{i}_{c}" for c in range(args.twin_copies)]
    print(f"# twin of {label} registered: raw LONG, {args.twin_copies} copies", flush=True)
del ts


def wall_ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def supported(key):
    qc = parse_sql(f"SELECT {key}, COUNT(*) FROM gpuBench GROUP BY {key} LIMIT 10")
    qc.num_groups_limit = 2_000_000_000
    cq = CQuery(qc)
    return lambda: api.call("query_supported", seg.handle, cq.ptr())


print(f"# prof_time_keys: {args.docs} docs, {args.reps} repetitions, medians")
# ---- (a) the first-use build -------------------------------------------------------------------------------------------------------------------------
for label, (spellings, _) in KEYS.items():
    build = {}
    for who, keys in ((label, spellings), ("twin of " + label, twin_of[label])):
        first, cached = [], []
        for key in keys:
            call = supported(key)
            t_first, _ = wall_ms(call)          # builds the key's virtual dictionary (key pass, sort, unique, ids, pack) and compiles the plan
            first.append(t_first)
            cached.append(statistics.median(wall_ms(call)[0] for _ in range(3)))
        diffs = [a - b for a, b in zip(first, cached)]
        build[who] = statistics.median(diffs)
        print(f"(a) {who:32s} first_call_wall_ms {statistics.median(first):9.3f}  cached_call_wall_ms {statistics.median(cached):9.3f}  "
              f"difference_ms {build[who]:9.3f}  ({len(keys)} builds; min {min(diffs):.3f}, max {max(diffs):.3f})", flush=True)
    print(f"(a) build of {label} / build of its twin: {build[label] / build['twin of ' + label]:.3f}")
print(f"(a) device bytes of the segment after the builds: {seg.device_bytes()}")
if args.build_only:
    seg.destroy()
    sys.exit(0)

# ---- (b) the steady-state query ------------------------------------------------------------------------------------------------------------------------
for label, (spellings, _) in KEYS.items():
    variants = {"group_by_time_key": spellings[0], "group_by_twin": twin_of[label][0]}
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
        print(f"(b) {label:24s} {n:18s} device_ms {statistics.median(dev[n]):9.3f}  (min {min(dev[n]):.3f}, max {max(dev[n]):.3f})  wall_ms {statistics.median(wall[n]):9.3f}  "
              f"kernel {st.kernel.decode():24s} groups {last[n].num_groups:9d}  docs_scanned {st.num_docs_scanned:11d}  entries_post_filter {st.num_entries_scanned_post_filter:11d}")
    print(f"(b) {label}: time key / twin: {statistics.median(dev['group_by_time_key']) / statistics.median(dev['group_by_twin']):.3f}", flush=True)
seg.destroy()
