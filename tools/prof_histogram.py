"""HISTOGRAM against the twin the parent commit can already run on the same segment — COUNT(*) GROUP BY a precomputed INT column of the
bin ids —, alternated in one process (dev tool, not a test), in the manner of tools/prof_moments.py and DESIGN 4.10's protocol.

gpuBench's raw INT column m (uniform over [0, 2^20)) at 2 x 10^8 docs by default, next to `one`, a raw INT column that holds one value (every
doc in one bin: the case in which the 64 lanes of a wavefront pile onto one address).  No ratio is fixed in advance.  The shapes:
  * HISTOGRAM(x, 0, 2^20, B), no GROUP BY, B = 10 and 1 000, x = m (uniform) and x = one      (pg_hist_one)
  * the same grouped by g7, a 7-value column                                                  (pg_hist_lds)
  * the edge form at 1 001 edges (1 000 bins of unequal widths) over m, with and without g7   (pg_hist_one / pg_hist_lds, the edges in LDS)
and for each the twin `SELECT b, COUNT(*) ... GROUP BY [g7,] b` over the raw INT column b of the bin ids.
Then pg_hist_one with and without the in-wavefront combination on the same four inputs: PG_HIST_COMBINE_ROUNDS = 0 (plain LDS atomics, one
per doc), 1, 2, 4, 8, 16 and 64 (every distinct bin of a 64-doc word combined); the constant of pg_device.h is chosen from these lines.

Which number comes from where, and the order to read them in:
  1. device time: the library's HIP-event total (pg_exec_stats.device_ms_total: the ordinary part, the filter pass and the counting pass),
     median of --reps alternated runs with the profiler off, with its spread;
  2. the ratio to the twin, from the same alternated runs;
  3. the fraction of 8 TB/s: pg_exec_stats.algorithmic_bytes over the device time — a whole-query rate, not a kernel's share of peak;
  4. wall time last: it includes the host's planning and the joins.
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

HI = 1 << 20
ONE = 600_000

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=200_000_000)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--only", default="", help="comma-separated query names (e.g. for a rocprofv3 run of one kernel)")
args = ap.parse_args()
n = args.docs

# 1 001 edges of unequal widths over [0, 2^20]: a quadratic ramp, integers, strictly increasing
EDGES = np.unique(np.concatenate(([0], (np.arange(1, 1000) ** 2 * (HI / 1000.0 ** 2)).astype(np.int64) + np.arange(1, 1000), [HI]))).astype(np.int64)
assert len(EDGES) == 1001
EDGE_SQL = "ARRAY[" + ",".join(str(int(e)) for e in EDGES) + "]"

api = capi.gpu_api()
api.call("init", 0)
seg = NativeSegment(api, HostSegment("prof_histogram", n))


def add(name, values):
    seg.add_column(build_column(name, values, "INT", dictionary=False), keep_host_buffers=False)
    print(f"# column {name} registered: raw INT", flush=True)


m_host = synth.generate_segment(n, columns=["m"])
m = decode_column(m_host.columns["m"], n).astype(np.int64)
seg.add_column(m_host.columns["m"], keep_host_buffers=False)
print(f"# column m registered: min {int(m.min())}, max {int(m.max())}", flush=True)
assert 0 <= m.min() and m.max() < HI
for bins in (10, 1000):   # floor((x - 0) / binLength) in double, as getBinId forms it
    add(f"b{bins}_m", np.floor(m.astype(np.float64) / (HI / bins)).astype(np.int32))
    add(f"b{bins}_one", np.full(n, int(np.floor(ONE / (HI / bins))), dtype=np.int32))
add("be_m", (np.searchsorted(EDGES, m, side="right") - 1).astype(np.int32))
del m
add("one", np.full(n, ONE, dtype=np.int32))
seg.add_column(build_column("g7", (np.arange(n, dtype=np.int32) * 5 + 3) % 7, "INT"), keep_host_buffers=False)
print("# column g7 registered: dictionary INT, 7 values", flush=True)

QUERIES = {}
for x in ("m", "one"):
    for bins in (10, 1000):
        QUERIES[f"h{bins}({x})"] = f"SELECT HISTOGRAM({x}, 0, {HI}, {bins}) FROM gpuBench"
        QUERIES[f"h{bins}({x})_twin"] = f"SELECT b{bins}_{x}, COUNT(*) FROM gpuBench GROUP BY b{bins}_{x} LIMIT 100000"
        QUERIES[f"h{bins}_g7({x})"] = f"SELECT g7, HISTOGRAM({x}, 0, {HI}, {bins}) FROM gpuBench GROUP BY g7 LIMIT 100000"
        QUERIES[f"h{bins}_g7({x})_twin"] = f"SELECT g7, b{bins}_{x}, COUNT(*) FROM gpuBench GROUP BY g7, b{bins}_{x} LIMIT 100000"
QUERIES["hedges(m)"] = f"SELECT HISTOGRAM(m, {EDGE_SQL}) FROM gpuBench"
QUERIES["hedges(m)_twin"] = "SELECT be_m, COUNT(*) FROM gpuBench GROUP BY be_m LIMIT 100000"
QUERIES["hedges_g7(m)"] = f"SELECT g7, HISTOGRAM(m, {EDGE_SQL}) FROM gpuBench GROUP BY g7 LIMIT 100000"
QUERIES["hedges_g7(m)_twin"] = "SELECT g7, be_m, COUNT(*) FROM gpuBench GROUP BY g7, be_m LIMIT 100000"
TWIN = {q: q + "_twin" for q in QUERIES if not q.endswith("_twin")}

names = [q for q in QUERIES if not args.only or q in args.only.split(",")]
qcs = {q: parse_sql(QUERIES[q]) for q in names}
skipped, first = {}, {}
for q in list(names):
    qcs[q].num_groups_limit = 2_000_000_000
    try:
        t0 = time.perf_counter()
        seg.execute(qcs[q], profile=True)   # warm-up: plans, code objects, virtual dictionaries
        seg.execute(qcs[q], profile=True)
        first[q] = (time.perf_counter() - t0) * 1e3
    except capi.NativeError as e:          # a refusal is a result of the measurement too
        skipped[q] = e.message
        names.remove(q)
    print(f"# warmed up {q}", flush=True)
dev = {q: [] for q in names}
wall = {q: [] for q in names}
last = {}
for _ in range(args.reps):
    for q in names:   # alternated: the twins see the same clocks and caches
        t0 = time.perf_counter()
        rb = seg.execute(qcs[q], profile=True)
        wall[q].append((time.perf_counter() - t0) * 1e3)
        dev[q].append(rb.stats.device_ms_total)
        last[q] = rb


def show(q):
    return QUERIES[q] if len(QUERIES[q]) < 200 else QUERIES[q][:90] + " ... " + QUERIES[q][-60:]


print(f"# prof_histogram: {n} docs, {args.reps} alternated reps, medians")
med = {}
for q in names:
    st = last[q].stats
    med[q] = statistics.median(dev[q])
    frac = st.algorithmic_bytes / (med[q] * 1e-3) / 8e12 if med[q] > 0 else 0.0
    print(f"{q:22s} device_ms {med[q]:9.3f}  (min {min(dev[q]):.3f}, max {max(dev[q]):.3f})  aggregate_ms {st.device_ms_aggregate:9.3f}  wall_ms {statistics.median(wall[q]):9.3f}  "
          f"warm_up_wall_ms {first[q]:9.3f}  groups {last[q].num_groups:6d}  kernel {st.kernel.decode():24s} docs_scanned {st.num_docs_scanned:11d}  "
          f"algorithmic_bytes {st.algorithmic_bytes:12d}  frac_of_8TBps {frac:.3f}  query: {show(q)}")
for q, why in skipped.items():
    print(f"{q:22s} refused: {why}")
for q, t in TWIN.items():
    if q in med and t in med and med[t] > 0:
        print(f"ratio {q} / {t} device time: {med[q] / med[t]:.3f}; wall time: {statistics.median(wall[q]) / statistics.median(wall[t]):.3f}")

# ---- pg_hist_one with and without the in-wavefront combination ----------------------------------------------------------------------------------
ONE_KERNEL = [q for q in ("h10(m)", "h1000(m)", "h10(one)", "h1000(one)", "hedges(m)") if q in names]
ROUNDS = (0, 1, 2, 4, 8, 16, 64)
print("# pg_hist_one by PG_HIST_COMBINE_ROUNDS (0: one plain LDS atomic per doc; r: the first r distinct bins of a 64-doc word combined, the rest plain atomics)")
table = {q: {} for q in ONE_KERNEL}
for _ in range(max(3, args.reps // 2)):
    for r in ROUNDS:   # alternated over the settings as well
        os.environ["PG_HIST_COMBINE_ROUNDS"] = str(r)
        api.call("options_reload")
        for q in ONE_KERNEL:
            rb = seg.execute(qcs[q], profile=True)
            assert rb.stats.kernel.decode() == "pg_hist_one"
            table[q].setdefault(r, []).append(rb.stats.device_ms_aggregate)
os.environ.pop("PG_HIST_COMBINE_ROUNDS")
api.call("options_reload")
for q in ONE_KERNEL:
    print(f"{q:22s} aggregate_ms by rounds: " + "  ".join(f"{r}: {statistics.median(table[q][r]):.3f}" for r in ROUNDS))
seg.destroy()
