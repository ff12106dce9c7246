"""Predicates over arithmetic expressions in WHERE on one synthetic segment (dev tool, not a test), in the manner of tools/prof_expr.py.

Three measurements:
  (a) the plan-time pass.  pg_expr_pred runs when a plan with an expression leaf is compiled, so every repetition is a query that differs only
      in its literal (a new plan, a new pass): `m * r_int > c` and `m - r_int > c` (c = 0: m > r_int).  Set against pg_expr_bounds — existing
      code doing the same loads and the same evaluation — over the same expression: the bounds pass is cached per text, so its repetitions are
      the spellings of the same work (times / mult, either operand order; minus / sub).  The kernels'
      own times come from a kernel trace of a --pass-only run, in a run of its own —
          rocprofv3 --kernel-trace -f csv -d DIR -- python tools/prof_expr_filter.py --pass-only
          python tools/kernel_trace_medians.py DIR     (dispatches, median / min / max per kernel: the first block of the profile file)
      — and the tool itself reports the wall time of the call that compiled the plan minus the median wall time of its cached repetitions.
  (b) the executed query: config 3's shape with the expression leaf AND-ed in against the same query without it — by default (the
      specialised kernel it would otherwise get) and with PG_FORCE_INTERPRETER (the interpreter kernels the leaf's PG_F_PUSH_WORDS forces),
      alternated in one process, medians of --reps runs, device time from pg_exec_stats.
  (c) plan compilation: wall time of the first and of the second execution of the query with the leaf.
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

CFG3 = "c_inv1 IN (0,1,2,3) AND c_inv2 IN (0,1) AND r_int BETWEEN 250000 AND 749999"
SELECT = "SELECT g1, COUNT(*), SUM(m) FROM gpuBench WHERE "
TAIL = " GROUP BY g1 LIMIT 100000"

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=1_000_000_000)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--pass-only", action="store_true", help="(a) alone: the run to put under a kernel trace")
args = ap.parse_args()

api = capi.gpu_api()
api.call("init", 0)
seg = NativeSegment(api, HostSegment("prof_expr_filter", args.docs))
col_bytes = {}
for name in (["r_int", "m"] if args.pass_only else ["c_inv1", "c_inv2", "r_int", "g1", "m"]):
    one = synth.generate_segment(args.docs, columns=[name])
    col_bytes[name] = len(one.columns[name].forward_index) if hasattr(one.columns[name].forward_index, "__len__") else 0
    seg.add_column(one.columns[name], keep_host_buffers=False)
    print(f"# column {name} registered ({col_bytes[name]} forward-index bytes)", flush=True)


def wall_ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def run_filter(where):
    ds = seg.filter("SELECT COUNT(*) FROM gpuBench WHERE " + where)
    st, card = ds.stats(), ds.cardinality()
    ds.free()
    return st, card


print(f"# prof_expr_filter: {args.docs} docs, {args.reps} repetitions, medians")
# ---- (a) the plan-time pass ------------------------------------------------------------------------------------------------------------------------
pass_bytes = col_bytes["m"] + col_bytes["r_int"] + args.docs // 8
for label, make in (("m * r_int > c", lambda i: f"m * r_int > {250_000_000_000 + i}"), ("m - r_int > c", lambda i: f"m - r_int > {i}")):
    first, cached, matches = [], [], []
    for i in range(args.reps):
        w = make(i)
        t_first, (st, card) = wall_ms(lambda: run_filter(w))    # compiles the plan: one pg_expr_pred pass over all docs
        t_again = statistics.median(wall_ms(lambda: run_filter(w))[0] for _ in range(3))
        first.append(t_first)
        cached.append(t_again)
        matches.append(card)
    est = statistics.median(a - b for a, b in zip(first, cached))
    print(f"(a) {label:16s} first_call_wall_ms {statistics.median(first):9.3f}  cached_call_wall_ms {statistics.median(cached):9.3f}  "
          f"difference_ms {est:9.3f}  (plan compilation + pg_expr_pred + its synchronise)  matches {matches[0]}  pass_algorithmic_bytes {pass_bytes}  "
          f"frac_of_8TBps_at_difference {pass_bytes / (est * 1e-3) / 8e12 if est > 0 else 0.0:.3f}")
for label, texts in (("bounds m * r_int", ["m * r_int", "mult(m, r_int)", "r_int * m", "mult(r_int, m)"]),
                     ("bounds m - r_int", ["m - r_int", "sub(m, r_int)"])):
    first, cached = [], []
    for text in texts:
        sql = f"SELECT SUM({text}) FROM gpuBench"
        try:
            t_first, _ = wall_ms(lambda: seg.execute(sql))        # the first execution of a new text: one pg_expr_bounds pass over all docs
            t_again = statistics.median(wall_ms(lambda: seg.execute(sql))[0] for _ in range(3))
        except capi.NativeError as e:
            print(f"(a) {label}: {text}: refused: {e.message}")
            continue
        first.append(t_first)
        cached.append(t_again)
    if first:
        est = statistics.median(a - b for a, b in zip(first, cached))
        print(f"(a) {label:16s} first_call_wall_ms {statistics.median(first):9.3f}  cached_call_wall_ms {statistics.median(cached):9.3f}  "
              f"difference_ms {est:9.3f}  (planning + pg_expr_bounds + its synchronise; {len(first)} spellings)")
if args.pass_only:
    seg.destroy()
    sys.exit(0)

# ---- (b) the executed query, (c) plan compilation ------------------------------------------------------------------------------------------------------
LEAF = "m * r_int > 250000000000"
variants = {
    "cfg3_and_leaf": (SELECT + CFG3 + " AND " + LEAF + TAIL, False),
    "cfg3_interpreter": (SELECT + CFG3 + TAIL, True),
    "cfg3_specialised": (SELECT + CFG3 + TAIL, False),
}


def knobs(force_interpreter):
    if force_interpreter:
        os.environ["PG_FORCE_INTERPRETER"] = "1"
    else:
        os.environ.pop("PG_FORCE_INTERPRETER", None)
    api.call("options_reload")


qcs = {}
first_wall, second_wall = {}, {}
for n, (sql, force) in variants.items():
    qcs[n] = parse_sql(sql)
    qcs[n].num_groups_limit = 2_000_000_000
    knobs(force)
    first_wall[n], _ = wall_ms(lambda: seg.execute(qcs[n], profile=True))
    second_wall[n], _ = wall_ms(lambda: seg.execute(qcs[n], profile=True))
dev = {n: [] for n in variants}
wall = {n: [] for n in variants}
last = {}
for _ in range(args.reps):
    for n, (sql, force) in variants.items():   # alternated: the variants see the same clocks and caches
        knobs(force)
        w, rb = wall_ms(lambda: seg.execute(qcs[n], profile=True))
        wall[n].append(w)
        dev[n].append(rb.stats.device_ms_total)
        last[n] = rb
knobs(False)
med = {}
for n in variants:
    st = last[n].stats
    med[n] = statistics.median(dev[n])
    frac = st.algorithmic_bytes / (med[n] * 1e-3) / 8e12 if med[n] > 0 else 0.0
    print(f"(b) {n:18s} device_ms {med[n]:9.3f}  wall_ms {statistics.median(wall[n]):9.3f}  kernel {st.kernel.decode():24s} docs_scanned {st.num_docs_scanned:11d}  "
          f"entries_in_filter {st.num_entries_scanned_in_filter:11d} exact {st.stats_exact}  algorithmic_bytes {st.algorithmic_bytes:12d}  frac_of_8TBps {frac:.3f}")
if med["cfg3_interpreter"] > 0 and med["cfg3_specialised"] > 0:
    print(f"(b) leaf / interpreter without it: {med['cfg3_and_leaf'] / med['cfg3_interpreter']:.3f}   (one more word stream)")
    print(f"(b) interpreter / specialised kernel, both without the leaf: {med['cfg3_interpreter'] / med['cfg3_specialised']:.3f}   (the follow-up's gap)")
print(f"(c) cfg3_and_leaf: first execution wall_ms {first_wall['cfg3_and_leaf']:.3f} (plan compilation with the pass), second {second_wall['cfg3_and_leaf']:.3f}; "
      f"cfg3 without the leaf: first {first_wall['cfg3_specialised']:.3f}, second {second_wall['cfg3_specialised']:.3f}")
seg.destroy()
