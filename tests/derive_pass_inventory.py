"""The three DERIVE passes — kernels that leave a cached per-doc product behind instead of an aggregate — tied to queries that run them on
segments larger than their launch grid:

  pg_expr_pred   pg_kernels_exprpred.hip, launched by expr_leaf_run (pg_plan.cpp): the match words of an arithmetic predicate in WHERE
  pg_expr_keys   pg_kernels_exprkey.hip, launched by expression_virtual_dictionary (pg_vdict.hip): one DOUBLE key per doc of an expression key
  pg_time_keys   pg_kernels_timekey.hip, launched by time_virtual_dictionary (pg_vdict.hip): one LONG key per doc of a time-bucket key

All three walk 64-doc words grid-stride, PG_EXPR_PRED_WORDS words per wavefront and iteration, under one grid cap; below the WRAP POINT — cap x
words per workgroup x 64 docs — no wavefront takes a second step.  launch_constants() reads what decides it from the sources, wrap_point()
derives it for a device of `cus` compute units, scale_data() builds one segment per ladder size (tests/kernel_inventory.py), and the
references of the large sizes — vectorised numpy over the models of tests/expression_model.py, tests/expression_filter_model.py and
tests/time_transform_model.py — live here so that they run, and are timed, without a GPU.  tests/test_derive_pass_inventory.py holds the
entries to the wrap point on the CPU; tests/test_gpu_derive_scale.py runs them."""
import os
import re
from dataclasses import dataclass
from typing import Tuple

import numpy as np

from pinot_amd.query import parse_sql
from pinot_amd.segment import build_segment
from tests import expression_filter_model as fm
from tests import expression_model as em
from tests import percentile_model as pm
from tests import side_kernel_inventory as si
from tests import time_transform_model as tm
from tests.kernel_inventory import LADDER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pinot_amd", "csrc")
PASSES = ("pg_expr_pred", "pg_expr_keys", "pg_time_keys")
KERNEL_SOURCE = {"pg_expr_pred": "pg_kernels_exprpred.hip", "pg_expr_keys": "pg_kernels_exprkey.hip", "pg_time_keys": "pg_kernels_timekey.hip"}
# the function that launches each pass, and the file it stands in
LAUNCH_SITE = {"pg_expr_pred": ("pg_plan.cpp", "expr_leaf_run"), "pg_expr_keys": ("pg_vdict.hip", "expression_virtual_dictionary"),
               "pg_time_keys": ("pg_vdict.hip", "time_virtual_dictionary")}
ASSUMED_CUS = si.ASSUMED_CUS
SMALL, BIG = LADDER[0], LADDER[3]
DOCS_PER_WORD = 64
BAND_DOCS = 65536
HK_CARD, HK2_CARD = 65_537, 2**21 + 1      # 17-bit and 22-bit ids in the virtual dictionaries of add(hk,'0.5') and mult(hk2,'3')
POOL_MAX = 20_000                            # distinct instants per time source: the reference evaluates the model once per distinct value
GROUPS_LIMIT = 4_000_000                     # numGroupsLimit of the high-cardinality keys: above HK2_CARD and above the doc count
SELECTIVITY = (0.05, 0.95)


def _source(name: str) -> str:
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _function_body(text: str, name: str) -> str:
    """the source from the definition of `name` to the next definition at column 0"""
    m = re.search(r"^[A-Za-z_][^\n;]*\b%s\(" % re.escape(name), text, re.M)
    assert m, f"{name}: no such function any more"
    end = re.search(r"^}", text[m.start():], re.M)
    assert end, name
    return text[m.start():m.start() + end.end()]


def launch_constants() -> dict:
    """what decides how many docs one grid step of each pass covers, read from the sources"""
    c = {}
    (c["words_per_wave"],) = si._int(r"#define PG_EXPR_PRED_WORDS (\d+)\b", _source("pg_device.h"), "pg_device.h PG_EXPR_PRED_WORDS")
    for p in PASSES:
        k = _source(KERNEL_SOURCE[p])
        (c[p + ".bounds"],) = si._int(r"__launch_bounds__\((\d+)\) %s\(" % p, k, p + " __launch_bounds__")
        (c[p + ".threads"],) = si._int(r"hipLaunchKernelGGL\(%s, dim3\(grid\), dim3\((\d+)\), 0, stream" % p, k, p + " launch")
        assert re.search(r"constexpr int k\w+Words = PG_EXPR_PRED_WORDS;", k), p + ": the words per wavefront are no longer PG_EXPR_PRED_WORDS"
        path, fn = LAUNCH_SITE[p]
        body = _function_body(_source(path), fn)
        c[p + ".waves"], = si._int(r"const int64_t per_wg = (\d+) \* PG_EXPR_PRED_WORDS;", body, fn + " per_wg")
        c[p + ".per_wg"] = c[p + ".waves"] * c["words_per_wave"]
        (c[p + ".cap"],) = si._int(r"std::min<int64_t>\(\(int64_t\)device_cus\(seg\.device\) \* (\d+), \([\w.]*n_words \+ per_wg - 1\) / per_wg\)", body, fn + " grid")
    return c


def wrap_point(cus: int = ASSUMED_CUS, c: dict = None, kernel: str = "pg_expr_pred") -> int:
    """the docs one grid step of a pass covers on `cus` compute units: cus x cap x words per workgroup x 64"""
    c = c or launch_constants()
    return cus * c[kernel + ".cap"] * c[kernel + ".per_wg"] * DOCS_PER_WORD


# ---- the entries ------------------------------------------------------------------------------------------------------------------------------------------
# match shapes.  pg_expr_pred: the leaf alone, ANDed with an index leaf, ORed with a scan, under NOT, alone behind the upsert snapshot of
# kernel_inventory.snapshot_doc_ids, and through pg_filter_exec.  The key passes: every doc, the two filters of tests/side_kernel_inventory.py
# (sparse and spread; dense at the wrap and at the tail), and SELECT DISTINCT over every doc.
PRED_SHAPES = ("lone", "and", "or", "not", "snapshot", "filter")
KEY_SHAPES = ("all", "sparse", "dense", "distinct")
AND_WITH, OR_WITH = "c_inv1 IN (1, 5)", si.SPARSE
# side_kernel_inventory.dense_filter puts ~3 000 docs just past the point it is given and ~3 000 at the tail; given a point half a stretch
# before the wrap, its first stretch lies on both sides of it: the last words of the first grid step and the first words of the second
DENSE_BACK = 1500


@dataclass(frozen=True)
class Entry:
    kernel: str                                # the pass: a member of PASSES
    text: str                                  # pg_expr_pred: the predicate as SQL; the key passes: the key as SQL (its canonical text)
    shapes: Tuple[str, ...]
    sizes: Tuple[int, ...] = (SMALL, BIG)
    groups_limit: int = 0                      # numGroupsLimit, where the default would cut the key space
    twin: bool = False                         # the key has a twin raw column on the large segment too: its reference is the oracle over the twin

    def where(self, shape: str, n: int, wrap: int) -> str:
        if self.kernel == "pg_expr_pred":
            return {"and": f"{self.text} AND {AND_WITH}", "or": f"{self.text} OR {OR_WITH}", "not": f"NOT ({self.text})"}.get(shape, self.text)
        return {"sparse": si.SPARSE, "dense": si.dense_filter(n, wrap - DENSE_BACK)}.get(shape, "")

    def sql(self, shape: str, n: int, wrap: int) -> str:
        w = self.where(shape, n, wrap)
        if self.kernel == "pg_expr_pred":
            if shape == "filter":
                return "SELECT COUNT(*) FROM t WHERE " + w
            return f"SELECT band, COUNT(*), SUM(pos), MIN(pos), MAX(pos) FROM t WHERE {w} GROUP BY band"
        if shape == "distinct":
            return f"SELECT DISTINCT {self.text} FROM t ORDER BY {self.text} DESC LIMIT 1000"
        agg = "COUNT(*), SUM(s)" if self.kernel == "pg_time_keys" else "COUNT(*), SUM(pos)"
        return f"SELECT {self.text}, {agg} FROM t" + (" WHERE " + w if w else "") + f" GROUP BY {self.text}"

    def expression(self) -> str:
        """the canonical text of the expression the pass evaluates"""
        if self.kernel == "pg_expr_pred":
            return parse_sql("SELECT COUNT(*) FROM t WHERE " + self.text).filter.predicate.column
        return parse_sql(self.sql("all", SMALL, 0)).group_by[0]

    def predicate_kind(self) -> str:
        return parse_sql("SELECT COUNT(*) FROM t WHERE " + self.text).filter.predicate.type

    def sources(self):
        """the columns the pass loads per doc"""
        return tm.columns_of(self.expression()) if self.kernel == "pg_time_keys" else em.columns_of(self.expression())


EIGHT = "ri,rl,rf,rd,di,dd,s,c_inv1"
# 2^62 comes first in add()'s order (literals before columns): every partial sum is rounded to a multiple of 1 024 (512 below 2^62), so the eight columns,
# a few millions in all, give a few thousand keys — and every operand decides which
ROUNDED_SUM = f"add({EIGHT},'4611686018427387904')"

E = Entry
ENTRIES = [
    # ---- pg_expr_pred: every predicate kind; 1, 2, 3 and 8 operand columns ----
    E("pg_expr_pred", "ri * rd > 1000", ("lone", "and")),                                     # RANGE: raw INT x raw DOUBLE
    E("pg_expr_pred", "add(rf,di,dd) BETWEEN -200 AND 600", ("lone", "not")),                 # RANGE: raw FLOAT, dictionary INT, dictionary DOUBLE
    E("pg_expr_pred", "di + 2 = 5", ("lone", "or")),                                          # EQ: one column
    E("pg_expr_pred", "mult(dd,di) != 0", ("lone", "snapshot")),                              # NOT_EQ (0.0 and -0.0 both equal 0)
    E("pg_expr_pred", "di - c_inv1 IN (0, 1, -1, 2.5)", ("lone",)),                           # IN
    E("pg_expr_pred", "di - c_inv1 NOT IN (0, 1, -1)", ("lone",)),                            # NOT_IN
    E("pg_expr_pred", f"add({EIGHT}) > 0", ("lone", "filter")),                               # RANGE: eight columns, every operand kind
    # ---- pg_expr_keys ----
    E("pg_expr_keys", "sub(di,'7')", ("all",), twin=True),
    E("pg_expr_keys", "divide(ri,'1000')", ("all",), twin=True),
    E("pg_expr_keys", ROUNDED_SUM, ("all",), twin=True),
    E("pg_expr_keys", "add(di,c_inv1,band)", ("all",), twin=True),                             # three columns: a trip of the operand loop and its remainder
    E("pg_expr_keys", "add(hk,'0.5')", ("sparse", "dense", "distinct"), groups_limit=GROUPS_LIMIT),   # 17-bit ids
    E("pg_expr_keys", "mult(hk2,'3')", ("sparse", "dense", "all"), groups_limit=GROUPS_LIMIT),        # 22-bit ids; every doc's id, too
    # ---- pg_time_keys: one text per time_load kind and per family ----
    E("pg_time_keys", "toepochdays(ts)", ("all",)),                                            # raw LONG
    E("pg_time_keys", "toepochminutesrounded(tsd,'5')", ("all",)),                             # dictionary LONG
    E("pg_time_keys", "timeconvert(sec,'SECONDS','MILLISECONDS')", ("all",)),                  # raw INT
    E("pg_time_keys", "datetrunc('month',secd,'SECONDS','-03:30','DAYS')", ("all",)),          # dictionary INT
    E("pg_time_keys", "datetrunc('week',ts)", ("all",)),
    E("pg_time_keys", "toepochdays(uid)", ("sparse", "dense"), groups_limit=GROUPS_LIMIT),     # one key per doc: 22-bit ids
]
del E

RAW = ("pos", "ri", "rl", "rf", "rd", "ts", "sec", "uid", "hk", "hk2")
SCHEMA = {"rl": "LONG", "rf": "FLOAT", "rd": "DOUBLE", "dd": "DOUBLE", "ts": "LONG", "tsd": "LONG", "uid": "LONG"}
OPERAND_KINDS = {("raw", "INT"), ("raw", "LONG"), ("raw", "FLOAT"), ("raw", "DOUBLE"), ("dict", "INT"), ("dict", "DOUBLE")}   # expr_load's branches
TIME_KINDS = {("raw", "LONG"), ("dict", "LONG"), ("raw", "INT"), ("dict", "INT")}                                             # time_load's


def column_kind(col: str):
    return ("raw" if col in RAW else "dict", SCHEMA.get(col, "INT"))


def entries_of(kernel: str, n: int = None):
    return [e for e in ENTRIES if e.kernel == kernel and (n is None or n in e.sizes)]


# ---- the segment ------------------------------------------------------------------------------------------------------------------------------------------
YEAR_MS = 365 * tm.DAY_MS
# 0 and -1; the Monday 1970-01-05, 2001-01-01 and 2001-09-01 (UTC) and the millisecond before each; a quarter of an hour on either side of 0
PLANTED_MS = (0, -1, 4 * tm.DAY_MS, 4 * tm.DAY_MS - 1, 978_307_200_000, 978_307_199_999, 999_302_400_000, 999_302_399_999, -900_000, 900_000)
PLANTED_S = tuple(dict.fromkeys(v // 1000 for v in PLANTED_MS))      # the same instants in seconds (floor): 0 once


def _pool(rng, planted, near_zero, near_2001, centre, dtype):
    """at most POOL_MAX distinct instants, the planted ones first"""
    half = (POOL_MAX - len(planted)) // 2
    p = np.concatenate([np.asarray(planted, dtype=np.int64), rng.integers(-near_zero, near_zero, half), centre + rng.integers(-near_2001, near_2001, half)])
    p = p[np.sort(np.unique(p, return_index=True)[1])]
    assert len(p) <= POOL_MAX and p[:len(planted)].tolist() == list(planted)
    return p.astype(dtype)


def scale_columns(n: int, wrap: int = 2_097_152):
    """(data, schema) of `n` docs, without twins: the columns of scale_data as numpy arrays"""
    rng = np.random.default_rng(7919 + n)
    idx = np.arange(n, dtype=np.int64)
    sign = lambda: np.where(rng.integers(0, 2, n) == 0, -1.0, 1.0)   # noqa: E731
    pool_ms = _pool(rng, PLANTED_MS, 3 * YEAR_MS, 2 * YEAR_MS, 998_449_445_321, np.int64)
    pool_s = _pool(rng, PLANTED_S, 90_000_000, 40_000_000, 998_449_445, np.int32)
    data = {
        "pos": idx.astype(np.int32),                                             # raw: SUM / MIN / MAX(pos) pin which docs matched
        "band": (idx // BAND_DOCS).astype(np.int32),
        "s": rng.integers(0, 1000, n).astype(np.int32),                          # the selector of the sparse shape
        "c_inv1": rng.integers(0, 8, n).astype(np.int32),                        # inverted index
        "srt": (idx // 4).astype(np.int32),                                      # sorted: the dense shape's docId ranges
        "ri": rng.integers(-20_000, 20_000, n).astype(np.int32),
        "rl": rng.integers(-10**6, 10**6, n).astype(np.int64),
        "rf": (rng.uniform(0.5, 1000.0, n) * sign()).astype(np.float32),
        "rd": rng.uniform(1e-3, 1e3, n) * sign(),
        "di": rng.integers(-5, 6, n).astype(np.int32),
        "dd": rng.choice(np.array([0.1, -7.0, 1e-3, 123.456, 1e3]), n),
        "ts": pool_ms[rng.integers(0, len(pool_ms), n)],
        "tsd": pool_ms[rng.integers(0, 3000, n)],
        "sec": pool_s[rng.integers(0, len(pool_s), n)],
        "secd": pool_s[rng.integers(0, 3000, n)],
        "uid": (idx - n // 2) * 3 * tm.DAY_MS + 12_345,                          # one day per doc
        "hk": (rng.permutation(idx % HK_CARD) - 30_000).astype(np.int32),        # every value of the key space at least once
        "hk2": rng.permutation(idx % HK2_CARD).astype(np.int32),
    }
    if n > 64:
        data["s"][[0, 1, 2, 3, n - 5, n - 4, n - 3, n - 2]] = 7                  # the sparse shape reaches the first and the last word ...
        if n > wrap + 64:
            data["s"][[wrap - 1, wrap, wrap + 1]] = 7                            # ... and both sides of the wrap point
        data["rl"][rng.choice(n, 7, replace=False)] = 2**53 + 1                  # LONGs that are no doubles
        for col, planted in (("ts", PLANTED_MS), ("tsd", PLANTED_MS), ("sec", PLANTED_S), ("secd", PLANTED_S)):
            data[col][rng.choice(n, len(planted), replace=False)] = planted
    assert len(np.unique(data["hk"])) == min(n, HK_CARD) and len(np.unique(data["hk2"])) == min(n, HK2_CARD)
    schema = {c: SCHEMA.get(c, "INT") for c in data}
    return data, schema


def twin_name(i: int) -> str:
    return "tw%d" % i


def scale_data(n: int, wrap: int = 2_097_152):
    """(host segment, data, schema, twins) of `n` docs: the columns of scale_columns and, as in the three families' own modules, a raw twin
    column per expression — DOUBLE for an arithmetic text, LONG for a time text — holding the model's values.  The small segment has a twin
    for every entry (the families' _check helpers compare against them); the large ones only for the entries that say so."""
    data, schema = scale_columns(n, wrap)
    twins = {}
    for e in ENTRIES:
        if n not in e.sizes or not (n == SMALL or e.twin):
            continue
        text = e.expression()
        if text in twins:
            continue
        twins[text] = twin_name(len(twins))
        if e.kernel == "pg_time_keys":
            data[twins[text]], schema[twins[text]] = time_keys(text, data), "LONG"
        else:
            data[twins[text]], schema[twins[text]] = evaluate(text, data, schema), "DOUBLE"
    host = build_segment("derive_scale_%d" % n, data, schema, inverted_index_columns=["c_inv1"], no_dictionary_columns=list(RAW) + list(twins.values()))
    return host, data, schema, twins


# ---- references: numpy over the models, no GPU ----------------------------------------------------------------------------------------------------------
def evaluate(text, data, schema, docs=None):
    with np.errstate(all="ignore"):
        return np.asarray(em.evaluate(text, data, schema, docs), dtype=np.float64)


def time_keys(text, data, docs=None):
    """time_transform_model.evaluate — one Python call per value — over the DISTINCT values of the source, mapped back to the docs"""
    src = np.asarray(data[tm.columns_of(text)[0]])
    if docs is not None:
        src = src[docs]
    values, inverse = np.unique(src, return_inverse=True)
    return np.array(tm.evaluate(text, values), dtype=np.int64)[inverse]


def filter_mask(f, data, schema):
    """the doc set of a filter tree from the models' evaluators: expression leaves through expression_model.evaluate and
    expression_filter_model.apply_predicate, plain INT columns compared as numbers"""
    if f.type == "PREDICATE":
        p = f.predicate
        v = evaluate(p.column, data, schema) if "(" in p.column else np.asarray(data[p.column], dtype=np.float64)
        return fm.apply_predicate(v, p)
    ms = [filter_mask(c, data, schema) for c in f.children]
    if f.type == "NOT":
        return ~ms[0]
    out = ms[0]
    for m in ms[1:]:
        out = (out & m) if f.type == "AND" else (out | m)
    return out


def where_mask(where, data, schema, keep=None):
    """the docs `where` selects (every doc without one), behind the snapshot `keep` (docIds) if there is one"""
    n = len(data["pos"])
    mask = filter_mask(parse_sql("SELECT COUNT(*) FROM t WHERE " + where).filter, data, schema) if where else np.ones(n, dtype=bool)
    if keep is not None:
        kept = np.zeros(n, dtype=bool)
        kept[keep] = True
        mask = mask & kept
    return mask


def fold_bands(mask, data):
    """{band: [COUNT(*), SUM(pos), MIN(pos), MAX(pos)]} of the docs of `mask`, the intermediate results as the executor types them"""
    docs = np.flatnonzero(mask)
    band = np.asarray(data["band"])[docs]
    pos = np.asarray(data["pos"], dtype=np.int64)[docs]
    assert (np.diff(pos) > 0).all()                      # pos is the docId: a band's first doc is its MIN, its last its MAX
    bands, first, counts = np.unique(band, return_index=True, return_counts=True)
    last = first + counts - 1
    sums = np.add.reduceat(pos, first) if len(docs) else np.zeros(0, dtype=np.int64)
    assert int(sums.max(initial=0)) < 2**53
    return {(int(b),): [int(c), float(t), float(pos[i]), float(pos[j])] for b, c, t, i, j in zip(bands, counts, sums, first, last)}


def fold_keys(keys, weights):
    """(the distinct keys ascending, their doc counts, the exact integer sums of `weights` per key) of one int64 key per doc"""
    u, inverse, counts = np.unique(keys, return_inverse=True, return_counts=True)
    order = np.argsort(inverse, kind="stable")
    sums = np.add.reduceat(np.asarray(weights, dtype=np.int64)[order], np.concatenate(([0], np.cumsum(counts)[:-1]))) if len(u) else np.zeros(0, dtype=np.int64)
    assert int(np.abs(sums).max(initial=0)) < 2**53
    return u, counts.astype(np.int64), sums


def double_bits(v):
    """Double.doubleToLongBits as int64"""
    return fm.long_bits(v).view(np.int64)


def same_doubles(got, want) -> bool:
    """percentile_model.same_double over two arrays"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return False
    probe = range(0, len(got), max(1, len(got) // 50))
    assert all(pm.same_double(got[i], want[i]) == bool(double_bits(got[i:i + 1])[0] == double_bits(want[i:i + 1])[0]) for i in probe)
    return bool(np.array_equal(double_bits(got), double_bits(want)))
