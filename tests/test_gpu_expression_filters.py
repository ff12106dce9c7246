"""Predicates over arithmetic expressions in WHERE on the GPU path (the reference's ExpressionFilterOperator: add / sub / mult / div over
columns and literals, compared by the raw DOUBLE evaluators; `a > b` arrives as minus(a,b) > 0).  The oracle has no expressions, so every
expectation comes from two independent sources:
  * a TWIN query through the oracle: each segment also carries, for every expression under test, a raw DOUBLE column holding
    tests/expression_model.evaluate(text, ...); WHERE <expr> <pred> must give exactly the doc set, the groups and the intermediate results
    the oracle gives for WHERE <that column> <pred>  (IN / NOT_IN over +-0.0 or NaN excepted: the model pins those);
  * tests/expression_filter_model.py: the five predicate evaluators and the iterator automaton restated from the Java, for the doc set
    again and for numEntriesScannedInFilter.
Sizes: 1 doc; 65 (a second, partial 64-doc word); 2047 / 2049 (a partial last wave tile, a second wave tile); 10 001 (a second 10 000-doc
block of ExpressionScanDocIdIterator, one doc long); 30 011 (several blocks, a partial last one)."""
import copy
import os
import re

import numpy as np
import pytest

from pinot_amd import capi, formats
from pinot_amd.executor import NativeSegment
from pinot_amd.query import CQuery, FilterContext, Predicate, parse_sql
from pinot_amd.segment import build_column, build_mv_column, build_segment
from tests import expression_filter_model as fm
from tests import expression_model as em
from tests import percentile_model as pm
from tests.kernel_inventory import snapshot_doc_ids

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 65, 2047, 2049, 10001, 30011]
BIG = 30011

# ---- the WHERE clauses under test (every expression in them gets a twin column) ---------------------------------------------------------------
OPERANDS = [
    "ri * rd > 1000",                                             # raw INT x raw DOUBLE
    "add(di,dl) <= 0",                                            # dictionary INT + dictionary LONG
    "sub(rl,'1') >= 9007199254740991",                            # LONGs beyond 2^53: cast (double), then computed
    "rf / df BETWEEN -100 AND 100",                               # raw FLOAT, dictionary FLOAT
    "mult(dd,rd) < -0.5",                                         # dictionary DOUBLE, raw DOUBLE
    "1000000 - ri != 1000007",                                    # a literal on the left
    "rd / 3 > 100.25",                                            # ... and on the right
    "add(ri,'2.5',rd,'-1',dd) > 0",                               # literals between columns
    "plus(minus(ri,di),times(rd,divide(dd,rf))) <= 12.5",         # the aliases, nested
    "add(div(di,ri),div(dl,rl)) > 1",
    # 15 operations over 8 columns
    "add(mult(ri,di),sub(rd,dd),div(rf,df),mult(dl,'0.000001'),rl,ri,di,rd,dd) > 0",
]
PREDICATES = [
    "ri - di > 0", "ri - di >= 0", "ri - di < 0", "ri - di <= 0", "ri - di = 0", "ri - di != 0", "ri - di <> 7",
    "ri + di BETWEEN -100 AND 100",
    "ri + di NOT BETWEEN -100 AND 100",
    "ri - di IN (0, 1, -1, 2.5)", "ri - di NOT IN (0, 1, -1)",
    "10 < ri - di",                                                # PredicateComparisonRewriter: ri - di > 10
    "ri > di",                                                     # ... minus(ri,di) > 0
    "ri + 1 >= di * 2",
    "(ri + di) * 2 > 10",                                          # a leading '(' that opens an expression
    "(ri - di > 0 OR rd / 3 > 100.25) AND g3 = 1",                 # ... and one that opens a predicate group
]
NON_FINITE = [
    "div(di,z) > 5",            # +-Inf rows: +Inf matches
    "div(di,z) < -5",           # -Inf matches
    "div(di,z) != 0.3",         # everything, the infinities included
    "div(z,z) != 1",            # 0 / 0 = NaN: != is TRUE for NaN
    "div(z,z) = 1",             # NaN equals nothing
    "div(z,z) >= 0",            # ... and lies in no range
    "mult(pz,'1') = 0",         # 0.0 and -0.0 both equal '0'
    "mult(pz,'1') != 0",
    "mult(pz,'1') >= 0",        # -0.0 >= 0.0
]
MODEL_ONLY = [                   # IN / NOT_IN over +-0.0 and NaN: DoubleOpenHashSet compares bit patterns (no twin: the oracle's raw scan compares numbers)
    "mult(pz,'1') IN (0)",       # +0.0 only
    "mult(pz,'1') IN ('-0.0')",  # -0.0 only
    "mult(pz,'1') NOT IN (0)",
    "div(z,z) IN (NaN, 1)",      # a set that holds NaN holds every NaN
    "div(z,z) NOT IN (NaN)",
]
SHAPES = [
    "ri - di > 0",                                                 # the leaf alone
    "NOT (ri - di > 0)",                                           # under NOT
    "c_inv = 3 AND ri - di > 0",                                   # AND with an inverted-index leaf
    "srt BETWEEN 3 AND 11 AND ri - di > 0",                        # ... a sorted leaf
    "rs < 300 AND ri - di > 0",                                    # ... a raw scan
    "s < 300 AND ri - di > 0",                                     # ... a dictionary scan
    "rs < 100 OR ri - di > 40",                                    # OR with a scan
    "ri - di > 0 AND rd / 3 > 100.25",                             # two expression leaves
    "ri - di > 0 OR NOT (rd / 3 > 100.25)",
    "c_inv IN (1, 5) AND (rs < 500 OR ri > di) AND NOT (ri * rd > 1000)",
]
EVERY_WHERE = OPERANDS + PREDICATES + NON_FINITE + MODEL_ONLY + SHAPES


def _signed(rng, lo, hi, n):
    return rng.integers(lo, hi, n) * rng.choice(np.array([-1, 1]), n)


def _leaves(f, out):
    if f.type == "PREDICATE":
        out.append(f.predicate)
    for c in f.children:
        _leaves(c, out)
    return out


def _where(where, flags=0):
    if isinstance(where, str):
        if "NaN" in where:   # (the SQL front end has no NaN literal: the predicate is written directly)
            m = re.match(r"^(\S+) (NOT IN|IN) \((.*)\)$", where)
            p = Predicate("NOT_IN" if m.group(2) == "NOT IN" else "IN", m.group(1), [v.strip() for v in m.group(3).split(",")])
            qc = parse_sql("SELECT COUNT(*) FROM t")
            qc.filter = FilterContext.pred(p)
        else:
            qc = parse_sql("SELECT COUNT(*) FROM t WHERE " + where)
    else:
        qc = where
    qc.flags |= flags
    return qc


def _data(n, seed=23):
    rng = np.random.default_rng(seed + n)
    rl = _signed(rng, 1, 400, n).astype(np.int64) * 0x1_0000_0003
    rl[rng.integers(0, n, 7)] = 2**53 + 1            # LONGs that are no doubles
    rl[rng.integers(0, n, 7)] = 2**53 + 3
    z = rng.integers(-2, 3, n).astype(np.int32)      # zeros among them: di / z is +-Inf there, z / z NaN
    data = {
        "g7": rng.integers(0, 7, n).astype(np.int32), "g3": rng.integers(0, 3, n).astype(np.int32),
        "k": rng.integers(0, 5000, n).astype(np.int32), "k3": rng.integers(0, 60, n).astype(np.int32),
        "rg": (rng.integers(0, 50, n) * 1000 - 7).astype(np.int32),
        "s": rng.integers(0, 1000, n).astype(np.int32), "rs": rng.integers(0, 1000, n).astype(np.int32),
        "c_inv": rng.integers(0, 8, n).astype(np.int32), "srt": np.sort(rng.integers(0, 20, n)).astype(np.int32),
        "di": _signed(rng, 1, 50, n).astype(np.int32), "dl": _signed(rng, 1, 300, n).astype(np.int64) * 10**10,
        "df": rng.choice(np.array([0.5, 1.5, -2.25, 3e3, 0.1], dtype=np.float32), n),
        "dd": rng.choice(np.array([0.1, -7.0, 1e-3, 123.456, 1e3]), n),
        "ri": _signed(rng, 1, 50, n).astype(np.int32), "rl": rl,
        "rf": (rng.uniform(0.5, 1000.0, n) * rng.choice(np.array([-1.0, 1.0]), n)).astype(np.float32),
        "rd": rng.uniform(1e-3, 1e3, n) * rng.choice(np.array([-1.0, 1.0]), n),
        "z": z, "pz": rng.choice(np.array([0.0, -0.0, 1.5, -3.0]), n),
        "txt": np.array(["t%d" % v for v in rng.integers(0, 5, n)], dtype=object).tolist(),
    }
    schema = {k: "INT" for k in data}
    schema.update(dl="LONG", rl="LONG", df="FLOAT", rf="FLOAT", dd="DOUBLE", rd="DOUBLE", pz="DOUBLE", txt="STRING")
    twins = {}
    for where in EVERY_WHERE:
        for p in _leaves(_where(where).filter, []):
            if "(" in p.column and p.column not in twins:
                name = "tw%d" % len(twins)
                twins[p.column] = name
                data[name] = em.evaluate(p.column, data, schema)
                schema[name] = "DOUBLE"
    host = build_segment("xf_%d" % n, data, schema, inverted_index_columns=["c_inv"],
                         no_dictionary_columns=["rg", "rs", "ri", "rl", "rf", "rd", "z", "pz"] + list(twins.values()))
    mv_rng = np.random.default_rng(n)
    mv_rows = [list(mv_rng.integers(0, 20, mv_rng.integers(1, 4))) for _ in range(n)]
    host.columns["mv"] = build_mv_column("mv", mv_rows, "INT")
    data["mv"] = mv_rows
    return host, data, schema, twins


_SEGMENTS = {}


@pytest.fixture(scope="module")
def segments(gpu_api, oracle_api):
    def get(n):
        if n not in _SEGMENTS:
            host, data, schema, twins = _data(n)
            _SEGMENTS[n] = (host, data, schema, twins, NativeSegment(gpu_api, host), NativeSegment(oracle_api, host))
        return _SEGMENTS[n]
    yield get
    for seg in _SEGMENTS.values():
        seg[4].destroy()
        seg[5].destroy()
    _SEGMENTS.clear()


def _twin(qc, twins):
    """the same query with every expression predicate moved onto its twin column"""
    t = copy.copy(qc)
    for cached in ("_cquery", "_cquery_native"):   # (the C structs an execution left on the QueryContext: not the twin's)
        t.__dict__.pop(cached, None)
    t.filter = copy.deepcopy(qc.filter)
    for p in _leaves(t.filter, []):
        if "(" in p.column:
            p.column = twins[p.column]
    return t


def _model_mask(f, data, schema):
    """the filter's doc set from the model's evaluators (plain columns compare as numbers too: INT columns and literals only)"""
    if f.type == "PREDICATE":
        p = f.predicate
        v = em.evaluate(p.column, data, schema) if "(" in p.column else np.asarray(data[p.column], dtype=np.float64)
        return fm.apply_predicate(v, p)
    ms = [_model_mask(c, data, schema) for c in f.children]
    if f.type == "NOT":
        return ~ms[0]
    out = ms[0]
    for m in ms[1:]:
        out = (out & m) if f.type == "AND" else (out | m)
    return out


def _check_filter(seg, where, twin=True):
    host, data, schema, twins, gpu, oracle = seg
    qc = _where(where)
    want = np.flatnonzero(_model_mask(qc.filter, data, schema))
    ds = gpu.filter(qc)
    got, words, card = ds.doc_ids(), ds.words(), ds.cardinality()
    ds.free()
    assert np.array_equal(got, want), (where, len(got), len(want))
    assert card == len(want)
    n = host.total_docs   # the words themselves: bit doc & 63 of word doc >> 6, nothing at or beyond numDocs
    bits = np.unpackbits(np.asarray(words, dtype="<u8").view(np.uint8), bitorder="little")
    assert np.array_equal(np.flatnonzero(bits), want) and not bits[n:].any(), where
    if twin:
        ods = oracle.filter(_twin(qc, twins))
        assert np.array_equal(ods.doc_ids(), want), where   # the two sources agree
        ods.free()
    b = gpu.execute(qc)
    assert b.aggregation_result() == [len(want)] and b.stats.num_docs_scanned == len(want), where
    assert b.stats.star_tree_index == -1
    return want


# ---- doc sets ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_operands(segments, n):
    for where in OPERANDS:
        _check_filter(segments(n), where)


@pytest.mark.parametrize("n", SIZES)
def test_predicates(segments, n):
    for where in PREDICATES:
        _check_filter(segments(n), where)


@pytest.mark.parametrize("n", [65, 2049, BIG])
def test_division_by_zero_matches_as_java_says(segments, n):
    _division_by_zero(segments(n), n)


def _division_by_zero(seg, n):
    data, schema = seg[1], seg[2]
    z = np.asarray(data["z"])
    if n > 1000:
        v = em.evaluate("div(di,z)", data, schema)
        assert np.isposinf(v).any() and np.isneginf(v).any()
    for where in NON_FINITE:
        _check_filter(seg, where)
    assert np.array_equal(_check_filter(seg, "div(z,z) != 1"), np.flatnonzero(z == 0))     # NaN != 1; z / z = 1 elsewhere
    assert np.array_equal(_check_filter(seg, "div(z,z) = 1"), np.flatnonzero(z != 0))      # NaN equals nothing
    assert np.array_equal(_check_filter(seg, "div(z,z) >= 0"), np.flatnonzero(z != 0))     # ... and lies in no range
    assert len(_check_filter(seg, "div(di,z) != 0.3")) == n                                  # nothing is refused, the infinities match


@pytest.mark.parametrize("n", [65, 2049])
def test_zero_signs_and_nan_under_eq_and_in(segments, n):
    seg = segments(n)
    pz = np.asarray(seg[1]["pz"])
    plus = np.flatnonzero((pz == 0) & ~np.signbit(pz))
    minus = np.flatnonzero((pz == 0) & np.signbit(pz))
    assert len(plus) and len(minus)
    both = np.sort(np.concatenate([plus, minus]))
    assert np.array_equal(_check_filter(seg, "mult(pz,'1') = 0"), both)                       # EQ: numeric
    assert np.array_equal(_check_filter(seg, "mult(pz,'1') IN (0)", twin=False), plus)        # IN: bit patterns
    assert np.array_equal(_check_filter(seg, "mult(pz,'1') IN ('-0.0')", twin=False), minus)
    assert len(_check_filter(seg, "mult(pz,'1') NOT IN (0)", twin=False)) == n - len(plus)
    z = np.asarray(seg[1]["z"])
    assert np.array_equal(_check_filter(seg, "div(z,z) IN (NaN, 1)", twin=False), np.arange(n))
    assert np.array_equal(_check_filter(seg, "div(z,z) NOT IN (NaN)", twin=False), np.flatnonzero(z != 0))


def test_range_bounds(segments):
    seg = segments(2047)
    gpu = seg[4]
    v = em.evaluate("minus(ri,di)", seg[1], seg[2])
    for lower, upper, li, ui in (("3", "7", True, True), ("3", "7", False, False), ("3", "7", True, False), ("3", "7", False, True),
                                 ("-Infinity", "0", True, True), ("0", "Infinity", False, True), ("Infinity", "*", True, False)):
        p = Predicate("RANGE", "minus(ri,di)", [], lower, upper, li, ui)
        qc = parse_sql("SELECT COUNT(*) FROM t")
        qc.filter = FilterContext.pred(p)
        ds = gpu.filter(qc)
        assert np.array_equal(ds.doc_ids(), np.flatnonzero(fm.apply_predicate(v, p))), (lower, upper, li, ui)
        ds.free()
    for lower, upper in (("Infinity", "*"), ("*", "-Infinity")):   # an exclusive bound at its infinity: "Invalid range", not an empty match
        qc = parse_sql("SELECT COUNT(*) FROM t")
        qc.filter = FilterContext.pred(Predicate("RANGE", "minus(ri,di)", [], lower, upper, False, False))
        _refused(seg[4].api, gpu, qc, capi.PG_ERR_INVALID_ARGUMENT, "Invalid range")


def test_contraction(gpu_api):
    """a = b = 2^27 + 1, c = -2^54: a * b rounds to 2^54 + 2^28, so a * b + c is 2^28 = 268435456 per doc; a fused multiply-add gives 2^28 + 1"""
    n = 65
    data = {"a": np.full(n, 2**27 + 1, dtype=np.int64), "b": np.full(n, 2**27 + 1, dtype=np.int64), "c": np.full(n, -2**54, dtype=np.int64)}
    schema = {"a": "LONG", "b": "LONG", "c": "LONG"}
    assert em.evaluate("plus(times(a,b),c)", data, schema).tolist() == [float(2**28)] * n
    seg = NativeSegment(gpu_api, build_segment("fma", data, schema, no_dictionary_columns=["b", "c"]))
    try:
        assert seg.execute("SELECT COUNT(*) FROM t WHERE a * b + c = 268435456").aggregation_result() == [n]
        assert seg.execute("SELECT COUNT(*) FROM t WHERE a * b + c = 268435457").aggregation_result() == [0]
        assert seg.execute("SELECT COUNT(*) FROM t WHERE add(mult(a,b),c) != 268435456").aggregation_result() == [0]
    finally:
        seg.destroy()


# ---- tree shapes, consumers: against the twin ---------------------------------------------------------------------------------------------------------
def _check_twin(seg, sql, flags=0):
    """`sql` on the GPU against its twin through the oracle: groups, intermediate results, numDocsScanned, numEntriesScannedPostFilter"""
    host, data, schema, twins, gpu, oracle = seg
    qc = parse_sql(sql)
    qc.flags |= flags
    if qc.selection or qc.distinct:
        # the oracle has neither operator: the rows come from the twin's doc set through the oracle and the host's columns (no ties at a cut:
        # the ORDER BY columns are all the columns selected)
        ods = oracle.filter(_twin(qc, twins))
        docs = ods.doc_ids()
        ods.free()
        cols = qc.selection or qc.distinct
        rows = [tuple(np.asarray(data[c])[d].item() for c in cols) for d in docs]
        gb = gpu.execute(qc)
        if qc.distinct:
            rows = sorted(set(rows))
            if qc.order_by:
                assert [c for c, _ in qc.order_by] == cols and len(cols) == 1
                rows = sorted(rows, reverse=not qc.order_by[0][1])[:qc.limit]
                assert gb.distinct_rows == rows, sql
            else:
                assert len(rows) <= qc.limit and sorted(gb.distinct_rows) == rows, sql
        elif qc.order_by:
            for c, asc in reversed(qc.order_by):
                rows.sort(key=lambda r: r[cols.index(c)], reverse=not asc)
            assert gb.selection_rows == rows[:qc.limit], sql
        else:
            assert gb.selection_rows == rows[:qc.limit], sql
        assert gb.stats.star_tree_index == -1
        return gb
    if any(a.function == "PERCENTILE" for a in qc.aggregations):
        # the oracle has no PERCENTILE either: the value lists come from tests/percentile_model.py over the twin's doc set through the oracle
        ods = oracle.filter(_twin(qc, twins))
        docs = ods.doc_ids()
        ods.free()
        gb = gpu.execute(qc)
        rows = gb.rows()
        groups = pm.group_docs([data[g] for g in qc.group_by], docs) if qc.group_by else {(): np.asarray(docs, dtype=np.int64)}
        assert set(rows) == set(groups), sql
        for key, gdocs in groups.items():
            for i, a in enumerate(qc.aggregations):
                assert a.function == "PERCENTILE", sql
                assert pm.same_runs(rows[key][i], pm.runs(pm.as_doubles(np.asarray(data[a.column])[gdocs], schema[a.column]))), (sql, key, a)
        read = set(qc.group_by) | {a.column for a in qc.aggregations}
        assert (gb.stats.num_docs_scanned, gb.stats.num_entries_scanned_post_filter) == pm.statistics(len(docs), read), sql
        assert gb.stats.star_tree_index == -1
        return gb
    gb, ob = gpu.execute(qc), oracle.execute(_twin(qc, twins))
    gr, orr = gb.rows(), ob.rows()
    assert set(gr) == set(orr), sql
    for key in orr:
        assert gr[key] == orr[key], (sql, key, gr[key], orr[key])
    assert gb.stats.num_docs_scanned == ob.stats.num_docs_scanned, sql
    assert gb.stats.num_entries_scanned_post_filter == ob.stats.num_entries_scanned_post_filter, sql   # the filter's operands do not count there
    assert gb.stats.star_tree_index == -1
    return gb


@pytest.mark.parametrize("n", SIZES)
def test_tree_shapes(segments, n):
    seg = segments(n)
    for where in SHAPES:
        _check_filter(seg, where)
        _check_twin(seg, "SELECT g7, COUNT(*), SUM(s), MAX(rd) FROM t WHERE " + where + " GROUP BY g7")


def test_column_to_column_comparison_through_parse_sql(segments):
    seg = segments(2049)
    data = seg[1]
    qc = parse_sql("SELECT COUNT(*) FROM t WHERE ri > di")
    assert qc.filter.predicate.column == "minus(ri,di)" and (qc.filter.predicate.lower, qc.filter.predicate.lower_inclusive) == ("0", False)
    assert seg[4].execute(qc).aggregation_result() == [int((np.asarray(data["ri"]) > np.asarray(data["di"])).sum())]


# (SUMs over INT / LONG columns only: a floating SUM is kept exact here while the oracle adds in doc order — tests/test_gpu_sum_exactness.py)
CONSUMERS = [
    "SELECT COUNT(*), SUM(s), MIN(rd), MAX(dl), AVG(rs) FROM t WHERE ri - di > 0",                                        # no GROUP BY
    "SELECT g7, g3, COUNT(*), SUM(dl), MAX(rd), MINMAXRANGE(ri) FROM t WHERE ri - di > 0 AND c_inv IN (1, 5) GROUP BY g7, g3",   # the LDS tier
    "SELECT k, k3, COUNT(*), SUM(s) FROM t WHERE ri - di > 0 GROUP BY k, k3 LIMIT 1000000",                               # a key space beyond LDS
    "SELECT rg, COUNT(*), SUM(s) FROM t WHERE ri - di > 0 GROUP BY rg LIMIT 100000",                                      # hashed raw keys
    "SELECT g3, COUNTMV(mv), SUMMV(mv), MAXMV(mv) FROM t WHERE rd / 3 > 100.25 GROUP BY g3",                              # an *MV aggregation
    "SELECT SUMMV(mv) FROM t WHERE ri - di > 0 AND s < 500",
    "SELECT g7, DISTINCTCOUNT(s), DISTINCTCOUNTHLL(k) FROM t WHERE ri > di GROUP BY g7",
    "SELECT DISTINCT g7, g3 FROM t WHERE ri - di > 0 LIMIT 100",                                                          # DISTINCT
    "SELECT DISTINCT k3 FROM t WHERE ri - di > 0 AND rs < 300 ORDER BY k3 DESC LIMIT 7",
    "SELECT s, rd, k FROM t WHERE ri - di > 0 LIMIT 10",                                                                    # a selection with LIMIT
    "SELECT s, k FROM t WHERE rd / 3 > 100.25 ORDER BY s, k DESC LIMIT 25",
    "SELECT g3, PERCENTILE(s, 50), PERCENTILE(rs, 99) FROM t WHERE ri - di > 0 GROUP BY g3",                              # a PERCENTILE
]


@pytest.mark.parametrize("n", [2049, BIG])
def test_consumers(segments, n):
    seg = segments(n)
    kernels = [_check_twin(seg, sql).stats.kernel.decode() for sql in CONSUMERS]
    if n == BIG:
        assert len({kernels[1], kernels[2], kernels[3]}) == 3, kernels   # three aggregation tiers ran: LDS table, partitions, hashed keys


def test_expression_aggregation_next_to_an_expression_filter(segments):
    seg = segments(BIG)
    host, data, schema, twins, gpu, oracle = seg
    docs = np.flatnonzero(_model_mask(_where("ri > di").filter, data, schema))
    b = gpu.execute("SELECT g3, COUNT(*), SUM(ri * rd), MAX(rd - dd) FROM t WHERE ri > di GROUP BY g3")
    rows = b.rows()
    groups = pm.group_docs([data["g3"]], docs)
    assert set(rows) == set(groups) and b.stats.num_docs_scanned == len(docs)
    for key, gdocs in groups.items():
        assert rows[key][0] == len(gdocs)
        assert pm.same_double(rows[key][1], em.agg_sum(em.evaluate("times(ri,rd)", data, schema, gdocs)))
        assert pm.same_double(rows[key][2], em.agg_max(em.evaluate("minus(rd,dd)", data, schema, gdocs)))


def test_upsert_snapshot(gpu_api, oracle_api):
    host, data, schema, twins = _data(2049, seed=5)
    g, o = NativeSegment(gpu_api, host), NativeSegment(oracle_api, host)
    keep = snapshot_doc_ids(host.total_docs)
    g.set_queryable_doc_ids(keep)
    o.set_queryable_doc_ids(keep)
    try:
        seg = (host, data, schema, twins, g, o)
        for sql in ("SELECT g7, COUNT(*), SUM(s) FROM t WHERE ri - di > 0 GROUP BY g7", "SELECT COUNT(*) FROM t WHERE NOT (ri - di > 0)",
                    "SELECT COUNT(*), MAX(rd) FROM t WHERE rs < 300 AND ri - di > 0", "SELECT s FROM t WHERE ri - di > 0 LIMIT 5"):
            _check_twin(seg, sql)
        ds = g.filter("SELECT COUNT(*) FROM t WHERE ri - di > 0")
        want = np.intersect1d(np.flatnonzero(_model_mask(_where("ri - di > 0").filter, data, schema)), keep)
        assert np.array_equal(ds.doc_ids(), want)
        ds.free()
    finally:
        g.destroy()
        o.destroy()


def test_null_handling_with_null_free_operands(gpu_api, oracle_api):
    host, data, schema, twins = _data(2049, seed=6)
    nulls = np.frombuffer(formats.serialize_roaring(np.array([3, 77, 2000], dtype=np.int64)), dtype=np.uint8)
    host.columns["s"].null_vector = nulls          # a column the expressions do not read
    g, o = NativeSegment(gpu_api, host), NativeSegment(oracle_api, host)
    try:
        seg = (host, data, schema, twins, g, o)
        NH = capi.QUERY_FLAG_NULL_HANDLING
        for sql in ("SELECT g7, COUNT(*), MAX(rd) FROM t WHERE ri - di > 0 GROUP BY g7", "SELECT COUNT(*) FROM t WHERE NOT (ri - di > 0)",
                    "SELECT COUNT(*) FROM t WHERE s < 500 AND ri - di > 0", "SELECT COUNT(*) FROM t WHERE NOT (s < 500 OR ri - di > 0)",
                    "SELECT g3, SUM(rs) FROM t WHERE ri - di > 0 AND s >= 100 GROUP BY g3"):
            _check_twin(seg, sql, flags=NH)
        qc = parse_sql("SELECT COUNT(*) FROM t WHERE add(s,ri) > 0")   # ... and one they do read: refused
        qc.flags |= NH
        _refused(gpu_api, g, qc, capi.PG_ERR_UNSUPPORTED, "expression over s, which holds nulls")
        assert g.execute("SELECT COUNT(*) FROM t WHERE add(s,ri) > 0").aggregation_result() == [int((np.asarray(data["s"]) + np.asarray(data["ri"]) > 0).sum())]
    finally:
        g.destroy()
        o.destroy()


# ---- statistics -------------------------------------------------------------------------------------------------------------------------------------
def _col_mask(data, where):
    p = _where(where).filter.predicate
    return fm.apply_predicate(np.asarray(data[p.column], dtype=np.float64), p)


def _check_stats(seg, where, tree):
    host, data, schema, twins, gpu, oracle = seg
    n = host.total_docs
    entries, docs = fm.entries_scanned_in_filter(tree, n)
    qc = parse_sql("SELECT COUNT(*), MAX(s) FROM t WHERE " + where)
    b = gpu.execute(qc)
    got = (b.stats.num_docs_scanned, b.stats.num_entries_scanned_in_filter, b.stats.stats_exact)
    print(where, n, "numDocsScanned / numEntriesScannedInFilter / exact:", got, "model:", (len(docs), entries))
    assert got == (len(docs), entries, 1), (where, n)
    ds = gpu.filter(qc)
    st = ds.stats()
    assert np.array_equal(ds.doc_ids(), np.asarray(docs, dtype=ds.doc_ids().dtype))
    assert (st.num_entries_scanned_in_filter, st.stats_exact) == (entries, 1), where
    ds.free()
    return entries


@pytest.mark.parametrize("n", SIZES)
def test_statistics(segments, n):
    seg = segments(n)
    data, schema = seg[1], seg[2]
    leaf = fm.apply_predicate(em.evaluate("minus(ri,di)", data, schema), _where("ri - di > 0").filter.predicate)
    rare = fm.apply_predicate(em.evaluate("minus(ri,di)", data, schema), _where("ri - di > 40").filter.predicate)
    assert _check_stats(seg, "ri - di > 0", ("expr", leaf)) == n                                    # the lone leaf: every doc once
    assert _check_stats(seg, "NOT (ri - di > 0)", ("not", ("expr", leaf))) == n
    inv = _col_mask(data, "c_inv = 3")
    assert _check_stats(seg, "c_inv = 3 AND ri - di > 0", ("and", [("index", inv), ("expr", leaf)])) == int(inv.sum())   # applyAnd: the candidates
    _check_stats(seg, "rs < 300 AND ri - di > 0", ("and", [("scan", _col_mask(data, "rs < 300")), ("expr", leaf)]))     # the leapfrog
    _check_stats(seg, "rs < 3 AND ri - di > 40", ("and", [("scan", _col_mask(data, "rs < 3")), ("expr", rare)]))
    _check_stats(seg, "rs < 100 OR ri - di > 40", ("or", [("scan", _col_mask(data, "rs < 100")), ("expr", rare)]))
    # NOT over the leaf is ExpressionFilterOperator#getFalses — an expression iterator over the rejected docs: applyAnd behind an index
    assert _check_stats(seg, "c_inv = 3 AND NOT (ri - di > 0)", ("and", [("index", inv), ("not", ("expr", leaf))])) == int(inv.sum())
    _check_stats(seg, "rs < 300 AND NOT (ri - di > 0)", ("and", [("scan", _col_mask(data, "rs < 300")), ("not", ("expr", leaf))]))
    _check_stats(seg, "rs < 100 OR NOT (ri - di > 0)", ("or", [("scan", _col_mask(data, "rs < 100")), ("not", ("expr", leaf))]))
    _check_stats(seg, "c_inv = 3 AND rs < 300 AND ri - di > 0",
                 ("and", [("index", inv), ("scan", _col_mask(data, "rs < 300")), ("expr", leaf)]))


def test_statistics_leaf_match_in_a_later_block(gpu_api):
    """AND(raw scan {5, 25000}, leaf {25000}) over 30 011 docs: the leaf's only match lies two blocks behind the scan's first candidate —
    35 017 entries, worked out by hand in tests/test_expression_filter_model.py"""
    n = BIG
    sc, la, lb = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32), np.ones(n, dtype=np.int32)
    sc[[5, 25000]] = 1
    la[25000] = 7
    iv, ma, lz = (np.arange(n) % 10).astype(np.int32), (np.arange(n) >= 25000).astype(np.int32), np.zeros(n, dtype=np.int32)
    data = {"sc": sc, "la": la, "lb": lb, "s": np.arange(n, dtype=np.int32) % 17, "iv": iv, "ma": ma, "lz": lz}
    schema = {k: "INT" for k in data}
    host = build_segment("later_block", data, schema, no_dictionary_columns=["sc", "la", "ma"], inverted_index_columns=["iv"])
    gpu = NativeSegment(gpu_api, host)
    try:
        seg = (host, data, schema, {}, gpu, None)
        assert _check_stats(seg, "sc = 1 AND la > lb", ("and", [("scan", sc == 1), ("expr", la > lb)])) == 6 + 30000 + 1 + 5010
        # the same leaf under a selection's LIMIT: the walk stops after the first doc (one scan advance, three blocks, one scan advance)
        b = gpu.execute("SELECT s FROM t WHERE sc = 1 AND la > lb LIMIT 1")
        entries, docs = fm.entries_scanned_in_filter(("and", [("scan", sc == 1), ("expr", la > lb)]), n, max_next=1)
        assert b.selection_rows == [(25000 % 17,)] and docs == [25000]
        assert (b.stats.num_entries_scanned_in_filter, b.stats.stats_exact) == (entries, 1) and entries == 6 + 30000 + 1
        # NOT over the leaf (ExpressionFilterOperator#getFalses: an expression iterator over the rejected docs), the numbers worked out by
        # hand in tests/test_expression_filter_model.py.  lb >= la holds everywhere but at doc 25000; la + lb is 1 everywhere but there.
        rejected = ~(lb >= la)
        assert np.flatnonzero(rejected).tolist() == [25000]
        assert _check_stats(seg, "iv = 0 AND NOT (lb >= la)", ("and", [("index", iv == 0), ("not", ("expr", lb >= la))])) == 3002
        assert _check_stats(seg, "sc = 1 AND NOT (lb >= la)", ("and", [("scan", sc == 1), ("not", ("expr", lb >= la))])) == 6 + 30000 + 1 + 5010
        assert _check_stats(seg, "sc = 1 AND la + lb NOT BETWEEN 0 AND 2",
                            ("and", [("scan", sc == 1), ("not", ("expr", (la + lb >= 0) & (la + lb <= 2)))])) == 6 + 30000 + 1 + 5010
        # ... and a LIMIT selection over NOT(leaf): ma > lz holds from doc 25000 on, the first block holds a rejected doc
        assert _check_stats(seg, "NOT (ma > lz)", ("not", ("expr", ma > lz))) == n
        b = gpu.execute("SELECT s FROM t WHERE NOT (ma > lz) LIMIT 1")
        assert b.selection_rows == [(0,)]
        assert (b.stats.num_entries_scanned_in_filter, b.stats.stats_exact) == (10000, 1)
    finally:
        gpu.destroy()


def test_reference_goldens(gpu_api):
    """NullHandlingEnabledQueriesTest's expression filter cases, per segment, as tests/test_expression_filter_model.py pins the model to them"""
    import json
    expected = json.load(open(os.path.join(ROOT, "tests", "golden", "expression_filter_expected.json")))
    for name in ("addition", "addition_inside_not"):
        case = expected[name]
        rows = np.array([case["null_replacement"] if v is None else v for v in case["rows"]], dtype=np.int32)
        seg = NativeSegment(gpu_api, build_segment(name, {"column1": rows}, {"column1": "INT"}))
        try:
            b = seg.execute(case["sql"])
            assert sorted(r[0] for r in b.selection_rows) == [-2147483648, -1] and len(b.selection_rows) == case["rows_per_segment"]
            assert (b.stats.num_entries_scanned_in_filter, b.stats.stats_exact) == (case["num_entries_scanned_in_filter"], 1)
        finally:
            seg.destroy()
    case = expected["second_block"]
    n = case["null_rows"]
    c1, c2 = np.full(n + 1, case["null_replacement"], dtype=np.int32), np.arange(n + 1, dtype=np.int32)
    c1[n], c2[n] = case["last_row"]
    seg = NativeSegment(gpu_api, build_segment("second_block", {"column1": c1, "column2": c2}, {"column1": "INT", "column2": "INT"}))
    try:
        b = seg.execute(case["sql"])
        assert b.selection_rows == [tuple(case["row"])]
        assert (b.stats.num_entries_scanned_in_filter, b.stats.stats_exact) == (case["num_entries_scanned_in_filter"], 1)
    finally:
        seg.destroy()


# ---- plan state ---------------------------------------------------------------------------------------------------------------------------------------
def test_star_tree_route_is_not_taken(gpu_api):
    from pinot_amd.segment import decode_column
    from tests.fixtures import synth_star_segment
    host = synth_star_segment(num_docs=20_000)
    seg = NativeSegment(gpu_api, host)
    try:
        m = decode_column(host.columns["m"], host.total_docs).astype(np.float64)
        h1 = decode_column(host.columns["h1"], host.total_docs)
        plain = seg.execute("SELECT h1, COUNT(*), SUM(m) FROM gpuBench GROUP BY h1")
        assert plain.stats.star_tree_index >= 0                      # the star-tree answers the query without the expression leaf ...
        threshold = float(np.median(m))
        b = seg.execute("SELECT h1, COUNT(*), SUM(m) FROM gpuBench WHERE m - 1 > %r GROUP BY h1" % threshold)
        assert b.stats.star_tree_index == -1                         # ... never the one with it
        keep = (m - 1.0) > threshold
        assert b.stats.num_docs_scanned == int(keep.sum()) > 0
        for key, (count, total) in b.rows().items():
            sel = keep & (h1 == key[0])
            assert count == int(sel.sum()) and total == float(m[sel].sum())
    finally:
        seg.destroy()


def test_plan_cache_keeps_the_words_per_literal(segments):
    seg = segments(2049)
    data, schema, gpu = seg[1], seg[2], seg[4]
    v = em.evaluate("minus(ri,di)", data, schema)
    for literal in (10, 20, 10, 20):   # the second round comes from the cached plans: each its own words
        for where, mask in (("ri - di > %d" % literal, v > literal), ("ri - di IN (%d, 1)" % literal, (v == literal) | (v == 1))):
            ds = gpu.filter("SELECT COUNT(*) FROM t WHERE " + where)
            assert np.array_equal(ds.doc_ids(), np.flatnonzero(mask)), where
            ds.free()
            assert gpu.execute("SELECT COUNT(*) FROM t WHERE " + where).aggregation_result() == [int(mask.sum())]


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------------
def _refused(gpu_api, seg, qc, status, text):
    for call in ("query_supported", "query_exec"):
        cq = CQuery(qc, tuple(seg.host.columns))
        h = capi.C.c_void_p()
        with pytest.raises(capi.NativeError) as e:
            if call == "query_supported":
                gpu_api.call(call, seg.handle, cq.ptr())
            else:
                gpu_api.call(call, seg.handle, cq.ptr(), capi.C.byref(h))
        assert e.value.status == status and text in e.value.message, (call, e.value.status, e.value.message)


def _with_filter(sql, f):
    qc = parse_sql(sql)
    qc.filter = f
    return qc


def test_refusals(gpu_api):
    host, data, schema, twins = _data(2047, seed=3)
    host.columns["by"] = build_column("by", [b"ab%d" % (i % 5) for i in range(host.total_docs)], "BYTES", dictionary=False)
    nulls = np.frombuffer(formats.serialize_roaring(np.array([3, 77, 2000], dtype=np.int64)), dtype=np.uint8)
    host.columns["di"].null_vector = nulls
    seg = NativeSegment(gpu_api, host)
    U, I, NF = capi.PG_ERR_UNSUPPORTED, capi.PG_ERR_INVALID_ARGUMENT, capi.PG_ERR_NOT_FOUND
    count = "SELECT COUNT(*) FROM t"
    group = "SELECT g7, COUNT(*), SUM(s) FROM t GROUP BY g7"
    select = "SELECT s FROM t LIMIT 5"
    distinct = "SELECT DISTINCT g7 FROM t"
    try:
        for sql in (count, group, select, distinct):
            for pred in ("IS_NULL", "IS_NOT_NULL"):
                _refused(gpu_api, seg, _with_filter(sql, FilterContext.pred(Predicate(pred, "add(ri,rd)"))), U, "IS [NOT] NULL over the expression add(ri,rd)")
            _refused(gpu_api, seg, _with_filter(sql, parse_sql(count + " WHERE add(mv,ri) > 0").filter), U, "expression over the multi-value column mv")
            _refused(gpu_api, seg, _with_filter(sql, parse_sql(count + " WHERE add(txt,ri) > 0").filter), U, "expression over the STRING column txt")
            _refused(gpu_api, seg, _with_filter(sql, parse_sql(count + " WHERE add(by,ri) > 0").filter), U, "expression over the BYTES column by")
            _refused(gpu_api, seg, _with_filter(sql, parse_sql(count + " WHERE mod(ri,2) = 0").filter), U, "the function mod")
            _refused(gpu_api, seg, _with_filter(sql, parse_sql(count + " WHERE abs(ri) > 3 AND s < 10").filter), U, "the function abs")
            _refused(gpu_api, seg, _with_filter(sql, parse_sql(count + " WHERE add(nope,ri) > 0").filter), NF, "column not found: nope")
            _refused(gpu_api, seg, _with_filter(sql, FilterContext.pred(Predicate("EQ", "add(ri,rd", ["1"]))), I, "expression:")
            _refused(gpu_api, seg, _with_filter(sql, FilterContext.pred(Predicate("EQ", "add(ri)", ["1"]))), I, "takes 2 or more arguments")
            _refused(gpu_api, seg, _with_filter(sql, FilterContext.pred(Predicate("EQ", "add(ri,rd)", ["x1"]))), I, "NumberFormatException")
        five = " AND ".join("ri + %d > di" % i for i in range(5))
        _refused(gpu_api, seg, parse_sql(count + " WHERE " + five), U, "more than 4 predicates over expressions in one filter")
        four = " AND ".join("ri + %d > di" % i for i in range(4))
        ri, di = np.asarray(data["ri"]), np.asarray(data["di"])
        assert seg.execute(count + " WHERE " + four).aggregation_result() == [int((ri > di).sum())]
        sixteen = "ri" + "".join(" + %d * rd" % i for i in range(2, 10))       # 8 products + 8 sums
        _refused(gpu_api, seg, parse_sql(count + " WHERE " + sixteen + " > 0"), U, "more than 15 operations")
        nine = "add(ri,di,rd,dd,rf,df,rl,dl,s) > 0"
        _refused(gpu_api, seg, parse_sql(count + " WHERE " + nine), U, "more than 8 distinct columns")
        # enableNullHandling: an operand column that holds nulls is refused; without the flag, and over null-free operands, the query runs
        qc = parse_sql(group + "")
        qc.filter = parse_sql(count + " WHERE NOT (di + ri > 0)").filter
        qc.flags |= capi.QUERY_FLAG_NULL_HANDLING
        _refused(gpu_api, seg, qc, U, "enableNullHandling: expression over di, which holds nulls")
        qc = parse_sql(count + " WHERE ri - rd > 0")
        qc.flags |= capi.QUERY_FLAG_NULL_HANDLING
        assert seg.execute(qc).aggregation_result() == [int((ri - np.asarray(data["rd"]) > 0).sum())]
    finally:
        seg.destroy()


def test_expression_filter_kernel_uses_no_scratch():
    """pg_expr_pred keeps the operands of its four 64-doc words and the program's intermediates in registers"""
    log = open(os.path.join(ROOT, "pinot_amd", "csrc", "pg_kernels_exprpred.resources.log")).read()
    kernels = re.findall(r"Function Name: (\w+)", log)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", log)]
    assert kernels == ["pg_expr_pred"] and scratch == [0], (kernels, scratch)
