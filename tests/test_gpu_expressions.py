"""Aggregations over arithmetic expressions on the GPU path (SUM / MIN / MAX / AVG / MINMAXRANGE over add / sub / mult / div) against
tests/expression_model.py over the ORACLE's match set: bit for bit (MIN / MAX over a mix of 0.0 and -0.0 excepted: they compare equal and the
reference's answer depends on doc order), numDocsScanned / numEntriesScannedPostFilter from the model, numEntriesScannedInFilter from the
oracle's filter.  The kernel names of the path (pg_expr_reg / pg_expr_lds / pg_expr_hbm) are tied to the model here, not to the oracle, which
has no expressions.

SUM against math.fsum is exact only while every non-zero per-doc value lies within 75 binary orders of the segment's largest magnitude (the
fixed-point scale is q = E - 127 with 2^E just above it, a double has 53 bits): _values() asserts that for every expression a test sums, over
all docs of its segment, so that an edit of the data cannot turn the comparison vacuous."""
import json
import os
import re

import numpy as np
import pytest

from oracle import po_datatable as dt
from pinot_amd import capi, formats
from pinot_amd.executor import Comm, NativeSegment
from pinot_amd.query import AggregationSpec, CQuery, QueryContext, parse_sql
from pinot_amd.segment import build_segment
from tests import expression_model as em
from tests import percentile_model as pm
from tests.fixtures import SV_FILTER, sv_segment
from tests.kernel_inventory import snapshot_doc_ids

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPECTED = json.load(open(os.path.join(ROOT, "tests", "golden", "expression_expected.json")))
SIZES = [2047, 65, 1]   # a partial last match word, two words, one doc


def _signed(rng, lo, hi, n):
    return rng.integers(lo, hi, n) * rng.choice(np.array([-1, 1]), n)


def _data(n, seed=11):
    rng = np.random.default_rng(seed + n)
    rl = _signed(rng, 1, 400, n).astype(np.int64) * 0x1_0000_0003
    rl[rng.integers(0, n, 7)] = 2**53 + 1            # LONGs that are no doubles: (double) rounds them
    rl[rng.integers(0, n, 7)] = 2**53 + 3
    one_big = np.zeros(n, dtype=np.int32)            # one group holding all but one doc
    one_big[n // 2] = 1
    data = {
        "g7": rng.integers(0, 7, n).astype(np.int32), "g20": rng.integers(0, 20, n).astype(np.int32), "g3": rng.integers(0, 3, n).astype(np.int32),
        "gbig": one_big, "rid": (np.arange(n) * 3 - 5).astype(np.int32), "rg": (rng.integers(0, 50, n) * 1000 - 7).astype(np.int32),
        "rs": np.array(["k%d" % v for v in rng.integers(0, 11, n)], dtype=object).tolist(),
        "rdk": rng.choice(np.array([0.5, -2.0, 7.25]), n),
        "s": rng.integers(0, 1000, n).astype(np.int32), "c_inv1": rng.integers(0, 8, n).astype(np.int32),
        # operands: all four types, dictionary-encoded and raw, never zero (they also divide)
        "di": _signed(rng, 1, 1000, n).astype(np.int32), "dl": _signed(rng, 1, 300, n).astype(np.int64) * 10**10,
        "df": rng.choice(np.array([0.5, 1.5, -2.25, 3e3, 0.1], dtype=np.float32), n),
        "dd": rng.choice(np.array([0.1, -7.0, 1e-3, 123.456, 1e3]), n),
        "ri": _signed(rng, 1, 1000, n).astype(np.int32), "rl": rl,
        "rf": (rng.uniform(0.5, 1000.0, n) * rng.choice(np.array([-1.0, 1.0]), n)).astype(np.float32),
        "rd": rng.uniform(1e-3, 1e3, n) * rng.choice(np.array([-1.0, 1.0]), n),
        "txt": np.array(["t%d" % v for v in rng.integers(0, 5, n)], dtype=object).tolist(),
    }
    schema = {k: "INT" for k in data}
    schema.update(dl="LONG", rl="LONG", df="FLOAT", rf="FLOAT", dd="DOUBLE", rd="DOUBLE", rdk="DOUBLE", rs="STRING", txt="STRING")
    host = build_segment("expr_%d" % n, data, schema, inverted_index_columns=["c_inv1"],
                         no_dictionary_columns=["rid", "rg", "rs", "rdk", "ri", "rl", "rf", "rd"])
    return host, data, schema


_SEGMENTS = {}
_VALUES = {}


@pytest.fixture(scope="module")
def segments(gpu_api, oracle_api):
    def get(n):
        if n not in _SEGMENTS:
            host, data, schema = _data(n)
            _SEGMENTS[n] = (host, data, schema, NativeSegment(gpu_api, host), NativeSegment(oracle_api, host))
        return _SEGMENTS[n]
    yield get
    for _, _, _, g, o in _SEGMENTS.values():
        g.destroy()
        o.destroy()
    _SEGMENTS.clear()
    _VALUES.clear()


def _values(seg, text, summed):
    """the expression's per-doc values over ALL docs of the segment, computed once per (segment, text); every one finite, and — for a summed
    expression — every non-zero one within 75 binary orders of the largest magnitude (what makes the comparison with fsum exact)"""
    data, schema = seg[1], seg[2]
    cache = _VALUES.setdefault(id(data), (data, {}))[1]   # (the entry keeps `data` alive: its id is not reused)
    if text not in cache:
        v = em.evaluate(text, data, schema)
        assert np.all(np.isfinite(v)), text
        nz = np.abs(v[v != 0.0])
        spread = int(np.frexp(nz.max())[1] - np.frexp(nz.min())[1]) if nz.size else 0
        cache[text] = (v, spread)
    v, spread = cache[text]
    if summed:
        assert spread <= 75, (text, spread)
    return v


def _filter(oracle, sql):
    """(matching docs, numEntriesScannedInFilter) of the query's filter, from the oracle"""
    where = sql.split(" FROM ", 1)[1].split(" GROUP BY ")[0].split(" ORDER BY ")[0].split(" LIMIT ")[0]
    ds = oracle.filter("SELECT COUNT(*) FROM " + where)
    docs, st = ds.doc_ids(), ds.stats()
    ds.free()
    return docs, st.num_entries_scanned_in_filter


def _same(got, want, min_max):
    if min_max and got == 0.0 and want == 0.0:   # 0.0 and -0.0 compare equal: which one the reference keeps depends on doc order
        return True
    return pm.same_double(got, want)


def _same_result(function, got, want):
    if function in ("SUM", "MIN", "MAX"):
        return _same(got, want, function != "SUM")
    if function == "AVG":
        return _same(got[0], want[0], False) and got[1] == want[1]
    return _same(got[0], want[0], True) and _same(got[1], want[1], True)


def _is_expression(spec):
    return "(" in (spec.column or "")


def _check(seg, sql, kernel=None, num_groups_limit=0, admitted=None):
    """Runs `sql` on the GPU and holds every aggregation over an expression and every COUNT(*) of it, its groups and its statistics to the model."""
    host, data, schema, gpu, oracle = seg
    qc = parse_sql(sql)
    qc.num_groups_limit = num_groups_limit
    docs, in_filter = _filter(oracle, sql)
    groups = pm.group_docs([data[g] for g in qc.group_by], docs) if qc.group_by else {(): np.asarray(docs, dtype=np.int64)}
    if admitted is not None:
        groups = {k: v for k, v in groups.items() if k in admitted}
    b = gpu.execute(qc)
    rows = b.rows()
    assert set(rows) == set(groups), sql
    read = set(qc.group_by)
    for a in qc.aggregations:
        if _is_expression(a):
            read |= set(em.columns_of(a.column))
        elif a.column:
            read.add(a.column)
    assert (b.stats.num_docs_scanned, b.stats.num_entries_scanned_post_filter) == pm.statistics(len(docs), read), sql
    assert b.stats.num_entries_scanned_in_filter == in_filter and b.stats.stats_exact == 1 and b.stats.num_total_docs == host.total_docs, sql
    assert b.stats.star_tree_index == -1
    if kernel is not None:
        assert b.stats.kernel.decode() == kernel, sql
    for key, gdocs in groups.items():
        for a, spec in enumerate(qc.aggregations):
            if spec.function == "COUNT":
                assert rows[key][a] == len(gdocs), (sql, key)
            if not _is_expression(spec):
                continue
            v = _values(seg, spec.column, spec.function in ("SUM", "AVG"))[gdocs]
            want = em.aggregate(spec.function, v)
            assert _same_result(spec.function, rows[key][a], want), (sql, key, spec, rows[key][a], want)
    return b


# ---- the reference's goldens ------------------------------------------------------------------------------------------------------------------
def test_transform_queries_goldens(gpu_api, oracle_api):
    """TransformQueriesTest#testTransformWithAvgInnerSegment: seven AvgPairs over its 10-row segment"""
    data, schema = em.transform_queries_segment()
    host = build_segment("testSegment", data, schema, no_dictionary_columns=["INT_COL2", "LONG_COL2"])
    seg = (host, data, schema, NativeSegment(gpu_api, host), NativeSegment(oracle_api, host))
    try:
        for sql, want_sum, want_count in EXPECTED["transform_avg"]:
            b = _check(seg, sql, kernel="pg_expr_reg")
            assert b.aggregation_result() == [(want_sum, want_count)], sql
    finally:
        seg[3].destroy()
        seg[4].destroy()


@pytest.fixture(scope="module")
def sv(gpu_api, oracle_api, sv_data):
    host = sv_segment(sv_data)
    data = {k: (v.tolist() if v.dtype.kind == "U" else v) for k, v in sv_data.items()}
    schema = {k: ("STRING" if isinstance(v, list) else "INT") for k, v in data.items()}
    g, o = NativeSegment(gpu_api, host), NativeSegment(oracle_api, host)
    yield host, data, schema, g, o
    g.destroy()
    o.destroy()


def test_max_add_golden(sv):
    """ForwardIndexDisabledSingleValueQueriesTest: MAX(ADD(column1, column9)) = 4.264013718E9, numEntriesScannedPostFilter 240 000 over four
    segments — two columns per doc, with and without the filter and GROUP BY column9 (an operand already)"""
    want = EXPECTED["max_add_column1_column9"]
    q = want["query"]
    b = _check(sv, q, kernel="pg_expr_reg")
    assert b.aggregation_result() == [want["value"]]
    assert b.stats.num_entries_scanned_post_filter == want["num_entries_scanned_post_filter_per_segment"] == 2 * sv[0].total_docs
    b = _check(sv, "SELECT column9, MAX(ADD(column1, column9)) FROM testTable GROUP BY column9")
    assert b.stats.num_entries_scanned_post_filter == want["num_entries_scanned_post_filter_per_segment"]
    assert max(r[0] for r in b.rows().values()) == want["value"]
    for tail in (SV_FILTER, SV_FILTER + " GROUP BY column9"):
        b = _check(sv, "SELECT MAX(ADD(column1, column9)) FROM testTable" + tail)
        assert b.stats.num_entries_scanned_post_filter == 2 * b.stats.num_docs_scanned and 0 < b.stats.num_docs_scanned < sv[0].total_docs


# ---- operands -----------------------------------------------------------------------------------------------------------------------------------
OPERANDS = [
    "SELECT SUM(ri * rd), MIN(ri * rd), MAX(ri * rd) FROM t",                                      # raw INT x raw DOUBLE
    "SELECT SUM(add(di,dl)), MINMAXRANGE(add(di,dl)) FROM t WHERE s < 700",                        # dictionary INT + dictionary LONG
    "SELECT g7, SUM(sub(rl,'1')), MAX(rl - 1), MIN(add(rl,'0')) FROM t GROUP BY g7",               # LONGs 2^53 + 1 and 2^53 + 3: cast, then computed
    "SELECT g3, AVG(rf / df), SUM(df * rf) FROM t WHERE c_inv1 IN (1, 5) GROUP BY g3",             # raw FLOAT, dictionary FLOAT
    "SELECT SUM(dd - rd), AVG(dd / rd), MINMAXRANGE(mult(dd,rd)) FROM t WHERE s BETWEEN 100 AND 900",   # dictionary DOUBLE, raw DOUBLE
    "SELECT g7, g3, SUM(1000000 - ri), SUM(1 / rd), SUM(rd / 3), MIN(0.1 - dd) FROM t GROUP BY g7, g3",   # a literal on either side
    "SELECT g20, SUM(add(ri,'2.5',rd,'-1',dd)), SUM(mult(df,'3',ri,'0.5',dd)) FROM t WHERE s >= 50 GROUP BY g20",            # literals between columns
    "SELECT g7, AVG(add(div(di,ri),div(dl,rl))), MAX(add(div(di,ri),div(dl,rl))) FROM t GROUP BY g7",                         # the goldens' nesting
    "SELECT SUM((ri + di) * (rd - dd) / rf), MIN(plus(minus(ri,di),times(rd,divide(dd,rf)))) FROM t WHERE s < 500",
]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("sql", OPERANDS)
def test_operands(segments, n, sql):
    _check(segments(n), sql)


def test_longs_are_cast_before_they_are_computed(segments):
    host, data, schema, gpu, oracle = segments(2047)
    v = _values(segments(2047), "sub(rl,'1')", True)
    assert float(2**53 - 1) in v and float(2**53 + 3) in v    # (double)(2^53 + 1) - 1 and (double)(2^53 + 3) - 1 = 2^53 + 4 - 1, rounded
    assert gpu.execute("SELECT MAX(rl - 1) FROM t").aggregation_result() == [float(2**53 + 3)]


def test_contraction(gpu_api, oracle_api):
    """a = b = 2^27 + 1, c = -2^54: a * b rounds to 2^54 + 2^28, so a * b + c is 2^28 per doc; a fused multiply-add gives 2^28 + 1"""
    n = 65
    data = {"a": np.full(n, 2**27 + 1, dtype=np.int64), "b": np.full(n, 2**27 + 1, dtype=np.int64), "c": np.full(n, -2**54, dtype=np.int64),
            "g": (np.arange(n) % 3).astype(np.int32)}
    schema = {"a": "LONG", "b": "LONG", "c": "LONG", "g": "INT"}
    host = build_segment("fma", data, schema, no_dictionary_columns=["b", "c"])
    seg = (host, data, schema, NativeSegment(gpu_api, host), NativeSegment(oracle_api, host))
    try:
        assert em.evaluate("plus(times(a,b),c)", data, schema).tolist() == [float(2**28)] * n
        b = _check(seg, "SELECT SUM(a * b + c), MAX(a * b + c) FROM t", kernel="pg_expr_reg")
        assert b.aggregation_result() == [float(n * 2**28), float(2**28)]
        _check(seg, "SELECT g, SUM(a * b + c), MIN(add(mult(a,b),c)) FROM t GROUP BY g", kernel="pg_expr_lds")
    finally:
        seg[3].destroy()
        seg[4].destroy()


# ---- tiers --------------------------------------------------------------------------------------------------------------------------------------
def test_tiers_and_their_boundaries(segments, gpu_knobs, gpu_api):
    seg = segments(2047)
    sql = "SELECT g7, SUM(ri * rd) FROM t WHERE s < 900 GROUP BY g7"   # 7 groups x 4 limbs = 28 slots
    _check(seg, sql, kernel="pg_expr_lds")
    _check(seg, "SELECT SUM(ri * rd) FROM t WHERE s < 900", kernel="pg_expr_reg")
    gpu_knobs(PG_EXPR_LDS_MAX_SLOTS=28)
    _check(seg, sql, kernel="pg_expr_lds")           # exactly at the LDS cap
    gpu_knobs(PG_EXPR_LDS_MAX_SLOTS=27)
    _check(seg, sql, kernel="pg_expr_hbm")           # one above it
    gpu_knobs(PG_EXPR_LDS_MAX_SLOTS=27, PG_EXPR_HBM_MAX_BYTES=224)
    _check(seg, sql, kernel="pg_expr_hbm")           # exactly at the HBM budget
    gpu_knobs(PG_EXPR_LDS_MAX_SLOTS=27, PG_EXPR_HBM_MAX_BYTES=223)
    _refused(gpu_api, seg[3], parse_sql(sql), capi.PG_ERR_UNSUPPORTED, "PG_EXPR_HBM_MAX_BYTES")   # one above it: refused
    gpu_knobs(PG_EXPR_LDS_MAX_SLOTS=28, PG_EXPR_HBM_MAX_BYTES=8)
    _check(seg, sql, kernel="pg_expr_lds")           # the LDS tier does not ask the HBM budget


@pytest.mark.parametrize("n", SIZES)
def test_default_tiers(segments, n):
    seg = segments(n)
    every = "SUM(ri * rd), MINMAXRANGE(ri * rd), AVG(add(di,dl)), MIN(rf / df), MAX(dd - rd), SUM(dd - rd)"   # 4 expressions, 17 slots per group
    _check(seg, f"SELECT {every} FROM t WHERE s >= 100", kernel="pg_expr_reg")
    _check(seg, f"SELECT g7, g20, g3, {every} FROM t WHERE s >= 100 GROUP BY g7, g20, g3", kernel="pg_expr_lds")        # 420 x 17 = 7 140 slots
    # one group per doc through a raw INT key: 2 047 x 17 = 34 799 slots are over the LDS cap of 16 384
    _check(seg, f"SELECT rid, {every} FROM t GROUP BY rid", kernel="pg_expr_hbm" if n == 2047 else "pg_expr_lds")
    _check(seg, f"SELECT rid, g3, SUM(ri * rd), COUNT(*) FROM t WHERE s < 800 GROUP BY rid, g3", kernel="pg_expr_hbm" if n == 2047 else "pg_expr_lds")


# ---- group shapes -------------------------------------------------------------------------------------------------------------------------------
SHAPES = [
    "SELECT g7, SUM(ri * rd), AVG(ri * rd) FROM t WHERE s > 5000 GROUP BY g7",                         # a filter matching nothing
    "SELECT SUM(ri * rd), MIN(ri * rd), MAX(ri * rd), AVG(ri * rd), MINMAXRANGE(ri * rd) FROM t WHERE s > 5000",   # ... without GROUP BY: the defaults
    "SELECT gbig, SUM(add(di,dl)), MINMAXRANGE(rd / ri) FROM t GROUP BY gbig",                        # one group holding all but one doc
    "SELECT rg, SUM(ri * rd), MAX(ri + rg) FROM t WHERE s < 800 GROUP BY rg",                          # a raw INT key, also an operand
    "SELECT rdk, AVG(rdk * ri), COUNT(*) FROM t GROUP BY rdk",                                         # a raw DOUBLE key
    "SELECT rs, g3, rg, SUM(rl / ri), COUNT(*) FROM t GROUP BY rs, g3, rg",                            # raw STRING / dictionary / raw INT keys
    "SELECT g7, SUM(ri * rd), SUM(ri + rd), MAX(rd - ri) FROM t GROUP BY g7",                          # expressions sharing columns
    "SELECT g3, SUM(ri * rd), AVG(ri * rd), AVG(times(ri,rd)), MIN(ri * rd) FROM t WHERE s < 600 GROUP BY g3",   # one expression under SUM, AVG and MIN
]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("sql", SHAPES)
def test_shapes(segments, n, sql):
    _check(segments(n), sql)


def test_defaults_over_no_doc(segments):
    gpu = segments(2047)[3]
    got = gpu.execute(SHAPES[1]).aggregation_result()
    assert got == [0.0, float("inf"), float("-inf"), (0.0, 0), (float("inf"), float("-inf"))]


def test_filter_matching_one_doc(segments):
    seg = segments(2047)
    doc = int(np.flatnonzero(seg[1]["gbig"] == 1)[0])
    b = _check(seg, "SELECT g7, SUM(ri * rd), MINMAXRANGE(add(di,dl)) FROM t WHERE gbig = 1 GROUP BY g7")
    assert b.stats.num_docs_scanned == 1 and list(b.rows()) == [(int(seg[1]["g7"][doc]),)]
    _check(seg, "SELECT AVG(rf / df) FROM t WHERE gbig = 1", kernel="pg_expr_reg")


def test_one_evaluation_per_text(segments):
    """SUM and AVG over one text share its accumulators: the sums are the same double"""
    rows = segments(2047)[3].execute("SELECT g7, SUM(ri * rd), AVG(ri * rd) FROM t GROUP BY g7").rows()
    for key, (total, (avg_sum, count)) in rows.items():
        assert pm.same_double(total, avg_sum) and count > 0


def test_next_to_plain_aggregations_and_a_percentile(segments):
    seg = segments(2047)
    host, data, schema, gpu, oracle = seg
    sql = "SELECT g7, COUNT(*), SUM(s), SUM(ri * rd), MAX(s), PERCENTILE(di, 95), AVG(dd - rd), MINMAXRANGE(ri) FROM t WHERE s < 800 GROUP BY g7"
    b = _check(seg, sql, kernel="pg_expr_lds")
    assert b.stats.percentile_passes == 1
    plain = oracle.execute("SELECT g7, COUNT(*), SUM(s), MAX(s), MINMAXRANGE(ri) FROM t WHERE s < 800 GROUP BY g7").rows()
    docs, _ = _filter(oracle, sql)
    groups = pm.group_docs([data["g7"]], docs)
    rows = b.rows()
    for key, want in plain.items():
        assert [rows[key][0], rows[key][1], rows[key][3], rows[key][6]] == want, key
        assert pm.same_runs(rows[key][4], pm.runs(pm.as_doubles(np.asarray(data["di"])[groups[key]], "INT")))
    qf = parse_sql("SELECT SUM(ri * rd), PERCENTILE(di, 50) FROM t")   # ... and its final form, without GROUP BY
    qf.flags |= capi.QUERY_FLAG_FINAL_PERCENTILE
    total, p50 = gpu.execute(qf).aggregation_result()
    assert pm.same_double(total, em.agg_sum(_values(seg, "times(ri,rd)", True))) and p50 == pm.final(pm.as_doubles(data["di"], "INT"), 50.0)


def test_upsert_snapshot(gpu_api, oracle_api):
    host, data, schema = _data(2047, seed=9)
    g, o = NativeSegment(gpu_api, host), NativeSegment(oracle_api, host)
    keep = snapshot_doc_ids(host.total_docs)
    g.set_queryable_doc_ids(keep)
    o.set_queryable_doc_ids(keep)
    try:
        seg = (host, data, schema, g, o)
        b = _check(seg, "SELECT SUM(ri * rd), MIN(rl / ri) FROM t", kernel="pg_expr_reg")
        assert b.stats.num_docs_scanned == len(keep)
        _check(seg, "SELECT g7, AVG(add(di,dl)), COUNT(*) FROM t WHERE s < 600 GROUP BY g7")
    finally:
        g.destroy()
        o.destroy()


def test_num_groups_limit(segments):
    seg = segments(2047)
    plain = parse_sql("SELECT g7, g20, COUNT(*) FROM t WHERE s < 900 GROUP BY g7, g20")
    plain.num_groups_limit = 13
    admitted = set(seg[3].execute(plain).rows())
    assert len(admitted) == 13
    b = _check(seg, "SELECT g7, g20, SUM(ri * rd), COUNT(*) FROM t WHERE s < 900 GROUP BY g7, g20", num_groups_limit=13, admitted=admitted)
    assert b.stats.num_groups_limit_reached == 1


def test_order_by_an_expression_aggregation_is_not_trimmed(segments):
    seg = segments(2047)
    qc = parse_sql("SELECT g7, g20, SUM(ri * rd), COUNT(*) FROM t GROUP BY g7, g20 ORDER BY SUM(ri * rd) DESC LIMIT 1")
    qc.min_segment_group_trim_size = 1
    assert len(seg[3].execute(qc).rows()) == 140        # every group: trimming by an expression aggregation is left to the broker
    qc = parse_sql("SELECT g7, g20, SUM(ri * rd), COUNT(*) FROM t GROUP BY g7, g20 ORDER BY COUNT(*) DESC LIMIT 1")
    qc.min_segment_group_trim_size = 1
    rows = seg[3].execute(qc).rows()
    assert len(rows) == 5                               # max(5 x limit, minSegmentGroupTrimSize), ordered by the remaining aggregation
    v = _values(seg, "times(ri,rd)", True)
    groups = pm.group_docs([seg[1]["g7"], seg[1]["g20"]], np.arange(2047))
    for key, (total, count) in rows.items():
        assert count == len(groups[key]) and pm.same_double(total, em.agg_sum(v[groups[key]]))


def test_data_table_carries_the_column_name(segments):
    host, data, schema, gpu, oracle = segments(2047)
    sql = "SELECT g3, COUNT(*), MAX(ADD(di, ri)), SUM(ri * 1.5), AVG(mult(ri,'1.5')), MINMAXRANGE(sub(sub(sub(sub(sub(sub(sub(ri,rd),rd),rd),rd),rd),rd),rd)) FROM t WHERE s < 500 GROUP BY g3"
    r = gpu.execute_native(sql, keep_device_table=False)
    t = dt.parse_data_table_v4(r.data_table_v4())
    rows = r.block().rows()
    r.free()
    assert t["names"] == ["g3", "count(*)", "max(add(di,ri))", "sum(times(ri,'1.5'))", "avg(mult(ri,'1.5'))",
                          "minmaxrange(sub(sub(sub(sub(sub(sub(sub(ri,rd),rd),rd),rd),rd),rd),rd))"]
    assert t["types"] == ["INT", "LONG", "DOUBLE", "DOUBLE", "OBJECT", "OBJECT"] and len(t["rows"]) == len(rows) == 3
    for g3, count, mx, total, avg, rng in t["rows"]:
        want = rows[(g3,)]
        assert count == want[0] and pm.same_double(mx, want[1]) and pm.same_double(total, want[2])
        assert pm.same_double(avg[0], want[3][0]) and avg[1] == want[3][1] == count       # AvgPair(sum, count)
        assert pm.same_double(rng[0], want[4][0]) and pm.same_double(rng[1], want[4][1])  # MinMaxRangePair(min, max)


def test_division_by_zero_is_refused_by_exec(gpu_api, oracle_api):
    n = 65
    z = np.arange(1, n + 1, dtype=np.int32)
    z[40] = 0
    data = {"a": np.arange(n, dtype=np.int32) + 1, "z": z, "g": (np.arange(n) % 3).astype(np.int32)}
    schema = {"a": "INT", "z": "INT", "g": "INT"}
    host = build_segment("divzero", data, schema, no_dictionary_columns=["z"])
    seg = NativeSegment(gpu_api, host)
    try:
        sql = "SELECT g, SUM(a / z) FROM t WHERE g = 0 GROUP BY g"      # doc 40 is not even in the match set: the bounds pass covers all docs
        gpu_api.call("query_supported", seg.handle, CQuery(parse_sql(sql)).ptr())   # the cache is empty: the shape is let through
        with pytest.raises(capi.NativeError) as e:
            seg.execute(sql)
        assert e.value.status == capi.PG_ERR_UNSUPPORTED and "NaN or an infinity" in e.value.message and "divide(a,z)" in e.value.message
        with pytest.raises(capi.NativeError) as e:                      # ... and answered from the cache afterwards
            gpu_api.call("query_supported", seg.handle, CQuery(parse_sql(sql)).ptr())
        assert e.value.status == capi.PG_ERR_UNSUPPORTED and "NaN or an infinity" in e.value.message
        assert seg.execute("SELECT SUM(z / a) FROM t").aggregation_result() == [em.agg_sum(data["z"].astype(np.float64) / data["a"])]
    finally:
        seg.destroy()


def test_star_tree_route_is_not_taken(gpu_api):
    from tests.fixtures import synth_star_segment
    host = synth_star_segment(num_docs=20_000)
    seg = NativeSegment(gpu_api, host)
    try:
        plain = seg.execute("SELECT h1, COUNT(*), SUM(m) FROM gpuBench GROUP BY h1")
        assert plain.stats.star_tree_index >= 0                      # the star-tree answers the query without an expression ...
        b = seg.execute("SELECT h1, COUNT(*), SUM(m), SUM(m * 2) FROM gpuBench GROUP BY h1")
        assert b.stats.star_tree_index == -1 and b.stats.num_docs_scanned == 20_000   # ... never the one with it
        for key, (count, total, doubled) in b.rows().items():
            assert (count, total) == tuple(plain.rows()[key]) and doubled == 2 * total
    finally:
        seg.destroy()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------
def _refused(gpu_api, seg, qc, status, text):
    for call in ("query_supported", "query_exec"):
        cq = CQuery(qc)
        h = capi.C.c_void_p()
        with pytest.raises(capi.NativeError) as e:
            if call == "query_supported":
                gpu_api.call(call, seg.handle, cq.ptr())
            else:
                gpu_api.call(call, seg.handle, cq.ptr(), capi.C.byref(h))
        assert e.value.status == status and text in e.value.message, (call, e.value.message)


def _spec(function, column, **kw):
    return QueryContext(aggregations=[AggregationSpec(function, column, **kw)])


def test_refusals(gpu_api):
    from pinot_amd.segment import build_column, build_mv_column
    host, data, schema = _data(2047, seed=3)
    rng = np.random.default_rng(1)
    host.columns["by"] = build_column("by", [b"ab%d" % (i % 5) for i in range(host.total_docs)], "BYTES", dictionary=False)
    host.columns["mv"] = build_mv_column("mv", [list(rng.integers(0, 20, rng.integers(1, 4))) for _ in range(host.total_docs)], "INT")
    nulls = np.frombuffer(formats.serialize_roaring(np.array([3, 77, 2000], dtype=np.int64)), dtype=np.uint8)
    host.columns["di"].null_vector = nulls
    host.columns["g20"].null_vector = nulls
    seg = NativeSegment(gpu_api, host)
    try:
        U, I, N = capi.PG_ERR_UNSUPPORTED, capi.PG_ERR_INVALID_ARGUMENT, capi.PG_ERR_NOT_FOUND
        for fn, kw in (("COUNT", {}), ("DISTINCTCOUNT", {}), ("DISTINCTCOUNTHLL", {"log2m": 8}), ("PERCENTILE", {"percentile": 50.0}),
                       ("SUMMV", {}), ("COUNTMV", {}), ("MINMAXRANGEMV", {})):
            _refused(gpu_api, seg, _spec(fn, "add(ri,rd)", **kw), U, fn + " over an expression")
        _refused(gpu_api, seg, parse_sql("SELECT SUM(ri + mv) FROM t"), U, "expression over the multi-value column mv")
        _refused(gpu_api, seg, parse_sql("SELECT SUM(ri + txt) FROM t"), U, "expression over the STRING column txt")
        _refused(gpu_api, seg, parse_sql("SELECT SUM(ri + rs) FROM t"), U, "expression over the STRING column rs")
        _refused(gpu_api, seg, parse_sql("SELECT SUM(ri + by) FROM t"), U, "expression over the BYTES column by")
        _refused(gpu_api, seg, parse_sql("SELECT SUM(mod(ri, 3)) FROM t"), U, "the function mod")
        _refused(gpu_api, seg, parse_sql("SELECT SUM(ri + abs(rd)) FROM t"), U, "the function abs")
        _refused(gpu_api, seg, parse_sql("SELECT mv, SUM(ri * rd) FROM t GROUP BY mv"), U, "next to the multi-value group-by column mv")
        for sql, text in (("SELECT g7, SUM(di * rd) FROM t GROUP BY g7", "expression over di, which holds nulls"),
                          ("SELECT g20, SUM(ri * rd) FROM t GROUP BY g20", "grouped by g20, which holds nulls")):
            qc = parse_sql(sql)
            qc.flags |= capi.QUERY_FLAG_NULL_HANDLING
            _refused(gpu_api, seg, qc, U, text)
        qc = parse_sql("SELECT g7, SUM(ri * rd), SUM(s) FROM t GROUP BY g7")   # columns without nulls run under the flag
        qc.flags |= capi.QUERY_FLAG_NULL_HANDLING
        assert len(seg.execute(qc).rows()) == 7
        _refused(gpu_api, seg, parse_sql("SELECT rid, SUM(ri * rd) FROM t GROUP BY rid, rl, rd, rf"), U, "group key space over 2^32")
        # the limits and the malformed texts, through pg_agg_spec.column as the Java side hands them over
        nine = "add(" + ",".join(["ri", "rd", "di", "dl", "df", "dd", "rl", "rf", "s"]) + ")"
        _refused(gpu_api, seg, _spec("SUM", nine), U, "more than 8 distinct columns")
        _refused(gpu_api, seg, _spec("SUM", "add(" + ",".join(["ri"] * 16) + ")"), U, "more than 15 operations")
        five = QueryContext(aggregations=[AggregationSpec("SUM", f"add(ri,'{k}')") for k in range(5)])
        _refused(gpu_api, seg, five, U, "more than 4 distinct expressions")
        _refused(gpu_api, seg, _spec("SUM", "add(ri,rd"), I, "unbalanced parentheses")
        _refused(gpu_api, seg, _spec("SUM", "add(ri,)"), I, "an empty argument")
        _refused(gpu_api, seg, _spec("SUM", "sub(ri,rd,dd)"), I, "sub takes exactly 2 arguments")
        _refused(gpu_api, seg, _spec("SUM", "add(ri,'5"), I, "unterminated quote")
        _refused(gpu_api, seg, _spec("SUM", "add('1','2')"), I, "expression without a column")
        _refused(gpu_api, seg, _spec("SUM", "add(ri,nosuch)"), N, "column not found: nosuch")
        _refused(gpu_api, seg, _spec("SUM", "add(ri," + "x" * 5000 + ")"), N, "column not found: xxx")
        # a result carrying an expression aggregation is merged by value on the Java side
        a = seg.execute_native("SELECT g7, COUNT(*), SUM(ri * rd) FROM t GROUP BY g7")
        b = seg.execute_native("SELECT g7, COUNT(*), SUM(ri * rd) FROM t GROUP BY g7")
        with pytest.raises(capi.NativeError) as e:
            a.merge(b)
        assert e.value.status == U and "expressions are merged by value" in e.value.message
        b.free()
        # ... and across GPUs: refused before the communicator is used (a world of one rank)
        comm = Comm.init_rank(gpu_api, 0, 1, 0, Comm.unique_id(gpu_api))
        try:
            with pytest.raises(capi.NativeError) as e:
                a.all_reduce(comm)
            assert e.value.status == U and "expressions are merged by value" in e.value.message
        finally:
            comm.destroy()
            a.free()
    finally:
        seg.destroy()


def test_expression_kernels_use_no_scratch():
    """the build leaves hipcc's kernel-resource-usage remarks of pg_kernels_expr.hip behind: no kernel of the path may spill"""
    log = os.path.join(ROOT, "pinot_amd", "csrc", "pg_kernels_expr.resources.log")
    if not os.path.exists(log):
        pytest.skip("library was built without the resource log")
    usage, cur = {}, None
    for line in open(log):
        m = re.search(r"Function Name: (\w+)", line)
        if m:
            cur = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and cur:
            usage[cur] = int(m.group(1))
    for k in ("pg_expr_bounds", "pg_expr_reg", "pg_expr_lds", "pg_expr_hbm", "pg_expr_init", "pg_expr_gather"):
        assert usage.get(k) == 0, (k, usage.get(k))
