"""CASE WHEN inside aggregations on the GPU path (SUM / MIN / MAX / AVG / MINMAXRANGE over case(...) — DESIGN 4.16) against
tests/case_model.py over the ORACLE's match set, bit for bit (MIN / MAX over a mix of 0.0 and -0.0 excepted, as in
tests/test_gpu_expressions.py), with numDocsScanned / numEntriesScannedPostFilter from the model and numEntriesScannedInFilter from the
oracle's filter.  Where a query has a filter twin it is also held to the oracle itself, as the reference's FilteredAggregationsTest does:
SUM(CASE WHEN c THEN x ELSE 0 END) is the oracle's SUM(x) WHERE c, MIN(... ELSE K) the smaller of the twin's MIN and K.

Segments of 2047, 65 and 1 docs: a partial last match word, two words, one doc.  SUM against math.fsum is exact while every non-zero value
lies within 75 binary orders of the segment's largest magnitude: _values() asserts it for every summed text."""
import os
import re

import numpy as np
import pytest

from oracle import po_datatable as dt
from pinot_amd import capi, formats
from pinot_amd.executor import NativeSegment
from pinot_amd.query import AggregationSpec, CQuery, QueryContext, parse_sql
from pinot_amd.segment import build_segment
from tests import case_model as cm
from tests import percentile_model as pm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [2047, 65, 1]   # a partial last match word, two words, one doc
U, I = capi.PG_ERR_UNSUPPORTED, capi.PG_ERR_INVALID_ARGUMENT


def _data(n, seed=23):
    rng = np.random.default_rng(seed + n)
    ints = np.array([-20, -7, -1, 0, 1, 2, 7, 19, 100000], dtype=np.int64)
    longs = np.array([-3_000_000_000, -7, 0, 1, 7, 3_000_000_000, 2**53], dtype=np.int64)      # 2^53 itself is still exact
    floats = np.array([0.5, 1.5, -2.25, 3e3, 0.1, 7.0, 0.0], dtype=np.float32)
    doubles = np.array([0.5, 0.1, -7.0, 1e-3, 123.456, 7.0, 0.123457, 3e3])
    corners = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1.5, -2.0])
    corner_col = rng.choice(corners, n)
    corner_col[: min(n, len(corners))] = corners[: min(n, len(corners))]
    strings = ["a0", "k1", "k2", "k3", "k4", "zz"]                                            # "a0" first and "zz" last in the dictionary
    st = rng.choice(np.array(strings, dtype=object), n)
    st[: min(n, len(strings))] = strings[: min(n, len(strings))]
    z = rng.integers(-3, 4, n).astype(np.int32)
    if n > 3:
        z[3] = 0
    data = {
        "g7": rng.integers(0, 7, n).astype(np.int32), "g3": rng.integers(0, 3, n).astype(np.int32), "rid": (np.arange(n) * 3 - 5).astype(np.int32),
        "s": rng.integers(0, 1000, n).astype(np.int32), "one": (np.arange(n) == n // 2).astype(np.int32),
        "di": rng.choice(ints, n).astype(np.int32), "dl": rng.choice(longs, n), "df": rng.choice(floats, n), "dd": rng.choice(doubles, n),
        "ri": rng.choice(ints, n).astype(np.int32), "rl": rng.choice(longs, n), "rf": rng.choice(floats, n), "rd": rng.choice(doubles, n),
        "m": rng.integers(1, 5000, n).astype(np.int32), "z": z, "a": rng.integers(1, 100, n).astype(np.int32),
        "rdn": corner_col, "big": rng.choice(np.array([1, 2**53 + 2, -5], dtype=np.int64), n),
        "st": st.tolist(), "uni": ["only"] * n, "rs": rng.choice(np.array(strings, dtype=object), n).tolist(),
    }
    schema = {k: "INT" for k in data}
    schema.update(dl="LONG", rl="LONG", big="LONG", df="FLOAT", rf="FLOAT", dd="DOUBLE", rd="DOUBLE", rdn="DOUBLE", st="STRING", uni="STRING", rs="STRING")
    host = build_segment("case_%d" % n, data, schema, no_dictionary_columns=["rid", "ri", "rl", "rf", "rd", "z", "rdn", "big", "rs"])
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
    """the expression's per-doc values over ALL docs, computed once per (segment, text): finite, and for a summed one within 75 binary orders"""
    data, schema = seg[1], seg[2]
    cache = _VALUES.setdefault(id(data), (data, {}))[1]
    if text not in cache:
        v = cm.evaluate(text, data, schema)
        assert np.all(np.isfinite(v)), text
        nz = np.abs(v[v != 0.0])
        cache[text] = (v, int(np.frexp(nz.max())[1] - np.frexp(nz.min())[1]) if nz.size else 0)
    v, spread = cache[text]
    if summed:
        assert spread <= 75, (text, spread)
    return v


def _filter(oracle, sql):
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


def _check(seg, sql, kernel=None, flags=0):
    """Runs `sql` on the GPU and holds every aggregation over an expression and every COUNT(*), the groups and the statistics to the model."""
    host, data, schema, gpu, oracle = seg
    qc = parse_sql(sql)
    qc.flags |= flags
    docs, in_filter = _filter(oracle, sql)
    groups = pm.group_docs([data[g] for g in qc.group_by], docs) if qc.group_by else {(): np.asarray(docs, dtype=np.int64)}
    b = gpu.execute(qc)
    rows = b.rows()
    assert set(rows) == set(groups), sql
    read = set(qc.group_by)
    for a in qc.aggregations:
        if _is_expression(a):
            read |= set(cm.columns_of(a.column))
        elif a.column:
            read.add(a.column)
    assert (b.stats.num_docs_scanned, b.stats.num_entries_scanned_post_filter) == pm.statistics(len(docs), read), sql
    assert b.stats.num_entries_scanned_in_filter == in_filter and b.stats.stats_exact == 1 and b.stats.num_total_docs == host.total_docs, sql
    if kernel is not None:
        assert b.stats.kernel.decode() == kernel, sql
    for key, gdocs in groups.items():
        for a, spec in enumerate(qc.aggregations):
            if spec.function == "COUNT":
                assert rows[key][a] == len(gdocs), (sql, key)
            if not _is_expression(spec):
                continue
            v = _values(seg, spec.column, spec.function in ("SUM", "AVG"))[gdocs]
            want = cm.aggregate(spec.function, v)
            assert _same_result(spec.function, rows[key][a], want), (sql, key, spec, rows[key][a], want)
    return b


def _sum_twin(seg, cond, x, where=""):
    """SUM(CASE WHEN cond THEN x ELSE 0 END) [WHERE w] against the oracle's SUM(x) WHERE cond [AND w] (x an INT / LONG column: both sums exact)"""
    b = _check(seg, f"SELECT SUM(CASE WHEN {cond} THEN {x} ELSE 0 END) FROM t" + (f" WHERE {where}" if where else ""), kernel="pg_expr_reg")
    twin = seg[4].execute(f"SELECT SUM({x}) FROM t WHERE {cond}" + (f" AND {where}" if where else "")).aggregation_result()
    assert b.aggregation_result() == twin, (cond, x, where)


# ---- the operand matrix -------------------------------------------------------------------------------------------------------------------------
OPS = ["=", "<>", ">", ">=", "<", "<="]
COLUMNS = ["di", "dl", "df", "dd", "ri", "rl", "rf", "rd"]
LITERALS = ["7", "3000000000", "0.5", "-7", "0.123457", "-3000000000", "1.5", "0"]   # INT, LONG and DOUBLE by their texts
PAIRS = [("di", "rl"), ("rf", "dd"), ("dl", "rd"), ("ri", "df"), ("rd", "dd"), ("rl", "di"), ("df", "rf"), ("dd", "ri")]


def _matrix(op):
    """every column against a literal on the right, on the left, and against another column"""
    right = [f"SUM(CASE WHEN {c} {op} {LITERALS[(i + OPS.index(op)) % 8]} THEN m ELSE 0 END)" for i, c in enumerate(COLUMNS)]
    left = [f"SUM(CASE WHEN {LITERALS[(i + 3 + OPS.index(op)) % 8]} {op} {c} THEN m ELSE 0 END)" for i, c in enumerate(COLUMNS)]
    pairs = [f"SUM(CASE WHEN {a} {op} {b} THEN m ELSE 0 END)" for a, b in PAIRS]
    out = []
    for items in (right, left):   # four condition columns and m
        out += ["SELECT " + ", ".join(items[:4]) + " FROM t", "SELECT g3, " + ", ".join(items[4:]) + " FROM t WHERE s < 800 GROUP BY g3"]
    # three pairs and m are seven columns: a query's expressions share eight
    return out + ["SELECT " + ", ".join(pairs[:3]) + " FROM t", "SELECT g3, " + ", ".join(pairs[3:6]) + " FROM t WHERE s < 800 GROUP BY g3",
                  "SELECT " + ", ".join(pairs[6:]) + " FROM t WHERE s >= 200"]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("op", OPS)
def test_operand_matrix(segments, n, op):
    for sql in _matrix(op):
        _check(segments(n), sql)


def test_the_matrix_separates_the_operators(segments):
    """the data holds the literals: = matches some docs and not all, for every column type (an edit of the data cannot make the matrix vacuous)"""
    seg = segments(2047)
    for col, lit in (("di", "7"), ("rl", "3000000000"), ("df", "0.5"), ("rd", "0.123457"), ("dl", "-7"), ("rf", "1.5")):
        v = _values(seg, parse_sql(f"SELECT SUM(CASE WHEN {col} = {lit} THEN 1 ELSE 0 END) FROM t").aggregations[0].column, True)
        assert 0 < v.sum() < 2047, (col, lit)


@pytest.mark.parametrize("n", SIZES)
def test_filter_twins(segments, n):
    seg = segments(n)
    _sum_twin(seg, "s > 500", "m")
    _sum_twin(seg, "di >= 2", "ri")
    _sum_twin(seg, "rl = 3000000000", "m", where="g7 < 5")
    _sum_twin(seg, "dd < 0.5", "di")
    _sum_twin(seg, "st = 'k2'", "m")
    # MIN(... ELSE K): the smaller of the twin's MIN and K when a doc fails the condition
    K = 9999999
    b = _check(seg, f"SELECT MIN(CASE WHEN m > 2500 THEN m ELSE {K} END), MAX(CASE WHEN m > 2500 THEN m ELSE -1 END) FROM t", kernel="pg_expr_reg")
    low, high = seg[4].execute("SELECT MIN(m), MAX(m) FROM t WHERE m > 2500").aggregation_result()
    fails = bool(np.any(seg[1]["m"] <= 2500))
    assert b.aggregation_result() == [min(low, K) if fails else low, max(high, -1.0) if fails else high]


# ---- selection ----------------------------------------------------------------------------------------------------------------------------------
SELECTION = [
    "SELECT SUM(CASE WHEN m > 3000 THEN 3 WHEN m > 2000 THEN 2 WHEN m > 1000 THEN 1 ELSE -1 END) FROM t",                       # three overlapping WHENs
    "SELECT g7, SUM(CASE WHEN m > 1000 THEN 1 WHEN m > 2000 THEN 2 WHEN m > 3000 THEN 3 ELSE -1 END), COUNT(*) FROM t GROUP BY g7",   # the first hides the others
    "SELECT SUM(CASE WHEN di > 0 AND ri > 0 THEN m ELSE 0 END), SUM(CASE WHEN di > 0 OR ri > 0 THEN m ELSE 0 END), SUM(CASE WHEN NOT di > 0 THEN m ELSE 0 END) FROM t",
    "SELECT g3, SUM(CASE WHEN (di > 0 OR rd < 1) AND NOT (rf = 0.5 OR dl <> 7 AND m > 100) THEN m ELSE 1 END) FROM t WHERE s < 900 GROUP BY g3",
    "SELECT SUM(CASE WHEN NOT (NOT (di = 7 AND (ri = 7 OR (rl > 0 AND rf < 2)))) THEN m END) FROM t",                            # nested, no ELSE: 0.0
    "SELECT SUM(CASE WHEN s < 500 THEN 1 ELSE 0 END), AVG(CASE WHEN st = 'k1' THEN 1 ELSE 0 END) FROM t",                       # literal-only branches: a conditional count
    "SELECT g7, SUM(CASE WHEN a > 50 THEN m * rd ELSE 0 END), MAX(CASE WHEN a > 50 THEN m - a ELSE m + a END) FROM t GROUP BY g7",    # arithmetic branches
    "SELECT SUM(CASE WHEN a > 50 THEN CASE WHEN m > 2500 THEN rd ELSE di END ELSE 0.25 END), MIN(CASE WHEN a < 10 THEN CASE WHEN di > 0 THEN di END ELSE m END) FROM t",
    "SELECT g3, SUM(m * CASE WHEN a > 50 THEN 1 ELSE 0 END), SUM(mult(case(greater_than(a,50),1,0),m)), AVG(2 + CASE WHEN di < 0 THEN rd ELSE dd END / a) FROM t GROUP BY g3",
    "SELECT SUM(CASE WHEN a + m > 2500 THEN m ELSE 0 END), SUM(CASE WHEN m / a >= rd * 2 THEN 1 ELSE 0 END) FROM t WHERE s >= 100",   # arithmetic operands of a comparison
]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("sql", SELECTION)
def test_selection(segments, n, sql):
    _check(segments(n), sql)


def test_priority_is_observed(segments):
    seg = segments(2047)
    m = seg[1]["m"].astype(np.int64)
    got = seg[3].execute(SELECTION[0]).aggregation_result()[0]
    assert got == float(np.where(m > 3000, 3, np.where(m > 2000, 2, np.where(m > 1000, 1, -1))).sum())
    got = seg[3].execute("SELECT SUM(CASE WHEN m > 1000 THEN 1 WHEN m > 2000 THEN 2 WHEN m > 3000 THEN 3 ELSE -1 END) FROM t").aggregation_result()[0]
    assert got == float(np.where(m > 1000, 1, -1).sum())


# ---- Double.compare ---------------------------------------------------------------------------------------------------------------------------------
CORNERS = ["rdn = 0", "rdn > 0", "rdn < 0", "rdn >= 0", "rdn <= -0.0", "rdn <> 0", "rdn > 1e308", "rdn < -1e308", "rdn = rdn", "rdn > rd", "rdn >= 1.5"]


@pytest.mark.parametrize("n", SIZES)
def test_double_compare_corners(segments, n):
    """a DOUBLE condition column holding 0.0, -0.0, NaN and +-Inf, finite branches: -0.0 is below 0.0, NaN equals NaN and is above +Infinity"""
    seg = segments(n)
    for k in range(0, len(CORNERS), 4):
        _check(seg, "SELECT " + ", ".join(f"SUM(CASE WHEN {c} THEN m ELSE 0 END)" for c in CORNERS[k:k + 4]) + " FROM t", kernel="pg_expr_reg")
    if n == 2047:
        rdn, m = seg[1]["rdn"], seg[1]["m"].astype(np.float64)
        neg_zero = (rdn == 0) & np.signbit(rdn)
        got = seg[3].execute("SELECT SUM(CASE WHEN rdn = 0 THEN m ELSE 0 END), SUM(CASE WHEN rdn < 0 THEN m ELSE 0 END), SUM(CASE WHEN rdn > 1e308 THEN m ELSE 0 END) FROM t").aggregation_result()
        assert neg_zero.any() and np.isnan(rdn).any()
        assert got == [m[(rdn == 0) & ~neg_zero].sum(), m[(rdn < 0) | neg_zero].sum(), m[np.isnan(rdn) | (rdn == np.inf)].sum()]


# ---- only the selected value counts -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_division_guard(segments, gpu_api, n):
    seg = segments(n)
    _check(seg, "SELECT SUM(CASE WHEN z <> 0 THEN a / z ELSE 0 END), MINMAXRANGE(CASE WHEN z <> 0 THEN a / z ELSE 0 END) FROM t", kernel="pg_expr_reg")
    _check(seg, "SELECT g3, AVG(CASE WHEN z = 0 THEN -1 ELSE m / z END) FROM t GROUP BY g3")
    if n > 3:   # a zero among the divisors: the unguarded quotient is still refused
        with pytest.raises(capi.NativeError) as e:
            seg[3].execute("SELECT SUM(a / z) FROM t")
        assert e.value.status == U and "NaN or an infinity" in e.value.message


# ---- typing -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_float_typing(segments, gpu_api, n):
    seg = segments(n)
    # FLOAT columns and INT / LONG literals make a FLOAT: 16777217 and 3000000001 are narrowed with (float); a DOUBLE literal keeps them
    b = _check(seg, "SELECT SUM(CASE WHEN a > 50 THEN rf ELSE 16777217 END), MAX(CASE WHEN a > 50 THEN df WHEN a > 20 THEN 3000000001 ELSE rf END), "
                    "SUM(CASE WHEN a > 50 THEN rf WHEN a > 20 THEN 0.5 ELSE 16777217 END) FROM t", kernel="pg_expr_reg")
    if n == 2047:
        a, rf = seg[1]["a"], seg[1]["rf"].astype(np.float64)
        assert b.aggregation_result()[0] == float(np.where(a > 50, rf, 16777216.0).sum())
        assert b.aggregation_result()[1] == float(np.float32(3000000001))
    _check(seg, "SELECT SUM(CASE WHEN a > 50 THEN CASE WHEN a > 70 THEN rf ELSE 16777217 END ELSE 1.5 END) FROM t")   # a FLOAT CASE inside a DOUBLE one
    for sql, text in (("SELECT SUM(CASE WHEN a > 50 THEN rf ELSE di END) FROM t", "a FLOAT-typed CASE with the INT column di"),
                      ("SELECT SUM(CASE WHEN a > 50 THEN rl ELSE df END) FROM t", "a FLOAT-typed CASE with the LONG column rl"),
                      ("SELECT SUM(CASE WHEN a > 50 THEN rf ELSE CASE WHEN a > 3 THEN 1 ELSE 2 END END) FROM t", "a FLOAT-typed CASE with an INT-typed CASE")):
        _refused(gpu_api, seg[3], parse_sql(sql), U, text)


# ---- STRING equality ------------------------------------------------------------------------------------------------------------------------------------
STRINGS = ["st = 'k2'", "st <> 'k2'", "st != 'a0'", "st = 'zz'", "st = 'nosuch'", "st <> 'nosuch'", "'k3' = st", "uni = 'only'", "uni <> 'only'", "uni = 'other'",
           "st = 'k1' AND m > 2500", "st = 'k4' OR NOT (uni = 'only' AND di > 0)", "st = '7'"]


@pytest.mark.parametrize("n", SIZES)
def test_string_equality(segments, n):
    seg = segments(n)
    for k in range(0, len(STRINGS), 4):
        _check(seg, "SELECT " + ", ".join(f"SUM(CASE WHEN {c} THEN m ELSE 0 END)" for c in STRINGS[k:k + 4]) + " FROM t")
    b = _check(seg, "SELECT g7, SUM(CASE WHEN st = 'k2' THEN m ELSE 0 END), COUNT(*) FROM t WHERE st <> 'k3' GROUP BY g7")
    assert b.stats.num_entries_scanned_post_filter == 3 * b.stats.num_docs_scanned      # g7, st, m: the condition column counts


# ---- aggregations, tiers, combinations ------------------------------------------------------------------------------------------------------------------
EVERY = "CASE WHEN di > 0 THEN rd ELSE dd END"


@pytest.mark.parametrize("n", SIZES)
def test_every_aggregation_and_every_tier(segments, gpu_knobs, n):
    seg = segments(n)
    aggs = f"SUM({EVERY}), MIN({EVERY}), MAX({EVERY}), AVG({EVERY}), MINMAXRANGE({EVERY}), SUM(case(greaterthan(di,'0'),rd,dd))"
    b = _check(seg, f"SELECT {aggs} FROM t", kernel="pg_expr_reg")
    r = b.aggregation_result()
    assert pm.same_double(r[0], r[3][0]) and pm.same_double(r[0], r[5]) and r[3][1] == n       # one evaluation per text
    _check(seg, f"SELECT g7, {aggs} FROM t WHERE s < 900 GROUP BY g7", kernel="pg_expr_lds")
    gpu_knobs(PG_EXPR_LDS_MAX_SLOTS=6)                                                         # a group's row alone has 7 slots
    _check(seg, f"SELECT g7, {aggs} FROM t WHERE s < 900 GROUP BY g7", kernel="pg_expr_hbm")


def test_combinations(segments):
    seg = segments(2047)
    host, data, schema, gpu, oracle = seg
    b = _check(seg, f"SELECT g7, SUM({EVERY}), MINMAXRANGE(CASE WHEN st = 'k1' THEN m END) FROM t WHERE one = 1 GROUP BY g7")     # a filter matching one doc
    assert b.stats.num_docs_scanned == 1
    none = f"SELECT SUM({EVERY}), MIN({EVERY}), MAX({EVERY}), AVG({EVERY}), MINMAXRANGE({EVERY}) FROM t WHERE s > 5000"             # ... and none
    _check(seg, none, kernel="pg_expr_reg")
    assert gpu.execute(none).aggregation_result() == [0.0, float("inf"), float("-inf"), (0.0, 0), (float("inf"), float("-inf"))]
    sql = f"SELECT g7, COUNT(*), SUM(s), SUM({EVERY}), MAX(s), PERCENTILE(di, 95), AVG(CASE WHEN st <> 'zz' THEN ri * rd END) FROM t WHERE s < 800 GROUP BY g7"
    b = _check(seg, sql, kernel="pg_expr_lds")
    assert b.stats.percentile_passes == 1
    plain = oracle.execute("SELECT g7, COUNT(*), SUM(s), MAX(s) FROM t WHERE s < 800 GROUP BY g7").rows()
    groups = pm.group_docs([data["g7"]], _filter(oracle, sql)[0])
    for key, want in plain.items():
        row = b.rows()[key]
        assert [row[0], row[1], row[3]] == want, key
        assert pm.same_runs(row[4], pm.runs(pm.as_doubles(np.asarray(data["di"])[groups[key]], "INT")))
    _check(seg, f"SELECT g3, SUM({EVERY}), AVG(CASE WHEN st = 'k1' THEN m ELSE 0 END) FROM t GROUP BY g3", flags=capi.QUERY_FLAG_NULL_HANDLING)   # no nulls, an ELSE
    qc = parse_sql(f"SELECT g7, SUM({EVERY}), COUNT(*) FROM t GROUP BY g7 ORDER BY SUM(case when di>0 then rd else dd end) DESC LIMIT 3")
    qc.min_segment_group_trim_size = 1
    assert qc.resolved_order_by() == [(capi.ORDER_BY_AGGREGATION, 0, False)]
    assert len(gpu.execute(qc).rows()) == 7                                                     # an ORDER BY naming it leaves the segment untrimmed


def test_data_table_carries_the_column_name(segments):
    host, data, schema, gpu, oracle = segments(2047)
    sql = "SELECT g3, COUNT(*), SUM(CASE WHEN a > 5 THEN a ELSE 0 END), AVG(case when st = 'k1' then 1 end), MAX(case(greater_than(a,5),a,0)) FROM t WHERE s < 500 GROUP BY g3"
    r = gpu.execute_native(sql, keep_device_table=False)
    t = dt.parse_data_table_v4(r.data_table_v4())
    rows = r.block().rows()
    r.free()
    assert t["names"] == ["g3", "count(*)", "sum(case(greaterthan(a,'5'),a,'0'))", "avg(case(equals(st,'k1'),'1','null'))", "max(case(greaterthan(a,'5'),a,'0'))"]
    assert t["types"] == ["INT", "LONG", "DOUBLE", "OBJECT", "DOUBLE"] and len(t["rows"]) == len(rows) == 3
    for g3, count, total, avg, mx in t["rows"]:
        want = rows[(g3,)]
        assert count == want[0] and pm.same_double(total, want[1]) and pm.same_double(avg[0], want[2][0]) and avg[1] == want[2][1] == count and pm.same_double(mx, want[3])


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


def _spec(function, column):
    return QueryContext(aggregations=[AggregationSpec(function, column)])


def test_refusals(gpu_api):
    host, data, schema = _data(2047, seed=5)
    host.columns["di"].null_vector = np.frombuffer(formats.serialize_roaring(np.array([3, 77, 2000], dtype=np.int64)), dtype=np.uint8)
    seg = NativeSegment(gpu_api, host)
    try:
        case = "CASE WHEN a > 5 THEN a ELSE 0 END"
        _refused(gpu_api, seg, parse_sql(f"SELECT COUNT(*) FROM t WHERE {case} > 3"), U, "in a WHERE predicate")
        _refused(gpu_api, seg, parse_sql(f"SELECT {case}, COUNT(*) FROM t GROUP BY {case}"), U, "as a GROUP BY / DISTINCT key")
        _refused(gpu_api, seg, parse_sql(f"SELECT DISTINCT {case} FROM t"), U, "as a GROUP BY / DISTINCT key")
        _refused(gpu_api, seg, _spec("SUM", "greater_than(a,'5')"), U, "greaterthan outside a WHEN")
        _refused(gpu_api, seg, _spec("SUM", "add(a,equals(a,'5'))"), U, "equals outside a WHEN")
        _refused(gpu_api, seg, parse_sql("SELECT SUM(CASE WHEN rs = 'k1' THEN 1 ELSE 0 END) FROM t"), U, "the raw STRING column rs")
        _refused(gpu_api, seg, _spec("SUM", "case(greater_than(st,'5'),'1','0')"), U, "an ordering comparison over the STRING column st")
        _refused(gpu_api, seg, _spec("SUM", "case(greater_than(st,'k1'),'1','0')"), I, "not a decimal number")
        _refused(gpu_api, seg, _spec("SUM", "case(equals(st,uni),'1','0')"), U, "compared with something other than a literal")
        _refused(gpu_api, seg, _spec("SUM", "case(equals(a,'1'),st,'0')"), U, "expression over the STRING column st")
        _refused(gpu_api, seg, _spec("SUM", "case(equals(a,'k1'),'1','0')"), I, "the literal 'k1' is not a decimal number")
        _refused(gpu_api, seg, parse_sql("SELECT SUM(CASE WHEN big > 5 THEN 1 ELSE 0 END) FROM t"), U, "the LONG column big, whose values reach beyond 2^53")
        _refused(gpu_api, seg, parse_sql("SELECT SUM(CASE WHEN rl < 9007199254740993 THEN 1 ELSE 0 END) FROM t"), U, "LONG literal 9007199254740993, beyond 2^53")
        _refused(gpu_api, seg, parse_sql("SELECT SUM(CASE WHEN a > 50 THEN rf ELSE ri END) FROM t"), U, "a FLOAT-typed CASE with the INT column ri")
        _refused(gpu_api, seg, parse_sql("SELECT SUM(CASE WHEN mod(a, 3) = 0 THEN 1 ELSE 0 END) FROM t"), U, "the function mod")
        _refused(gpu_api, seg, _spec("COUNT", "case(equals(a,'1'),'1','0')"), U, "COUNT over an expression")
        _refused(gpu_api, seg, _spec("SUM", "case(equals(a,'1'),'1')"), I, "odd number of arguments")
        for sql, text in ((f"SELECT SUM(CASE WHEN a > 5 THEN a END) FROM t", "a CASE without ELSE"),
                          (f"SELECT SUM(CASE WHEN di > 5 THEN a ELSE 0 END) FROM t", "expression over di, which holds nulls")):
            qc = parse_sql(sql)
            qc.flags |= capi.QUERY_FLAG_NULL_HANDLING
            _refused(gpu_api, seg, qc, U, text)
        assert seg.execute("SELECT SUM(CASE WHEN di > 5 THEN a ELSE 0 END) FROM t").aggregation_result()[0] > 0      # ... and runs without the flag
        big_then = seg.execute("SELECT MAX(CASE WHEN a > 0 THEN big ELSE 0 END) FROM t").aggregation_result()     # beyond 2^53 as a BRANCH: cast like any operand
        assert big_then == [float(2**53 + 2)]
    finally:
        seg.destroy()


def test_expression_kernels_use_no_scratch():
    """the build leaves hipcc's kernel-resource-usage remarks behind: the select must not turn the register-indexed vectors into scratch"""
    for name, kernels in (("pg_kernels_expr", ("pg_expr_bounds", "pg_expr_reg", "pg_expr_lds", "pg_expr_hbm")), ("pg_kernels_exprpred", ("pg_expr_pred",)),
                          ("pg_kernels_exprkey", ("pg_expr_keys",))):
        log = os.path.join(ROOT, "pinot_amd", "csrc", name + ".resources.log")
        assert os.path.exists(log), log
        usage, cur = {}, None
        for line in open(log):
            m = re.search(r"Function Name: (\w+)", line)
            if m:
                cur = m.group(1)
            m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
            if m and cur:
                usage[cur] = int(m.group(1))
        for k in kernels:
            assert usage.get(k) == 0, (k, usage.get(k))
