"""COVAR_POP / COVAR_SAMP on the GPU path (PG_AGG_COVARPOP / PG_AGG_COVARSAMP) against tests/covariance_model.py over the ORACLE's match set
and group assignment: the tuple (sumX, sumY, sumXY, count) bit for bit the Fraction model's on data inside the documented window (checked
with the model itself, so the model alone decides), the statistics from the model and the oracle's filter, and the tuple's members bit
for bit what SUM(x), SUM(y), SUM(x * y) and COUNT(*) of the same query return.  The kernel names of the path (pg_covar_reg / pg_covar_reg_wide /
pg_covar_lds / pg_covar_hbm) are tied to the model here, not to the oracle, which has no covariance."""
import os
import re
import threading

import numpy as np
import pytest

from oracle import po_datatable as dt
from pinot_amd import capi, formats
from pinot_amd.executor import NativeSegment, covariance_final
from pinot_amd.query import CQuery, parse_sql
from pinot_amd.segment import build_segment
from tests import covariance_model as cm
from tests import percentile_model as pm
from tests import variance_model as vm
from tests.kernel_inventory import snapshot_doc_ids

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = cm.header_constants()
LDS_SLOTS = K["PG_COVAR_LDS_SLOTS"]
PAIR_SLOTS = cm.slots_per_group(["DOUBLE", "DOUBLE"], 1, K)   # one pair of two non-INT columns: count, two sums, the products
G_FIT = LDS_SLOTS // PAIR_SLOTS                               # the last key space whose table of such a pair fits pg_covar_lds
SCHEMA_OF = {"xi": "INT", "ri": "INT", "xl": "LONG", "rl": "LONG", "xf": "FLOAT", "rf": "FLOAT", "xd": "DOUBLE", "rd": "DOUBLE"}
# mixed pairs: every kind as dictionary-encoded (x*) and as raw (r*) column, with itself among them
MIXED = [("xi", "rd"), ("rl", "xf"), ("xd", "ri"), ("rf", "xl"), ("xi", "ri"), ("rl", "xl"), ("rd", "rd"), ("xf", "xf")]
# the reference's own query (StatisticalQueriesTest): 8 covariances over 6 columns
REFERENCE_8 = [("xi", "ri"), ("xd", "rd"), ("xi", "xd"), ("xi", "rl"), ("xi", "xf"), ("xd", "rl"), ("xd", "xf"), ("rl", "xf")]


def _data(n, seed=23):
    """data inside the windows: the non-zero magnitudes of every FLOAT / DOUBLE column span less than 2^10"""
    rng = np.random.default_rng(seed + n)
    sign = lambda: np.where(rng.integers(0, 2, n) == 0, -1.0, 1.0)   # noqa: E731
    data = {
        "g7": rng.integers(0, 7, n).astype(np.int32), "g20": rng.integers(0, 20, n).astype(np.int32), "g2": (np.arange(n) % 2).astype(np.int32),
        "s": rng.integers(0, 1000, n).astype(np.int32), "c_inv1": rng.integers(0, 8, n).astype(np.int32),
        "kfit": (np.arange(n) % G_FIT).astype(np.int32), "kover": (np.arange(n) % (G_FIT + 1)).astype(np.int32),
        # INT x INT products pass 2^53: (double) x * (double) y rounds
        "xi": rng.integers(-5000, 5000, n).astype(np.int32) * 400_003, "ri": rng.integers(-2**31, 2**31 - 1, n, dtype=np.int64).astype(np.int32),
        "xl": rng.integers(-300, 300, n).astype(np.int64) * 10**15 + 1, "rl": rng.integers(-2**62, 2**62, n, dtype=np.int64),
        "xf": (rng.choice(rng.uniform(1.0, 1000.0, 97), n) * sign()).astype(np.float32), "rf": (rng.uniform(1.0, 1000.0, n) * sign()).astype(np.float32),
        "xd": rng.choice(rng.uniform(1e-3, 1.0, 211), n) * sign(), "rd": (1e9 + rng.standard_normal(n)),
        "u1": rng.permutation(n).astype(np.int32), "u2": rng.permutation(n).astype(np.int32), "u3": rng.permutation(n).astype(np.int32),
        "txt": np.array(["t%d" % v for v in rng.integers(0, 5, n)], dtype=object).tolist(),
    }
    data["rl"][rng.integers(0, n, 3)] = 2**62 + 1      # LONGs that are no doubles
    schema = {k: "INT" for k in data}
    schema.update(SCHEMA_OF)
    schema.update(txt="STRING")
    host = build_segment("covar_%d" % n, data, schema, inverted_index_columns=["c_inv1"], no_dictionary_columns=["ri", "rl", "rf", "rd"])
    return host, data, schema


_SEGMENTS = {}
_WINDOW_CHECKED = set()


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


def _filter(oracle, sql):
    """(matching docs, numEntriesScannedInFilter) of the query's filter, from the oracle"""
    where = sql.split(" FROM ", 1)[1].split(" GROUP BY ")[0].split(" ORDER BY ")[0].split(" LIMIT ")[0]
    ds = oracle.filter("SELECT COUNT(*) FROM " + where)
    docs, st = ds.doc_ids(), ds.stats()
    ds.free()
    return docs, st.num_entries_scanned_in_filter


def _norm(key):
    return tuple(float(k) if isinstance(k, (int, float, np.integer, np.floating)) else k for k in key)


def _same_tuple(got, want):
    return all(cm.same_bits(g, w) for g, w in zip(got[:3], want[:3])) and got[3] == want[3]


def _doubles(data, schema, col, docs=None):
    v = np.asarray(data[col])
    return cm.as_doubles(v if docs is None else v[docs], schema[col])


def _inside_the_window(host, data, schema, x, y):
    """the whole columns lie inside the documented window (the column bounds are the segment's): the model alone decides the expected bits"""
    key = (host.name if hasattr(host, "name") else id(host), host.total_docs, x, y)
    if key not in _WINDOW_CHECKED:
        assert cm.in_exact_window(_doubles(data, schema, x), _doubles(data, schema, y), schema[x], schema[y], K), (x, y)
        _WINDOW_CHECKED.add(key)


def _check(seg, sql, kernel=None, num_groups_limit=0, admitted=None, qc=None):
    """Runs `sql` on the GPU and holds every covariance aggregation and COUNT(*) of it, its groups and its statistics to the model."""
    host, data, schema, gpu, oracle = seg
    qc = qc or parse_sql(sql)
    qc.num_groups_limit = num_groups_limit
    docs, in_filter = _filter(oracle, sql)
    groups = pm.group_docs([np.asarray(data[g]) for g in qc.group_by], docs) if qc.group_by else {(): np.asarray(docs, dtype=np.int64)}
    groups = {_norm(k): v for k, v in groups.items()}
    if admitted is not None:
        groups = {k: v for k, v in groups.items() if k in admitted}
    b = gpu.execute(qc)
    rows = {_norm(k): v for k, v in b.rows().items()}
    assert set(rows) == set(groups), sql
    read = set(qc.group_by)
    for a in qc.aggregations:   # every distinct column once, however many pairs name it; an expression's operand columns once each
        read |= set(re.findall(r"[A-Za-z_]\w*", a.column)) & set(data) if a.column else set()
    assert (b.stats.num_docs_scanned, b.stats.num_entries_scanned_post_filter) == pm.statistics(len(docs), read), sql
    assert b.stats.num_entries_scanned_in_filter == in_filter and b.stats.stats_exact == 1 and b.stats.num_total_docs == host.total_docs, sql
    assert b.stats.star_tree_index == -1
    if kernel is not None:
        assert b.stats.kernel.decode() == kernel, sql
    for a, spec in enumerate(qc.aggregations):
        if spec.function in cm.FUNCTIONS:
            x, y = spec.column.split(",")
            _inside_the_window(host, data, schema, x, y)
    for key, gdocs in groups.items():
        for a, spec in enumerate(qc.aggregations):
            if spec.function == "COUNT":
                assert rows[key][a] == len(gdocs), (sql, key)
            if spec.function not in cm.FUNCTIONS:
                continue
            x, y = spec.column.split(",")
            want = cm.exact_tuple(_doubles(data, schema, x, gdocs), _doubles(data, schema, y, gdocs))
            assert _same_tuple(rows[key][a], want), (sql, key, spec, rows[key][a], want)
            assert cm.same_bits(covariance_final(spec.function, rows[key][a]), cm.final(spec.function, want)), (sql, key, spec)
    return b


def _aggs(pairs):
    fns = ("COVAR_POP", "COVAR_SAMP")
    return ", ".join(f"{fns[i % 2]}({x}, {y})" for i, (x, y) in enumerate(pairs))


# ---- doc counts and layouts ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 2049])
def test_doc_counts_and_column_layouts(segments, n):
    """INT / LONG / FLOAT / DOUBLE arguments, dictionary-encoded and raw, in mixed pairs and with themselves, with and without a filter,
    without GROUP BY and with one column"""
    seg = segments(n)
    for where in ("", " WHERE s < 500"):
        _check(seg, f"SELECT {_aggs(MIXED)}, COUNT(*) FROM t{where}", kernel="pg_covar_reg_wide")
        _check(seg, f"SELECT COVAR_POP(xi, rd), COVAR_SAMP(xi, rd), COUNT(*) FROM t{where}", kernel="pg_covar_reg")   # one pair: the narrow register kernel
        _check(seg, f"SELECT COVAR_SAMP(rf, rf) FROM t{where}", kernel="pg_covar_reg")
        _check(seg, f"SELECT g7, {_aggs(MIXED)} FROM t{where} GROUP BY g7", kernel="pg_covar_lds")


# ---- tiers ------------------------------------------------------------------------------------------------------------------------------------------------
def test_tier_boundary_and_the_hbm_budget(segments, gpu_knobs, gpu_api):
    assert (G_FIT * PAIR_SLOTS <= LDS_SLOTS < (G_FIT + 1) * PAIR_SLOTS) and G_FIT > 1000
    seg = segments(20011)
    fit = "SELECT kfit, COVAR_POP(rd, xd) FROM t WHERE s < 900 GROUP BY kfit"
    over = "SELECT kover, COVAR_POP(rd, xd) FROM t WHERE s < 900 GROUP BY kover"
    _check(seg, fit, kernel="pg_covar_lds")         # the last table that fits the workgroup's LDS
    _check(seg, over, kernel="pg_covar_hbm")        # one group more
    _check(seg, "SELECT kover, COVAR_SAMP(ri, xi), COVAR_POP(xd, rl), COUNT(*) FROM t GROUP BY kover", kernel="pg_covar_hbm")   # integer slots too, no match words
    table_bytes = (G_FIT + 1) * PAIR_SLOTS * 8
    gpu_knobs(PG_COVAR_HBM_MAX_BYTES=table_bytes)
    _check(seg, over, kernel="pg_covar_hbm")        # exactly at the budget
    gpu_knobs(PG_COVAR_HBM_MAX_BYTES=table_bytes - 1)
    _refused(gpu_api, seg[3], parse_sql(over), capi.PG_ERR_UNSUPPORTED, "more than PG_COVAR_HBM_MAX_BYTES")
    _check(seg, fit, kernel="pg_covar_lds")         # the LDS tier does not ask the budget


# ---- query shapes -----------------------------------------------------------------------------------------------------------------------------------------
SHAPES = [
    "SELECT g7, g20, COVAR_POP(xd, ri), COVAR_SAMP(rf, xl) FROM t WHERE s < 800 GROUP BY g7, g20",
    "SELECT g7, g20, COVAR_SAMP(xl, rd), COUNT(*) FROM t WHERE c_inv1 IN (1, 5) GROUP BY g7, g20",   # an index-only filter, two keys
    "SELECT g7, COVAR_POP(xd, rd) FROM t WHERE s > 5000 GROUP BY g7",                                 # a filter matching nothing: no group
    "SELECT g2, COVAR_POP(g2, g7), COVAR_SAMP(g2, g2) FROM t GROUP BY g2",                            # a constant argument within every group
]


@pytest.mark.parametrize("n", [2049, 20011])
@pytest.mark.parametrize("sql", SHAPES)
def test_shapes(segments, n, sql):
    _check(segments(n), sql)


def test_filter_matching_nothing_without_group_by(segments):
    b = _check(segments(2049), "SELECT COVAR_POP(xd, ri), COVAR_SAMP(rl, xf) FROM t WHERE s > 5000", kernel="pg_covar_reg_wide")
    assert b.aggregation_result() == [(0.0, 0.0, 0.0, 0)] * 2
    assert all(np.copysign(1.0, v) == 1.0 for t in b.aggregation_result() for v in t[:3])
    assert [covariance_final(f, t) for f, t in zip(cm.FUNCTIONS, b.aggregation_result())] == [cm.NEG_INF] * 2


def test_num_groups_limit(segments):
    seg = segments(20011)
    plain = parse_sql("SELECT g7, g20, COUNT(*) FROM t WHERE s < 900 GROUP BY g7, g20")
    plain.num_groups_limit = 13
    admitted = {_norm(k) for k in seg[3].execute(plain).rows()}
    assert len(admitted) == 13
    b = _check(seg, "SELECT g7, g20, COVAR_POP(rd, xi), COUNT(*) FROM t WHERE s < 900 GROUP BY g7, g20", num_groups_limit=13, admitted=admitted)
    assert b.stats.num_groups_limit_reached == 1


def test_order_by_a_covariance_is_not_trimmed(segments):
    seg = segments(20011)
    sql = "SELECT g7, g20, COVAR_POP(xd, rf), COUNT(*) FROM t GROUP BY g7, g20 ORDER BY COVAR_POP(xd, rf) DESC LIMIT 1"
    qc = parse_sql(sql)
    qc.min_segment_group_trim_size = 1
    b = _check(seg, sql, qc=qc)
    assert len(b.rows()) == 140 and qc.limit == 1       # every group: trimming by a covariance is left to the broker, LIMIT travels unchanged
    qc = parse_sql("SELECT g7, g20, COVAR_POP(xd, rf), COUNT(*) FROM t GROUP BY g7, g20 ORDER BY COUNT(*) DESC LIMIT 1")
    qc.min_segment_group_trim_size = 1
    rows = seg[3].execute(qc).rows()
    assert len(rows) == 5                               # max(5 x limit, minSegmentGroupTrimSize), ordered by the remaining aggregation
    for key, (t, count) in rows.items():
        assert t[3] == count


def test_upsert_snapshot(gpu_api, oracle_api):
    host, data, schema = _data(20011, seed=9)
    g, o = NativeSegment(gpu_api, host), NativeSegment(oracle_api, host)
    keep = snapshot_doc_ids(host.total_docs)
    g.set_queryable_doc_ids(keep)
    o.set_queryable_doc_ids(keep)
    try:
        seg = (host, data, schema, g, o)
        b = _check(seg, "SELECT COVAR_POP(rd, xi), COVAR_SAMP(xf, rl) FROM t", kernel="pg_covar_reg_wide")
        assert b.stats.num_docs_scanned == len(keep)
        _check(seg, "SELECT COVAR_POP(rd, xi), COVAR_SAMP(rd, xi) FROM t WHERE s < 600", kernel="pg_covar_reg")
        _check(seg, "SELECT g7, COVAR_SAMP(rf, xd), COUNT(*) FROM t WHERE s < 600 GROUP BY g7", kernel="pg_covar_lds")
    finally:
        g.destroy()
        o.destroy()


def test_the_reference_query_of_eight_covariances_over_six_columns(segments):
    seg = segments(2049)
    sql = "SELECT " + ", ".join(f"COVAR_POP({x}, {y})" for x, y in REFERENCE_8) + " FROM t"
    b = _check(seg, sql, kernel="pg_covar_reg_wide")
    assert b.stats.num_entries_scanned_post_filter == 6 * seg[0].total_docs
    b = _check(seg, sql + " WHERE s < 500", kernel="pg_covar_reg_wide")
    assert b.stats.num_entries_scanned_post_filter == 6 * b.stats.num_docs_scanned
    _check(seg, "SELECT g7, " + sql[len("SELECT "):] + " GROUP BY g7", kernel="pg_covar_lds")


def test_two_functions_over_one_pair_share_slots_and_one_pass(segments):
    seg = segments(20011)
    two = _check(seg, "SELECT g7, COVAR_POP(rd, ri), COVAR_SAMP(rd, ri), COVAR_POP(rd, xd) FROM t WHERE s < 800 GROUP BY g7", kernel="pg_covar_lds")
    one = _check(seg, "SELECT g7, COVAR_SAMP(rd, ri), COVAR_POP(rd, xd) FROM t WHERE s < 800 GROUP BY g7", kernel="pg_covar_lds")
    # one pass, one set of slots per distinct column and per distinct pair: the pass reads the same bytes whatever the number of functions
    assert two.stats.algorithmic_bytes == one.stats.algorithmic_bytes and two.stats.percentile_passes == 0
    for key, (a, b, c) in two.rows().items():
        assert a == b == one.rows()[key][0] and c == one.rows()[key][1] and a[0] == c[0]   # the shared column's sum
    # the slot count decides the tier: G_FIT groups of one pair fit LDS with both functions over it as with one
    _check(seg, "SELECT kfit, COVAR_POP(rd, xd), COVAR_SAMP(rd, xd) FROM t GROUP BY kfit", kernel="pg_covar_lds")
    # the ordered pair is the unit: (y, x) is another pair, the same three sums with x and y exchanged
    b = _check(seg, "SELECT COVAR_POP(rd, xd), COVAR_POP(xd, rd) FROM t", kernel="pg_covar_reg_wide")   # two pairs: past the narrow register kernel
    (p, q), = b.rows().values()
    assert (p[0], p[1], p[2], p[3]) == (q[1], q[0], q[2], q[3])


def test_members_equal_the_sums_of_the_same_query(segments):
    """sumX, sumY, sumXY and count bit for bit what SUM(x), SUM(y), SUM(x * y) and COUNT(*) return next to the covariance (data inside both
    windows: every column's magnitudes span less than 2^10)"""
    seg = segments(20011)
    schema = seg[2]
    for x, y in (("rd", "xd"), ("xf", "rf"), ("xi", "xd"), ("rl", "xf"), ("xi", "ri")):
        for sql in (f"SELECT COVAR_POP({x}, {y}), SUM({x}), SUM({y}), SUM({x} * {y}), COUNT(*) FROM t WHERE s < 700",
                    f"SELECT g7, COVAR_SAMP({x}, {y}), SUM({x}), SUM({y}), SUM({x} * {y}), COUNT(*) FROM t GROUP BY g7"):
            b = _check(seg, sql)
            assert b.stats.kernel.decode().startswith("pg_expr_")   # the expression pass is the outer one
            for key, (t, sx, sy, sxy, count) in b.rows().items():
                assert cm.same_bits(t[1], sy) and cm.same_bits(t[2], sxy) and t[3] == count, (sql, key, t, sx, sy, sxy)
                # (SUM over a LONG column adds the longs themselves; the covariance adds them as getDoubleValuesSV reads them, rounded:
                # beyond 2^53 the two sums are sums of different values)
                assert schema[x] == "LONG" or cm.same_bits(t[0], sx), (sql, key, t, sx)


def test_next_to_variance_percentile_and_an_expression_aggregation(segments):
    """the frames nest: the expression pass outside, the covariance pass inside it, the variance's and the PERCENTILE's inside that"""
    seg = segments(20011)
    host, data, schema, gpu, oracle = seg
    sql = "SELECT g7, COVAR_POP(rd, xi), VAR_POP(rd), PERCENTILE(xi, 50), SUM(ri * xd), COUNT(*), COVAR_SAMP(xl, rf), MAX(s) FROM t WHERE s < 800 GROUP BY g7"
    b = _check(seg, sql)
    assert b.stats.kernel.decode().startswith("pg_expr_") and b.stats.percentile_passes == 1
    alone = gpu.execute("SELECT g7, VAR_POP(rd), PERCENTILE(xi, 50), SUM(ri * xd), MAX(s) FROM t WHERE s < 800 GROUP BY g7").rows()
    for key, v in b.rows().items():
        assert v[1] == alone[key][0] and pm.same_runs(v[2], alone[key][1]) and vm.same_bits(v[3], alone[key][2]) and v[6] == alone[key][3]
        assert vm.same_bits(v[0][0], v[1][1])   # sumX of the covariance is the variance tuple's sum
    b = _check(seg, "SELECT COVAR_SAMP(rf, xd), STDDEV_POP(rf), PERCENTILE(rd, 99), COUNT(*) FROM t")   # without the expression: the covariance pass is the outer one
    assert b.stats.kernel.decode() == "pg_covar_reg"
    b = _check(seg, "SELECT g7, LASTWITHTIME(xd, s, 'DOUBLE'), COVAR_POP(xd, rd) FROM t GROUP BY g7")     # inside the FIRSTWITHTIME / LASTWITHTIME pass
    assert b.stats.kernel.decode().startswith("pg_wt_")


def test_star_tree_route_is_not_taken(gpu_api):
    from tests.fixtures import synth_star_segment
    host = synth_star_segment(num_docs=20_000)
    seg = NativeSegment(gpu_api, host)
    try:
        plain = seg.execute("SELECT h1, COUNT(*), SUM(m) FROM gpuBench GROUP BY h1")
        assert plain.stats.star_tree_index >= 0
        b = seg.execute("SELECT h1, COUNT(*), SUM(m), COVAR_POP(m, m) FROM gpuBench GROUP BY h1")
        assert b.stats.star_tree_index == -1 and b.stats.num_docs_scanned == 20_000
        for key, (count, total, t) in b.rows().items():
            assert (count, total) == tuple(plain.rows()[key]) and t[3] == count and t[0] == total == t[1]
    finally:
        seg.destroy()


# ---- the data table -----------------------------------------------------------------------------------------------------------------------------------------
def test_data_table_bytes_and_names(segments, monkeypatch):
    """A covariance column is an OBJECT of ObjectSerDeUtils type 32 holding CovarianceTuple#toBytes: double sumX, double sumY, double sumXY,
    long count, big-endian; its name is getType().getName().toLowerCase() + "(" + x + "," + y + ")" """
    inner = dt.deserialize_object
    monkeypatch.setattr(dt, "deserialize_object", lambda kind, b: ("CovarianceTuple", bytes(b)) if kind == 32 else inner(kind, b))
    host, data, schema, gpu, oracle = segments(2049)
    sql = "SELECT g2, COUNT(*), COVAR_POP(rd, xi), COVAR_SAMP(  rf ,xl) FROM t WHERE s < 500 GROUP BY g2"
    r = gpu.execute_native(sql, keep_device_table=False)
    t = dt.parse_data_table_v4(r.data_table_v4())
    r.free()
    assert t["names"] == ["g2", "count(*)", "covarpop(rd,xi)", "covarsamp(rf,xl)"]
    assert t["types"] == ["INT", "LONG", "OBJECT", "OBJECT"] and len(t["rows"]) == 2
    docs, _ = _filter(oracle, sql)
    for row in t["rows"]:
        gdocs = docs[np.asarray(data["g2"])[docs] == row[0]]
        assert row[1] == len(gdocs)
        for cell, (x, y) in zip(row[2:], (("rd", "xi"), ("rf", "xl"))):
            want = cm.exact_tuple(_doubles(data, schema, x, gdocs), _doubles(data, schema, y, gdocs))
            assert cell == ("CovarianceTuple", cm.to_bytes(want)) and len(cell[1]) == 32, (row[0], x, y)
    r = gpu.execute_native("SELECT COVAR_POP(xd, ri) FROM t WHERE s > 5000", keep_device_table=False)
    t = dt.parse_data_table_v4(r.data_table_v4())
    r.free()
    assert t["names"] == ["covarpop(xd,ri)"] and [list(row) for row in t["rows"]] == [[("CovarianceTuple", cm.to_bytes((0.0, 0.0, 0.0, 0)))]]
    # blanks in the argument list as the C ABI may carry it do not reach the name
    qc = parse_sql("SELECT COVAR_POP(xd, ri) FROM t")
    qc.aggregations[0].column = " xd , ri "
    r = gpu.execute_native(qc, keep_device_table=False)
    assert dt.parse_data_table_v4(r.data_table_v4())["names"] == ["covarpop(xd,ri)"]
    r.free()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------------
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


def test_refusals(gpu_api):
    from pinot_amd.segment import build_mv_column
    host, data, schema = _data(2049, seed=3)
    rng = np.random.default_rng(1)
    n = host.total_docs
    host.columns["mv"] = build_mv_column("mv", [list(rng.integers(0, 20, rng.integers(1, 4))) for _ in range(n)], "INT")
    nulls = np.frombuffer(formats.serialize_roaring(np.array([3, 77, 2000], dtype=np.int64)), dtype=np.uint8)
    host.columns["xi"].null_vector = nulls
    host.columns["g20"].null_vector = nulls
    seg = NativeSegment(gpu_api, host)
    u = rng.uniform(1.0, 2.0, n)
    bad = {"dn": np.where(np.arange(n) == 5, np.nan, 1.5), "fi": np.where(np.arange(n) % 7 == 0, np.inf, 2.5).astype(np.float32), "g": np.zeros(n, dtype=np.int32),
           "b520": u * 2.0**520, "b500": u[::-1] * 2.0**500, "b490": -u * 2.0**490, "one": np.ones(n)}
    bad_schema = {"dn": "DOUBLE", "fi": "FLOAT", "g": "INT", "b520": "DOUBLE", "b500": "DOUBLE", "b490": "DOUBLE", "one": "DOUBLE"}
    bad_seg = NativeSegment(gpu_api, build_segment("covar_bad", bad, bad_schema, no_dictionary_columns=["dn", "b500"]))
    try:
        U = capi.PG_ERR_UNSUPPORTED
        for fn, name in (("COVAR_POP", "COVAR_POP"), ("covarsamp", "COVAR_SAMP")):
            _refused(gpu_api, seg, parse_sql(f"SELECT {fn}(txt, xd) FROM t"), U, f"{name} over the STRING column txt")
            _refused(gpu_api, seg, parse_sql(f"SELECT {fn}(xd, mv) FROM t"), U, f"{name} over the multi-value column mv")
            _refused(gpu_api, seg, parse_sql(f"SELECT g7, {fn}(ri * xd, xd) FROM t GROUP BY g7"), U, f"{name} over an expression")
            _refused(gpu_api, seg, parse_sql(f"SELECT {fn}(xd, nope) FROM t"), capi.PG_ERR_NOT_FOUND, "column not found: nope")
            for args, given in (("xd", 1), ("xd,ri,rd", 3)):
                qc = parse_sql(f"SELECT {fn}(xd, ri) FROM t")
                qc.aggregations[0].column = args
                _refused(gpu_api, seg, qc, capi.PG_ERR_INVALID_ARGUMENT, f"{name} takes 2 arguments (two columns), {given} given")
        _refused(gpu_api, seg, parse_sql("SELECT mv, COVAR_POP(xd, ri) FROM t GROUP BY mv"), U, "next to the multi-value group-by column mv")
        for pair, text in (("ri, xi", "COVAR_POP over xi, which holds nulls"), ("xd, ri", "grouped by g20, which holds nulls")):
            qc = parse_sql(f"SELECT g20, COVAR_POP({pair}) FROM t GROUP BY g20")
            qc.flags |= capi.QUERY_FLAG_NULL_HANDLING
            _refused(gpu_api, seg, qc, U, text)
        qc = parse_sql("SELECT g7, COVAR_SAMP(xd, ri), SUM(ri) FROM t GROUP BY g7")   # columns without nulls run under the flag
        qc.flags |= capi.QUERY_FLAG_NULL_HANDLING
        assert len(seg.execute(qc).rows()) == 7
        _refused(gpu_api, seg, parse_sql("SELECT u1, u2, u3, COVAR_POP(xd, ri) FROM t GROUP BY u1, u2, u3"), U, "group key space over 2^32")
        cols = ["xi", "xl", "xf", "xd", "ri", "rl", "rf", "rd", "s", "g7"]
        assert len(cols) == K["PG_COVAR_MAX_COLS"] + 2
        ten = ", ".join(f"COVAR_POP({cols[i]}, {cols[i + 1]})" for i in range(0, len(cols), 2))
        _refused(gpu_api, seg, parse_sql(f"SELECT {ten} FROM t"), U, "more than %d distinct columns" % K["PG_COVAR_MAX_COLS"])
        pairs = [(cols[0], c) for c in cols[1:8]] + [(cols[1], cols[2]), (cols[1], cols[3])]
        assert len(pairs) == K["PG_COVAR_MAX_PAIRS"] + 1 and len({c for p in pairs for c in p}) == 8
        _refused(gpu_api, seg, parse_sql("SELECT " + ", ".join(f"COVAR_POP({x}, {y})" for x, y in pairs) + " FROM t"), U, "more than %d distinct column pairs" % K["PG_COVAR_MAX_PAIRS"])
        _refused(gpu_api, bad_seg, parse_sql("SELECT COVAR_POP(one, dn) FROM t"), U, "COVAR_POP over dn, which holds a NaN or an infinity")
        _refused(gpu_api, bad_seg, parse_sql("SELECT g, COVAR_SAMP(fi, one) FROM t GROUP BY g"), U, "COVAR_SAMP over fi, which holds a NaN or an infinity")
        # the overflow bound from both sides: the bounds' exponents 528 + 512 reach 1024, 512 + 496 do not
        assert (cm.fx_exp_of(float(bad["b520"].max())), cm.fx_exp_of(float(bad["b500"].max())), cm.fx_exp_of(float(np.abs(bad["b490"]).max()))) == (528, 512, 496)
        _refused(gpu_api, bad_seg, parse_sql("SELECT COVAR_POP(b520, b500) FROM t"), U, "admit a product that overflows a double")
        (got,) = bad_seg.execute("SELECT COVAR_POP(b500, b490) FROM t").aggregation_result()
        xs, ys = [float(v) for v in bad["b500"]], [float(v) for v in bad["b490"]]
        assert cm.in_exact_window(xs, ys, "DOUBLE", "DOUBLE", K) and _same_tuple(got, cm.exact_tuple(xs, ys)) and np.isfinite(got[2])
        # a result carrying a covariance is merged on the Java side
        a = seg.execute_native("SELECT g7, COUNT(*), COVAR_POP(xd, ri) FROM t GROUP BY g7")
        b = seg.execute_native("SELECT g7, COUNT(*), COVAR_POP(xd, ri) FROM t GROUP BY g7")
        with pytest.raises(capi.NativeError) as e:
            a.merge(b)
        assert e.value.status == U and "CovarianceTuple#apply" in e.value.message
        # the third double exists for this kind only
        out = np.zeros(8)
        assert gpu_api.f("result_doubles")(a.handle, 1, 2, out.ctypes.data, 8) == capi.PG_OK
        assert gpu_api.f("result_doubles")(a.handle, 1, 3, out.ctypes.data, 8) == capi.PG_ERR_INVALID_ARGUMENT
        assert gpu_api.f("result_doubles")(a.handle, 0, 2, out.ctypes.data, 8) == capi.PG_ERR_INVALID_ARGUMENT   # COUNT(*)
        a.free()
        b.free()
    finally:
        seg.destroy()
        bad_seg.destroy()


def test_two_threads_on_one_segment(segments):
    seg = segments(20011)
    gpu = seg[3]
    sqls = ["SELECT g7, COVAR_POP(rd, xi), COVAR_SAMP(xi, rf) FROM t WHERE s < 700 GROUP BY g7", "SELECT kover, COVAR_SAMP(rf, xd) FROM t GROUP BY kover"]
    want = [gpu.execute(q).rows() for q in sqls]
    errors = []

    def work(i):
        try:
            for _ in range(5):
                assert gpu.execute(sqls[i]).rows() == want[i]
        except BaseException as e:   # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    _check(seg, sqls[0], kernel="pg_covar_lds")


# ---- the build ----------------------------------------------------------------------------------------------------------------------------------------------
def test_covariance_kernels_use_no_scratch():
    """the build leaves hipcc's kernel-resource-usage remarks of pg_kernels_covar.hip behind: no kernel of the path may spill"""
    log = os.path.join(ROOT, "pinot_amd", "csrc", "pg_kernels_covar.resources.log")
    usage, cur = {}, None
    for line in open(log):
        m = re.search(r"Function Name: (\w+)", line)
        if m:
            cur = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and cur:
            usage[cur] = int(m.group(1))
    for k in ("pg_covar_reg", "pg_covar_reg_wide", "pg_covar_lds", "pg_covar_hbm"):
        assert usage.get(k) == 0, (k, usage.get(k))
