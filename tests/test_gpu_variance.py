"""VAR_POP / VAR_SAMP / STDDEV_POP / STDDEV_SAMP on the GPU path (PG_AGG_VARPOP .. PG_AGG_STDDEVSAMP) against tests/variance_model.py over the
ORACLE's match set and group assignment: the tuple (count, sum, m2) bit for bit the Fraction model's on data inside the exact window, never
further from the truth than the reference's docId-order arithmetic on the ill-conditioned columns, the statistics from the model and the
oracle's filter.  The three kernel names of the path (pg_var_reg / pg_var_lds / pg_var_hbm) are tied to the model here, not to the oracle,
which has no variance."""
import os
import re
import threading
from fractions import Fraction

import numpy as np
import pytest

from oracle import po_datatable as dt
from pinot_amd import capi, formats
from pinot_amd.executor import CancelToken, NativeSegment, variance_final
from pinot_amd.query import CQuery, parse_sql
from pinot_amd.segment import build_segment
from tests import percentile_model as pm
from tests import time_transform_model as tm
from tests import variance_model as vm
from tests.kernel_inventory import snapshot_doc_ids

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = vm.header_constants()
LDS_SLOTS = int(re.search(r"#define PG_VAR_LDS_SLOTS (\d+)", open(os.path.join(ROOT, "pinot_amd", "csrc", "pg_device.h")).read()).group(1))
DBL_SLOTS = K["PG_VAR_SUM_LIMBS"] + K["PG_VAR_SQ_LIMBS"]
G_FIT = LDS_SLOTS // (1 + DBL_SLOTS)          # the last key space whose table of one DOUBLE column fits pg_var_lds
DICT_COLS, RAW_COLS = ("xi", "xl", "xf", "xd"), ("ri", "rl", "rf", "rd")
SCHEMA_OF = {"xi": "INT", "ri": "INT", "xl": "LONG", "rl": "LONG", "xf": "FLOAT", "rf": "FLOAT", "xd": "DOUBLE", "rd": "DOUBLE"}
DAY_MS = 86_400_000


def _data(n, seed=17):
    """exact-window data: the non-zero magnitudes of every FLOAT / DOUBLE column span less than 2^10"""
    rng = np.random.default_rng(seed + n)
    sign = lambda: np.where(rng.integers(0, 2, n) == 0, -1.0, 1.0)   # noqa: E731
    data = {
        "g7": rng.integers(0, 7, n).astype(np.int32), "g20": rng.integers(0, 20, n).astype(np.int32), "g3": rng.integers(0, 3, n).astype(np.int32),
        "g2": (np.arange(n) % 2).astype(np.int32), "rg": (rng.integers(0, 50, n) * 1000 - 7).astype(np.int32),
        "ts": rng.integers(-3 * DAY_MS, 4 * DAY_MS, n).astype(np.int64),
        "s": rng.integers(0, 1000, n).astype(np.int32), "c_inv1": rng.integers(0, 8, n).astype(np.int32),
        "kfit": (np.arange(n) % G_FIT).astype(np.int32), "kover": (np.arange(n) % (G_FIT + 1)).astype(np.int32),
        "xi": rng.integers(-5000, 5000, n).astype(np.int32) * 400_003, "ri": rng.integers(-2**31, 2**31 - 1, n, dtype=np.int64).astype(np.int32),
        "xl": rng.integers(-300, 300, n).astype(np.int64) * 10**15 + 1, "rl": rng.integers(-2**62, 2**62, n, dtype=np.int64),
        "xf": (rng.choice(rng.uniform(1.0, 1000.0, 97), n) * sign()).astype(np.float32), "rf": (rng.uniform(1.0, 1000.0, n) * sign()).astype(np.float32),
        "xd": rng.choice(rng.uniform(1e-3, 1.0, 211), n) * sign(), "rd": (1e9 + rng.standard_normal(n)),
        "u1": rng.permutation(n).astype(np.int32), "u2": rng.permutation(n).astype(np.int32), "u3": rng.permutation(n).astype(np.int32),
        "y1": rng.integers(0, 9, n).astype(np.int32), "txt": np.array(["t%d" % v for v in rng.integers(0, 5, n)], dtype=object).tolist(),
    }
    data["rl"][rng.integers(0, n, 3)] = 2**62 + 1      # LONGs that are no doubles
    schema = {k: "INT" for k in data}
    schema.update(SCHEMA_OF)
    schema.update(ts="LONG", txt="STRING")
    host = build_segment("var_%d" % n, data, schema, inverted_index_columns=["c_inv1"], no_dictionary_columns=["rg", "ts", "ri", "rl", "rf", "rd"])
    return host, data, schema


_SEGMENTS = {}


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


def _key_column(text, data):
    """the values of a group-by key over all docs: a column, rg / 1000 (one IEEE division), or a time-bucket transform (tests/time_transform_model.py)"""
    if text in data:
        return np.asarray(data[text])
    if text.startswith("divide("):
        return np.asarray(data["rg"], dtype=np.float64) / 1000.0
    return np.array(tm.evaluate(text, data[tm.columns_of(text)[0]]), dtype=np.int64)


def _norm(key):
    return tuple(float(k) if isinstance(k, (int, float, np.integer, np.floating)) else k for k in key)


def _same_tuple(got, want):
    return got[0] == want[0] and vm.same_bits(got[1], want[1]) and vm.same_bits(got[2], want[2])


def _check(seg, sql, kernel=None, num_groups_limit=0, admitted=None, qc=None):
    """Runs `sql` on the GPU and holds every variance aggregation and COUNT(*) of it, its groups and its statistics to the model."""
    host, data, schema, gpu, oracle = seg
    qc = qc or parse_sql(sql)
    qc.num_groups_limit = num_groups_limit
    docs, in_filter = _filter(oracle, sql)
    groups = pm.group_docs([_key_column(g, data) for g in qc.group_by], docs) if qc.group_by else {(): np.asarray(docs, dtype=np.int64)}
    groups = {_norm(k): v for k, v in groups.items()}
    if admitted is not None:
        groups = {k: v for k, v in groups.items() if k in admitted}
    b = gpu.execute(qc)
    rows = {_norm(k): v for k, v in b.rows().items()}
    assert set(rows) == set(groups), sql
    read = set()
    for a in qc.aggregations:   # an expression's operand columns count once each
        read |= ({a.column} if a.column in data else set(re.findall(r"[A-Za-z_]\w*", a.column)) & set(data)) if a.column else set()
    for g in qc.group_by:
        read |= {g} if g in data else ({"rg"} if g.startswith("divide(") else {tm.columns_of(g)[0]})
    assert (b.stats.num_docs_scanned, b.stats.num_entries_scanned_post_filter) == pm.statistics(len(docs), read), sql
    assert b.stats.num_entries_scanned_in_filter == in_filter and b.stats.stats_exact == 1 and b.stats.num_total_docs == host.total_docs, sql
    assert b.stats.star_tree_index == -1
    if kernel is not None:
        assert b.stats.kernel.decode() == kernel, sql
    for key, gdocs in groups.items():
        for a, spec in enumerate(qc.aggregations):
            if spec.function == "COUNT":
                assert rows[key][a] == len(gdocs), (sql, key)
            if spec.function not in vm.FUNCTIONS:
                continue
            d = vm.as_doubles(np.asarray(data[spec.column])[gdocs], schema[spec.column])
            want = vm.exact_tuple(d)
            assert _same_tuple(rows[key][a], want), (sql, key, spec, rows[key][a], want)
            assert rows[key][a][2] >= 0.0 and np.copysign(1.0, rows[key][a][2]) == 1.0
            assert vm.same_bits(variance_final(spec.function, rows[key][a]), vm.final(spec.function, want)), (sql, key, spec)
    return b


def _aggs(cols):
    fns = ("VAR_POP", "VAR_SAMP", "STDDEV_POP", "STDDEV_SAMP")
    return ", ".join(f"{fns[i % 4]}({c})" for i, c in enumerate(cols))


# ---- doc counts and layouts ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049])
def test_doc_counts_and_column_layouts(segments, n):
    """INT / LONG / FLOAT / DOUBLE arguments, dictionary-encoded and raw, with and without a filter, without GROUP BY and with one column"""
    seg = segments(n)
    for cols in (DICT_COLS, RAW_COLS):
        for where in ("", " WHERE s < 500"):
            _check(seg, f"SELECT {_aggs(cols)}, COUNT(*) FROM t{where}", kernel="pg_var_reg")
            _check(seg, f"SELECT g7, {_aggs(cols)} FROM t{where} GROUP BY g7", kernel="pg_var_lds")


# ---- tiers ------------------------------------------------------------------------------------------------------------------------------------------------
def test_tier_boundary_and_the_hbm_budget(segments, gpu_knobs, gpu_api):
    assert (G_FIT * (1 + DBL_SLOTS) <= LDS_SLOTS < (G_FIT + 1) * (1 + DBL_SLOTS)) and G_FIT > 1000
    seg = segments(20011)
    fit = "SELECT kfit, STDDEV_POP(rd) FROM t WHERE s < 900 GROUP BY kfit"
    over = "SELECT kover, STDDEV_POP(rd) FROM t WHERE s < 900 GROUP BY kover"
    _check(seg, fit, kernel="pg_var_lds")         # the last table that fits the workgroup's LDS
    _check(seg, over, kernel="pg_var_hbm")        # one group more
    _check(seg, "SELECT kover, VAR_SAMP(ri), VAR_POP(xd), COUNT(*) FROM t GROUP BY kover", kernel="pg_var_hbm")   # both paths, no match words
    table_bytes = (G_FIT + 1) * (1 + DBL_SLOTS) * 8
    gpu_knobs(PG_VAR_HBM_MAX_BYTES=table_bytes)
    _check(seg, over, kernel="pg_var_hbm")        # exactly at the budget
    gpu_knobs(PG_VAR_HBM_MAX_BYTES=table_bytes - 1)
    _refused(gpu_api, seg[3], parse_sql(over), capi.PG_ERR_UNSUPPORTED, "more than PG_VAR_HBM_MAX_BYTES")
    _check(seg, fit, kernel="pg_var_lds")         # the LDS tier does not ask the budget


# ---- against the reference's drift ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", vm.ILL_CONDITIONED)
def test_never_further_from_the_truth_than_the_reference(gpu_api, name):
    """|gpu - exact| <= |reference restated - exact| for m2 and for sum, without a tolerance: ours is the correctly rounded value (these columns
    lie inside the exact window: tests/test_moments_host.py); tests/test_variance_model.py shows the restatement finite and off on them"""
    data_type, values = vm.VECTORS[name]
    n = len(values)
    dtype = {"INT": np.int32, "LONG": np.int64, "FLOAT": np.float32, "DOUBLE": np.float64}[data_type]
    data = {"x": np.array(values, dtype=dtype), "g": np.zeros(n, dtype=np.int32)}
    host = build_segment("ill_" + name, data, {"x": data_type, "g": "INT"}, no_dictionary_columns=["x"])
    seg = NativeSegment(gpu_api, host)
    try:
        d = vm.as_doubles(values, data_type)
        _, sx, m2 = vm.exact_moments(d)
        for sql, grouped, kernel in (("SELECT VAR_POP(x) FROM t", False, "pg_var_reg"), ("SELECT g, VAR_POP(x) FROM t GROUP BY g", True, "pg_var_lds")):
            b = seg.execute(sql)
            assert b.stats.kernel.decode() == kernel
            (got,) = list(b.rows().values())[0]
            ref = vm.reference_tuple(d, grouped)
            print(name, grouped, "gpu", got, "reference", ref, "exact m2", float(m2))
            assert got[0] == n == ref[0]
            assert abs(Fraction(got[2]) - m2) <= abs(Fraction(ref[2]) - m2)
            assert abs(Fraction(got[1]) - sx) <= abs(Fraction(ref[1]) - sx)
            assert _same_tuple(got, vm.exact_tuple(d))
    finally:
        seg.destroy()


# ---- query shapes -----------------------------------------------------------------------------------------------------------------------------------------
SHAPES = [
    "SELECT g7, g20, VAR_POP(xd), STDDEV_SAMP(ri) FROM t WHERE s < 800 GROUP BY g7, g20",
    "SELECT g7, g20, g3, VAR_SAMP(xl), COUNT(*) FROM t WHERE c_inv1 IN (1, 5) GROUP BY g7, g20, g3",     # an index-only filter, three keys (420 groups x 11 slots: LDS)
    "SELECT rg, STDDEV_POP(rf), VAR_POP(xi) FROM t WHERE s BETWEEN 100 AND 700 GROUP BY rg",              # a raw group key: its virtual dictionary
    "SELECT rg / 1000, VAR_POP(rd), COUNT(*) FROM t WHERE s < 900 GROUP BY rg / 1000",                    # an expression key
    "SELECT toEpochDays(ts), g3, STDDEV_SAMP(xf), VAR_POP(rl) FROM t GROUP BY toEpochDays(ts), g3",       # a time-bucket key
    "SELECT g7, VAR_POP(xd) FROM t WHERE s > 5000 GROUP BY g7",                                           # a filter matching nothing: no group
    "SELECT g2, VAR_POP(g2), VAR_SAMP(g2), STDDEV_POP(g7) FROM t GROUP BY g2",                            # every value of a group equal: m2 exactly 0.0
]


@pytest.mark.parametrize("n", [2049, 20011])
@pytest.mark.parametrize("sql", SHAPES)
def test_shapes(segments, n, sql):
    _check(segments(n), sql)


def test_filter_matching_nothing_without_group_by(segments):
    b = _check(segments(2049), "SELECT VAR_POP(xd), VAR_SAMP(ri), STDDEV_POP(rl), STDDEV_SAMP(xf) FROM t WHERE s > 5000", kernel="pg_var_reg")
    assert b.aggregation_result() == [(0, 0.0, 0.0)] * 4
    assert [variance_final(f, t) for f, t in zip(vm.FUNCTIONS, b.aggregation_result())] == [vm.NEG_INF] * 4


def test_num_groups_limit(segments):
    seg = segments(20011)
    plain = parse_sql("SELECT g7, g20, COUNT(*) FROM t WHERE s < 900 GROUP BY g7, g20")
    plain.num_groups_limit = 13
    admitted = {_norm(k) for k in seg[3].execute(plain).rows()}
    assert len(admitted) == 13
    b = _check(seg, "SELECT g7, g20, STDDEV_POP(rd), COUNT(*) FROM t WHERE s < 900 GROUP BY g7, g20", num_groups_limit=13, admitted=admitted)
    assert b.stats.num_groups_limit_reached == 1


def test_order_by_a_variance_is_not_trimmed(segments):
    seg = segments(20011)
    sql = "SELECT g7, g20, VAR_POP(xd), COUNT(*) FROM t GROUP BY g7, g20 ORDER BY VAR_POP(xd) DESC LIMIT 1"
    qc = parse_sql(sql)
    qc.min_segment_group_trim_size = 1
    b = _check(seg, sql, qc=qc)
    assert len(b.rows()) == 140 and qc.limit == 1       # every group: trimming by a variance is left to the broker, LIMIT travels unchanged
    qc = parse_sql("SELECT g7, g20, VAR_POP(xd), COUNT(*) FROM t GROUP BY g7, g20 ORDER BY COUNT(*) DESC LIMIT 1")
    qc.min_segment_group_trim_size = 1
    rows = seg[3].execute(qc).rows()
    assert len(rows) == 5                               # max(5 x limit, minSegmentGroupTrimSize), ordered by the remaining aggregation
    for key, (t, count) in rows.items():
        assert t[0] == count


def test_upsert_snapshot(gpu_api, oracle_api):
    host, data, schema = _data(20011, seed=9)
    g, o = NativeSegment(gpu_api, host), NativeSegment(oracle_api, host)
    keep = snapshot_doc_ids(host.total_docs)
    g.set_queryable_doc_ids(keep)
    o.set_queryable_doc_ids(keep)
    try:
        seg = (host, data, schema, g, o)
        b = _check(seg, "SELECT VAR_POP(rd), STDDEV_SAMP(xi) FROM t", kernel="pg_var_reg")
        assert b.stats.num_docs_scanned == len(keep)
        _check(seg, "SELECT g7, VAR_SAMP(rf), COUNT(*) FROM t WHERE s < 600 GROUP BY g7", kernel="pg_var_lds")
    finally:
        g.destroy()
        o.destroy()


def test_four_functions_over_two_columns_share_slots_and_one_pass(segments):
    seg = segments(20011)
    four = _check(seg, "SELECT g7, VAR_POP(rd), VAR_SAMP(rd), STDDEV_POP(ri), STDDEV_SAMP(ri) FROM t WHERE s < 800 GROUP BY g7", kernel="pg_var_lds")
    two = _check(seg, "SELECT g7, VAR_POP(rd), STDDEV_POP(ri) FROM t WHERE s < 800 GROUP BY g7", kernel="pg_var_lds")
    # one pass, one set of slots per distinct column: the pass reads the same bytes whatever the number of functions over a column
    assert four.stats.algorithmic_bytes == two.stats.algorithmic_bytes and four.stats.percentile_passes == 0
    for key, (a, b, c, d) in four.rows().items():
        assert a == b == two.rows()[key][0] and c == d == two.rows()[key][1]
    # the slot count decides the tier: G_FIT groups of one DOUBLE column fit LDS with four functions over it as with one
    _check(seg, f"SELECT kfit, {_aggs(['rd'] * 4)} FROM t GROUP BY kfit", kernel="pg_var_lds")


def test_next_to_percentile_and_an_expression_aggregation(segments):
    """the frames nest: the expression pass outside, the variance pass inside it, the PERCENTILE's inside that"""
    seg = segments(20011)
    host, data, schema, gpu, oracle = seg
    sql = "SELECT g7, VAR_POP(rd), PERCENTILE(xi, 50), SUM(ri * xd), COUNT(*), STDDEV_SAMP(xl), MAX(s) FROM t WHERE s < 800 GROUP BY g7"
    b = _check(seg, sql)
    assert b.stats.kernel.decode().startswith("pg_expr_") and b.stats.percentile_passes == 1
    rows = b.rows()
    alone = gpu.execute("SELECT g7, PERCENTILE(xi, 50), SUM(ri * xd), MAX(s) FROM t WHERE s < 800 GROUP BY g7").rows()
    for key, v in rows.items():
        assert pm.same_runs(v[1], alone[key][0]) and vm.same_bits(v[2], alone[key][1]) and v[5] == alone[key][2]
    b = _check(seg, "SELECT STDDEV_POP(rf), PERCENTILE(rd, 99), COUNT(*) FROM t")   # without the expression: the variance pass is the outer one
    assert b.stats.kernel.decode() == "pg_var_reg"


def test_star_tree_route_is_not_taken(gpu_api):
    from tests.fixtures import synth_star_segment
    host = synth_star_segment(num_docs=20_000)
    seg = NativeSegment(gpu_api, host)
    try:
        plain = seg.execute("SELECT h1, COUNT(*), SUM(m) FROM gpuBench GROUP BY h1")
        assert plain.stats.star_tree_index >= 0
        b = seg.execute("SELECT h1, COUNT(*), SUM(m), VAR_POP(m) FROM gpuBench GROUP BY h1")
        assert b.stats.star_tree_index == -1 and b.stats.num_docs_scanned == 20_000
        for key, (count, total, t) in b.rows().items():
            assert (count, total) == tuple(plain.rows()[key]) and t[0] == count and t[1] == total
    finally:
        seg.destroy()


# ---- the data table -----------------------------------------------------------------------------------------------------------------------------------------
def test_data_table_bytes_and_names(segments, monkeypatch):
    """A variance column is an OBJECT of ObjectSerDeUtils type 33 holding VarianceTuple#toBytes: long count, double sum, double m2, big-endian;
    its name is getType().getName().toLowerCase() + "(" + column + ")" """
    inner = dt.deserialize_object
    monkeypatch.setattr(dt, "deserialize_object", lambda kind, b: ("VarianceTuple", bytes(b)) if kind == 33 else inner(kind, b))
    host, data, schema, gpu, oracle = segments(2049)
    sql = "SELECT g2, COUNT(*), VAR_POP(rd), VAR_SAMP(xi), STDDEV_POP(rf), STDDEV_SAMP(xl) FROM t WHERE s < 500 GROUP BY g2"
    r = gpu.execute_native(sql, keep_device_table=False)
    t = dt.parse_data_table_v4(r.data_table_v4())
    r.free()
    assert t["names"] == ["g2", "count(*)", "varpop(rd)", "varsamp(xi)", "stddevpop(rf)", "stddevsamp(xl)"]
    assert t["types"] == ["INT", "LONG", "OBJECT", "OBJECT", "OBJECT", "OBJECT"] and len(t["rows"]) == 2
    docs, _ = _filter(oracle, sql)
    for row in t["rows"]:
        gdocs = docs[np.asarray(data["g2"])[docs] == row[0]]
        assert row[1] == len(gdocs)
        for cell, col in zip(row[2:], ("rd", "xi", "rf", "xl")):
            want = vm.exact_tuple(vm.as_doubles(np.asarray(data[col])[gdocs], schema[col]))
            assert cell == ("VarianceTuple", vm.to_bytes(want)) and len(cell[1]) == 24, (row[0], col)
    r = gpu.execute_native("SELECT VAR_POP(xd) FROM t WHERE s > 5000", keep_device_table=False)
    t = dt.parse_data_table_v4(r.data_table_v4())
    r.free()
    assert t["names"] == ["varpop(xd)"] and [list(row) for row in t["rows"]] == [[("VarianceTuple", vm.to_bytes((0, 0.0, 0.0)))]]


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
    bad = {"dn": np.where(np.arange(n) == 5, np.nan, 1.5), "fi": np.where(np.arange(n) % 7 == 0, np.inf, 2.5).astype(np.float32), "g": np.zeros(n, dtype=np.int32)}
    bad_seg = NativeSegment(gpu_api, build_segment("var_bad", bad, {"dn": "DOUBLE", "fi": "FLOAT", "g": "INT"}, no_dictionary_columns=["dn"]))
    try:
        U = capi.PG_ERR_UNSUPPORTED
        for fn, name in (("VAR_POP", "VAR_POP"), ("VARSAMP", "VAR_SAMP"), ("stddev_pop", "STDDEV_POP"), ("STDDEV_SAMP", "STDDEV_SAMP")):
            _refused(gpu_api, seg, parse_sql(f"SELECT {fn}(txt) FROM t"), U, f"{name} over the STRING column txt")
            _refused(gpu_api, seg, parse_sql(f"SELECT {fn}(mv) FROM t"), U, f"{name} over the multi-value column mv")
            _refused(gpu_api, seg, parse_sql(f"SELECT g7, {fn}(ri * xd) FROM t GROUP BY g7"), U, f"{name} over an expression")
        _refused(gpu_api, seg, parse_sql("SELECT mv, VAR_POP(xd) FROM t GROUP BY mv"), U, "next to the multi-value group-by column mv")
        for col, text in (("xi", "VAR_POP over xi, which holds nulls"), ("xd", "grouped by g20, which holds nulls")):
            qc = parse_sql(f"SELECT g20, VAR_POP({col}) FROM t GROUP BY g20")
            qc.flags |= capi.QUERY_FLAG_NULL_HANDLING
            _refused(gpu_api, seg, qc, U, text)
        qc = parse_sql("SELECT g7, STDDEV_POP(xd), SUM(ri) FROM t GROUP BY g7")   # columns without nulls run under the flag
        qc.flags |= capi.QUERY_FLAG_NULL_HANDLING
        assert len(seg.execute(qc).rows()) == 7
        _refused(gpu_api, seg, parse_sql("SELECT u1, u2, u3, VAR_POP(xd) FROM t GROUP BY u1, u2, u3"), U, "group key space over 2^32")
        _refused(gpu_api, seg, parse_sql("SELECT VAR_POP(xd), VAR_POP(ri), VAR_POP(rl), VAR_POP(xf), VAR_POP(rd) FROM t"), U, "more than 4 distinct columns")
        _refused(gpu_api, bad_seg, parse_sql("SELECT VAR_POP(dn) FROM t"), U, "VAR_POP over dn, which holds a NaN or an infinity")
        _refused(gpu_api, bad_seg, parse_sql("SELECT g, STDDEV_SAMP(fi) FROM t GROUP BY g"), U, "STDDEV_SAMP over fi, which holds a NaN or an infinity")
        # a result carrying a variance is merged on the Java side
        a = seg.execute_native("SELECT g7, COUNT(*), VAR_POP(xd) FROM t GROUP BY g7")
        b = seg.execute_native("SELECT g7, COUNT(*), VAR_POP(xd) FROM t GROUP BY g7")
        with pytest.raises(capi.NativeError) as e:
            a.merge(b)
        assert e.value.status == U and "VarianceTuple#apply" in e.value.message
        a.free()
        b.free()
        # cancellation: the token is polled before the ordinary part is planned
        token = CancelToken(gpu_api)
        token.request()
        with pytest.raises(capi.NativeError) as e:
            seg.execute_native("SELECT g7, VAR_POP(xd) FROM t GROUP BY g7", cancel=token)
        assert e.value.status == capi.PG_ERR_CANCELLED
        token.reset()
        r = seg.execute_native("SELECT g7, VAR_POP(xd) FROM t GROUP BY g7", cancel=token)
        assert len(r.block().rows()) == 7
        r.free()
        token.destroy()
    finally:
        seg.destroy()
        bad_seg.destroy()


def test_two_threads_on_one_segment(segments):
    seg = segments(20011)
    gpu = seg[3]
    sqls = ["SELECT g7, VAR_POP(rd), STDDEV_SAMP(xi) FROM t WHERE s < 700 GROUP BY g7", "SELECT kover, VAR_SAMP(rf) FROM t GROUP BY kover"]
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
    _check(seg, sqls[0], kernel="pg_var_lds")


# ---- the build ----------------------------------------------------------------------------------------------------------------------------------------------
def test_variance_kernels_use_no_scratch():
    """the build leaves hipcc's kernel-resource-usage remarks of pg_kernels_var.hip behind: no kernel of the path may spill"""
    log = os.path.join(ROOT, "pinot_amd", "csrc", "pg_kernels_var.resources.log")
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
    for k in ("pg_var_reg", "pg_var_lds", "pg_var_hbm"):
        assert usage.get(k) == 0, (k, usage.get(k))
