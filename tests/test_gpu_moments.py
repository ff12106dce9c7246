"""SKEWNESS / KURTOSIS on the GPU path (PG_AGG_SKEWNESS / PG_AGG_KURTOSIS) against tests/fourth_moment_model.py over the ORACLE's match set
and group assignment: the tuple (n, m1, m2, m3, m4) bit for bit the Fraction model's on data inside the exact windows, the statistics from
the model and the oracle's filter.  The three kernel names of the path (pg_moment_reg / pg_moment_lds / pg_moment_hbm) are tied to the model
here, not to the oracle, which has no fourth moment."""
import math
import os
import re

import numpy as np
import pytest

from oracle import po_datatable as dt
from pinot_amd import capi, formats
from pinot_amd.executor import Comm, NativeSegment, kurtosis_final, skewness_final
from pinot_amd.query import CQuery, SqlError, parse_sql  # noqa: F401
from pinot_amd.segment import build_column, build_segment
from tests import covariance_model as cm
from tests import fourth_moment_model as fm
from tests import percentile_model as pm
from tests import variance_model as vm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = fm.header_constants()
LDS_SLOTS, DBL_SLOTS, INT_SLOTS, MAX_COLS = K["PG_MOMENT_LDS_SLOTS"], K["PG_M4_DBL_SLOTS"], K["PG_M4_INT_SLOTS"], K["PG_MOMENT_MAX_COLS"]
G_FIT = LDS_SLOTS // (1 + DBL_SLOTS)          # the last key space whose table of one DOUBLE column fits pg_moment_lds
DICT_COLS, RAW_COLS = ("xi", "xl", "xf", "xd"), ("ri", "rl", "rf", "rd")
SCHEMA_OF = {"xi": "INT", "ri": "INT", "xl": "LONG", "rl": "LONG", "xf": "FLOAT", "rf": "FLOAT", "xd": "DOUBLE", "rd": "DOUBLE"}
FINAL = {"SKEWNESS": skewness_final, "KURTOSIS": kurtosis_final}


def _data(n, seed=23):
    """exact-window data: the non-zero magnitudes of every FLOAT / DOUBLE column span less than 2^10"""
    rng = np.random.default_rng(seed + n)
    sign = lambda: np.where(rng.integers(0, 2, n) == 0, -1.0, 1.0)   # noqa: E731
    data = {
        "g7": rng.integers(0, 7, n).astype(np.int32), "g20": rng.integers(0, 20, n).astype(np.int32), "g2": (np.arange(n) % 2).astype(np.int32),
        "s": rng.integers(0, 1000, n).astype(np.int32), "c_inv1": rng.integers(0, 8, n).astype(np.int32),
        "kfit": (np.arange(n) % G_FIT).astype(np.int32), "kover": (np.arange(n) % (G_FIT + 1)).astype(np.int32),
        "xi": rng.integers(-5000, 5000, n).astype(np.int32) * 400_003, "ri": rng.integers(-2**31, 2**31 - 1, n, dtype=np.int64).astype(np.int32),
        "xl": rng.integers(-300, 300, n).astype(np.int64) * 10**15 + 1, "rl": rng.integers(-2**62, 2**62, n, dtype=np.int64),
        "xf": (rng.choice(rng.uniform(1.0, 1000.0, 97), n) * sign()).astype(np.float32), "rf": (rng.uniform(1.0, 1000.0, n) * sign()).astype(np.float32),
        "xd": rng.choice(rng.uniform(1e-3, 1.0, 211), n) * sign(), "rd": (1e9 + rng.standard_normal(n)),
        "u1": rng.permutation(n).astype(np.int32), "u2": rng.permutation(n).astype(np.int32), "u3": rng.permutation(n).astype(np.int32),
        "txt": np.array(["t%d" % v for v in rng.integers(0, 5, n)], dtype=object).tolist(),
    }
    data["ri"][0], data["rl"][0] = -2**31, 2**62 + 1      # the INT whose powers are largest; a LONG that is no double
    schema = {k: "INT" for k in data}
    schema.update(SCHEMA_OF)
    schema.update(txt="STRING")
    host = build_segment("m4_%d" % n, data, schema, inverted_index_columns=["c_inv1"], no_dictionary_columns=["ri", "rl", "rf", "rd"])
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


def _norm(key):
    return tuple(float(k) if isinstance(k, (int, float, np.integer, np.floating)) else k for k in key)


def _check(seg, sql, kernel=None, qc=None):
    """Runs `sql` on the GPU and holds every SKEWNESS / KURTOSIS and COUNT(*) of it, its groups and its statistics to the model."""
    host, data, schema, gpu, oracle = seg
    qc = qc or parse_sql(sql)
    docs, in_filter = _filter(oracle, sql)
    groups = pm.group_docs([np.asarray(data[g]) for g in qc.group_by], docs) if qc.group_by else {(): np.asarray(docs, dtype=np.int64)}
    groups = {_norm(k): v for k, v in groups.items()}
    b = gpu.execute(qc)
    rows = {_norm(k): v for k, v in b.rows().items()}
    assert set(rows) == set(groups), sql
    read = set(qc.group_by)
    for a in qc.aggregations:   # an expression's operand columns and a covariance's two arguments count once each
        read |= ({a.column} if a.column in data else set(re.findall(r"[A-Za-z_]\w*", a.column)) & set(data)) if a.column else set()
    assert (b.stats.num_docs_scanned, b.stats.num_entries_scanned_post_filter) == pm.statistics(len(docs), read), sql
    assert b.stats.num_entries_scanned_in_filter == in_filter and b.stats.stats_exact == 1 and b.stats.num_total_docs == host.total_docs, sql
    assert b.stats.star_tree_index == -1
    if kernel is not None:
        assert b.stats.kernel.decode() == kernel, sql
    for key, gdocs in groups.items():
        for a, spec in enumerate(qc.aggregations):
            if spec.function == "COUNT":
                assert rows[key][a] == len(gdocs), (sql, key)
            if spec.function not in fm.FUNCTIONS:
                continue
            want = fm.exact_tuple(fm.as_doubles(np.asarray(data[spec.column])[gdocs], schema[spec.column]))
            got = rows[key][a]
            assert fm.same_tuple(got, want), (sql, key, spec, got, want)
            if got[0] > 0:
                assert got[2] >= 0.0 and got[4] >= 0.0 and all(math.copysign(1.0, got[i]) == 1.0 for i in (2, 4)) and (got[3] != 0.0 or math.copysign(1.0, got[3]) == 1.0)
            final, model = FINAL[spec.function](got), fm.final(spec.function, want)
            assert (math.isnan(final) and math.isnan(model)) or final == pytest.approx(model, rel=1e-12), (sql, key, spec)
    return b


def _aggs(cols):
    return ", ".join(f"{('SKEWNESS', 'KURTOSIS')[i % 2]}({c})" for i, c in enumerate(cols))


# ---- the first case: fails on a tree without the feature with a SqlError --------------------------------------------------------------------------
def test_skewness_of_a_raw_int_column(segments):
    _check(segments(257), "SELECT SKEWNESS(ri) FROM t", kernel="pg_moment_reg")


# ---- doc counts, layouts, filters ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 4, 65, 255, 257, 2047, 2049])
def test_doc_counts_and_column_layouts(segments, n):
    """INT / LONG / FLOAT / DOUBLE arguments, dictionary-encoded and raw, MAX_COLS at a time; no filter, a scan filter and an index filter;
    without GROUP BY and with one column"""
    seg = segments(n)
    cols = DICT_COLS + RAW_COLS
    for i in range(0, len(cols), MAX_COLS):
        pair = cols[i:i + MAX_COLS]
        where = ("", " WHERE s < 500", " WHERE c_inv1 IN (1, 5)")[(i // MAX_COLS) % 3]
        for w in {"", where}:
            _check(seg, f"SELECT {_aggs(pair)}, COUNT(*) FROM t{w}", kernel="pg_moment_reg")
            _check(seg, f"SELECT g7, {_aggs(pair[::-1])} FROM t{w} GROUP BY g7", kernel="pg_moment_lds")


# ---- tiers ------------------------------------------------------------------------------------------------------------------------------------------------
def test_tier_boundary_and_the_hbm_budget(segments, gpu_knobs, gpu_api):
    assert (G_FIT * (1 + DBL_SLOTS) <= LDS_SLOTS < (G_FIT + 1) * (1 + DBL_SLOTS)) and G_FIT == 512
    seg = segments(2049)
    fit = "SELECT kfit, KURTOSIS(rd) FROM t WHERE s < 900 GROUP BY kfit"
    over = "SELECT kover, KURTOSIS(rd) FROM t WHERE s < 900 GROUP BY kover"
    _check(seg, fit, kernel="pg_moment_lds")         # the last table that fits the workgroup's LDS
    _check(seg, over, kernel="pg_moment_hbm")        # one group more
    _check(seg, "SELECT kover, SKEWNESS(ri), KURTOSIS(xd), COUNT(*) FROM t GROUP BY kover", kernel="pg_moment_hbm")   # both paths, no match words
    # the integer path's rows are shorter: more groups fit
    g_int = LDS_SLOTS // (1 + INT_SLOTS)
    assert g_int > 2 * G_FIT
    _check(seg, "SELECT kover, SKEWNESS(ri) FROM t GROUP BY kover", kernel="pg_moment_lds")
    table_bytes = (G_FIT + 1) * (1 + DBL_SLOTS) * 8
    gpu_knobs(PG_MOMENT_HBM_MAX_BYTES=table_bytes)
    _check(seg, over, kernel="pg_moment_hbm")        # exactly at the budget
    gpu_knobs(PG_MOMENT_HBM_MAX_BYTES=table_bytes - 1)
    _refused(gpu_api, seg[3], parse_sql(over), capi.PG_ERR_UNSUPPORTED, "more than PG_MOMENT_HBM_MAX_BYTES")
    _check(seg, fit, kernel="pg_moment_lds")         # the LDS tier does not ask the budget


# ---- the model's vectors through the kernels ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mean1e9_double", "mean1e9_int", "int_extremes", "long_2_62", "floats", "symmetric", "negative_skew", "at_2_200", "tiny_m4"])
def test_model_vectors(gpu_api, name):
    data_type, values = fm.VECTORS[name]
    n = len(values)
    dtype = {"INT": np.int32, "LONG": np.int64, "FLOAT": np.float32, "DOUBLE": np.float64}[data_type]
    data = {"x": np.array(values, dtype=dtype), "g": np.zeros(n, dtype=np.int32)}
    host = build_segment("m4v_" + name, data, {"x": data_type, "g": "INT"}, no_dictionary_columns=["x"])
    seg = NativeSegment(gpu_api, host)
    try:
        want = fm.exact_tuple(fm.as_doubles(values, data_type))
        for sql, kernel in (("SELECT KURTOSIS(x) FROM t", "pg_moment_reg"), ("SELECT g, SKEWNESS(x) FROM t GROUP BY g", "pg_moment_lds")):
            b = seg.execute(sql)
            assert b.stats.kernel.decode() == kernel
            (got,) = list(b.rows().values())[0]
            assert fm.same_tuple(got, want), (name, sql, got, want)
    finally:
        seg.destroy()


# ---- query shapes -----------------------------------------------------------------------------------------------------------------------------------------
def test_skewness_and_kurtosis_of_one_column_share_slots(segments):
    seg = segments(2049)
    both = _check(seg, "SELECT g7, SKEWNESS(rd), KURTOSIS(rd), KURTOSIS(ri), SKEWNESS(ri) FROM t WHERE s < 800 GROUP BY g7", kernel="pg_moment_lds")
    one = _check(seg, "SELECT g7, KURTOSIS(rd), SKEWNESS(ri) FROM t WHERE s < 800 GROUP BY g7", kernel="pg_moment_lds")
    # one pass, one set of slots per distinct column: the pass reads the same bytes whatever the number of functions over a column
    assert both.stats.algorithmic_bytes == one.stats.algorithmic_bytes
    for key, (a, b, c, d) in both.rows().items():
        assert fm.same_tuple(a, b) and fm.same_tuple(a, one.rows()[key][0]) and fm.same_tuple(c, d) and fm.same_tuple(c, one.rows()[key][1])
    # the slot count decides the tier: G_FIT groups of one DOUBLE column fit LDS with two functions over it as with one
    _check(seg, "SELECT kfit, SKEWNESS(rd), KURTOSIS(rd) FROM t GROUP BY kfit", kernel="pg_moment_lds")


def test_next_to_the_other_side_passes(segments):
    """the frames nest: the expression pass outside, then the covariance's, then this one, the variance's and the PERCENTILE's inside it"""
    seg = segments(2049)
    host, data, schema, gpu, oracle = seg
    sql = "SELECT g7, SKEWNESS(rd), VAR_POP(rd), COVAR_POP(xd, ri), PERCENTILE(xi, 50), SUM(ri * xd), COUNT(*), KURTOSIS(xl), MAX(s) FROM t WHERE s < 800 GROUP BY g7"
    b = _check(seg, sql)
    assert b.stats.kernel.decode().startswith("pg_expr_") and b.stats.percentile_passes == 1
    rows = b.rows()
    alone = gpu.execute("SELECT g7, VAR_POP(rd), COVAR_POP(xd, ri), PERCENTILE(xi, 50), SUM(ri * xd), MAX(s) FROM t WHERE s < 800 GROUP BY g7").rows()
    docs, _ = _filter(oracle, sql)
    for key, v in rows.items():
        gdocs = docs[np.asarray(data["g7"])[docs] == key[0]]
        assert v[1] == alone[key][0] == vm.exact_tuple(vm.as_doubles(np.asarray(data["rd"])[gdocs], "DOUBLE"))
        assert v[2] == alone[key][1] == cm.exact_tuple(cm.as_doubles(np.asarray(data["xd"])[gdocs], "DOUBLE"), cm.as_doubles(np.asarray(data["ri"])[gdocs], "INT"))
        assert pm.same_runs(v[3], alone[key][2]) and vm.same_bits(v[4], alone[key][3]) and v[7] == alone[key][4]
    b = _check(seg, "SELECT KURTOSIS(rf), VAR_POP(rf), PERCENTILE(rd, 99), COUNT(*) FROM t")   # without the outer passes this one is the outer one
    assert b.stats.kernel.decode() == "pg_moment_reg"


def test_order_by_a_skewness_is_not_trimmed(segments):
    seg = segments(2049)
    sql = "SELECT g7, g20, SKEWNESS(xd), COUNT(*) FROM t GROUP BY g7, g20 ORDER BY SKEWNESS(xd) DESC LIMIT 1"
    qc = parse_sql(sql)
    qc.min_segment_group_trim_size = 1
    b = _check(seg, sql, qc=qc)
    assert len(b.rows()) > 100 and qc.limit == 1        # every group: trimming by a skewness is left to the broker, LIMIT travels unchanged
    qc = parse_sql("SELECT g7, g20, SKEWNESS(xd), COUNT(*) FROM t GROUP BY g7, g20 ORDER BY COUNT(*) DESC LIMIT 1")
    qc.min_segment_group_trim_size = 1
    rows = seg[3].execute(qc).rows()
    assert len(rows) == 5                               # max(5 x limit, minSegmentGroupTrimSize), ordered by the remaining aggregation
    for key, (t, count) in rows.items():
        assert t[0] == count


def test_filter_matching_nothing(segments):
    seg = segments(2049)
    b = _check(seg, "SELECT SKEWNESS(xd), KURTOSIS(ri) FROM t WHERE s > 5000", kernel="pg_moment_reg")
    for t in b.aggregation_result():
        assert fm.same_tuple(t, (0, fm.NAN, fm.NAN, fm.NAN, fm.NAN))   # the reference's fresh PinotFourthMoment
        assert math.isnan(skewness_final(t)) and math.isnan(kurtosis_final(t))
    assert len(_check(seg, "SELECT g7, KURTOSIS(xd) FROM t WHERE s > 5000 GROUP BY g7").rows()) == 0   # with GROUP BY: no group


def test_star_tree_route_is_not_taken(gpu_api):
    from tests.fixtures import synth_star_segment
    host = synth_star_segment(num_docs=20_000)
    seg = NativeSegment(gpu_api, host)
    try:
        plain = seg.execute("SELECT h1, COUNT(*), SUM(m) FROM gpuBench GROUP BY h1")
        assert plain.stats.star_tree_index >= 0
        b = seg.execute("SELECT h1, COUNT(*), SUM(m), KURTOSIS(m) FROM gpuBench GROUP BY h1")
        assert b.stats.star_tree_index == -1 and b.stats.num_docs_scanned == 20_000
        for key, (count, total, t) in b.rows().items():
            assert (count, total) == tuple(plain.rows()[key]) and t[0] == count and t[1] == pytest.approx(total / count, rel=1e-15)
    finally:
        seg.destroy()


# ---- the data table -----------------------------------------------------------------------------------------------------------------------------------------
def test_data_table_bytes_and_names(segments, monkeypatch):
    """A column is an OBJECT of ObjectSerDeUtils type 34 holding PinotFourthMoment#serialize: long n, doubles m1 .. m4, big-endian; its name
    is getType().getName().toLowerCase() + "(" + column + ")" """
    inner = dt.deserialize_object
    monkeypatch.setattr(dt, "deserialize_object", lambda kind, b: ("PinotFourthMoment", bytes(b)) if kind == 34 else inner(kind, b))
    host, data, schema, gpu, oracle = segments(2049)
    sql = "SELECT g2, COUNT(*), SKEWNESS(rd), KURTOSIS(xi) FROM t WHERE s < 500 GROUP BY g2"
    r = gpu.execute_native(sql, keep_device_table=False)
    t = dt.parse_data_table_v4(r.data_table_v4())
    r.free()
    assert t["names"] == ["g2", "count(*)", "skewness(rd)", "kurtosis(xi)"]
    assert t["types"] == ["INT", "LONG", "OBJECT", "OBJECT"] and len(t["rows"]) == 2
    docs, _ = _filter(oracle, sql)
    for row in t["rows"]:
        gdocs = docs[np.asarray(data["g2"])[docs] == row[0]]
        assert row[1] == len(gdocs)
        for cell, col in zip(row[2:], ("rd", "xi")):
            want = fm.exact_tuple(fm.as_doubles(np.asarray(data[col])[gdocs], schema[col]))
            assert cell == ("PinotFourthMoment", fm.to_bytes(want)) and len(cell[1]) == 40, (row[0], col)
    r = gpu.execute_native("SELECT KURTOSIS(xd) FROM t WHERE s > 5000", keep_device_table=False)
    t = dt.parse_data_table_v4(r.data_table_v4())
    r.free()
    assert t["names"] == ["kurtosis(xd)"] and [list(row) for row in t["rows"]] == [[("PinotFourthMoment", fm.to_bytes((0, fm.NAN, fm.NAN, fm.NAN, fm.NAN)))]]


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
    host.columns["by"] = build_column("by", [b"ab%d" % (i % 5) for i in range(n)], "BYTES", dictionary=False)
    nulls = np.frombuffer(formats.serialize_roaring(np.array([3, 77, 2000], dtype=np.int64)), dtype=np.uint8)
    host.columns["xi"].null_vector = nulls
    host.columns["g20"].null_vector = nulls
    seg = NativeSegment(gpu_api, host)
    bad = {"dn": np.where(np.arange(n) == 5, np.nan, 1.5), "fi": np.where(np.arange(n) % 7 == 0, np.inf, 2.5).astype(np.float32),
           "big": np.where(np.arange(n) == 9, 2.0**300, 1.0), "edge": np.choose(np.arange(n) % 3, [2.0**239, -(2.0**238), 1.5 * 2.0**237]), "g": np.zeros(n, dtype=np.int32)}
    bad_seg = NativeSegment(gpu_api, build_segment("m4_bad", bad, {"dn": "DOUBLE", "fi": "FLOAT", "big": "DOUBLE", "edge": "DOUBLE", "g": "INT"}, no_dictionary_columns=["dn", "big"]))
    try:
        U = capi.PG_ERR_UNSUPPORTED
        for fn, name in (("SKEWNESS", "SKEWNESS"), ("kurtosis", "KURTOSIS")):
            _refused(gpu_api, seg, parse_sql(f"SELECT {fn}(txt) FROM t"), U, f"{name} over the STRING column txt")
            _refused(gpu_api, seg, parse_sql(f"SELECT g7, {fn}(by) FROM t GROUP BY g7"), U, f"{name} over the BYTES column by")
            _refused(gpu_api, seg, parse_sql(f"SELECT {fn}(mv) FROM t"), U, f"{name} over the multi-value column mv")
            _refused(gpu_api, seg, parse_sql(f"SELECT g7, {fn}(ri * xd) FROM t GROUP BY g7"), U, f"{name} over an expression")
            _refused(gpu_api, bad_seg, parse_sql(f"SELECT {fn}(dn) FROM t"), U, f"{name} over dn, which holds a NaN or an infinity")
            _refused(gpu_api, bad_seg, parse_sql(f"SELECT g, {fn}(fi) FROM t GROUP BY g"), U, f"{name} over fi, which holds a NaN or an infinity")
            _refused(gpu_api, bad_seg, parse_sql(f"SELECT {fn}(big) FROM t"), U, f"{name} over big: the column's bound 2^304 admits a fourth power that overflows a double")
        # 2^239 < 2^240 = 2^E, 4 E = 960: the largest bound that runs
        (t,) = bad_seg.execute("SELECT KURTOSIS(edge) FROM t").aggregation_result()
        assert fm.same_tuple(t, fm.exact_tuple([float(v) for v in bad["edge"]]))
        _refused(gpu_api, seg, parse_sql("SELECT mv, KURTOSIS(xd) FROM t GROUP BY mv"), U, "next to the multi-value group-by column mv")
        for col, text in (("xi", "SKEWNESS over xi, which holds nulls"), ("xd", "grouped by g20, which holds nulls")):
            qc = parse_sql(f"SELECT g20, SKEWNESS({col}) FROM t GROUP BY g20")
            qc.flags |= capi.QUERY_FLAG_NULL_HANDLING
            _refused(gpu_api, seg, qc, U, text)
        qc = parse_sql("SELECT g7, KURTOSIS(xd), SUM(ri) FROM t GROUP BY g7")   # columns without nulls run under the flag
        qc.flags |= capi.QUERY_FLAG_NULL_HANDLING
        assert len(seg.execute(qc).rows()) == 7
        _refused(gpu_api, seg, parse_sql("SELECT u1, u2, u3, SKEWNESS(xd) FROM t GROUP BY u1, u2, u3"), U, "group key space over 2^32")
        cols = ", ".join(f"SKEWNESS({c})" for c in (DICT_COLS + RAW_COLS)[:MAX_COLS + 1])
        _refused(gpu_api, seg, parse_sql(f"SELECT {cols} FROM t"), U, f"more than {MAX_COLS} distinct columns")
        # a result carrying one is merged on the Java side
        a = seg.execute_native("SELECT g7, COUNT(*), SKEWNESS(xd) FROM t GROUP BY g7")
        b = seg.execute_native("SELECT g7, COUNT(*), SKEWNESS(xd) FROM t GROUP BY g7")
        with pytest.raises(capi.NativeError) as e:
            a.merge(b)
        assert e.value.status == U and "PinotFourthMoment#combine" in e.value.message
        # ... also across devices: the refusal comes before any communication (a world of one rank)
        comm = Comm.init_rank(gpu_api, 0, 1, 0, Comm.unique_id(gpu_api))
        with pytest.raises(capi.NativeError) as e:
            a.all_reduce(comm)
        assert e.value.status == U and "PinotFourthMoment#combine" in e.value.message
        comm.destroy()
        a.free()
        b.free()
    finally:
        seg.destroy()
        bad_seg.destroy()


# ---- the build ----------------------------------------------------------------------------------------------------------------------------------------------
def test_moment_kernels_use_no_scratch():
    """the build leaves hipcc's kernel-resource-usage remarks of pg_kernels_moment.hip behind: no kernel of the path may spill"""
    log = os.path.join(ROOT, "pinot_amd", "csrc", "pg_kernels_moment.resources.log")
    assert os.path.exists(log), "the build writes the resource log next to the library"
    usage, cur = {}, None
    for line in open(log):
        m = re.search(r"Function Name: (\w+)", line)
        if m:
            cur = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and cur:
            usage[cur] = int(m.group(1))
    for k in ("pg_moment_reg", "pg_moment_lds", "pg_moment_hbm"):
        assert usage.get(k) == 0, (k, usage.get(k))
