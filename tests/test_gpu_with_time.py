"""FIRSTWITHTIME / LASTWITHTIME on the GPU path (PG_AGG_FIRSTWITHTIME / PG_AGG_LASTWITHTIME) against tests/with_time_model.py — the reference's
docId-order loops restated — over the ORACLE's match set and group assignment: every pair (value, time) bit for bit, for both modes of
pg_with_time.h (packed, wide) and the three tiers (pg_wt_reg / pg_wt_lds / pg_wt_hbm), the statistics from the model and the oracle's filter.
The kernel names are tied to the model here, not to the oracle, which has no such function."""
import os
import re

import numpy as np
import pytest

from oracle import po_datatable as dt
from pinot_amd import capi, formats
from pinot_amd.executor import NativeSegment, extract_final
from pinot_amd.query import AggregationSpec, CQuery, parse_sql, with_time_arguments
from pinot_amd.segment import build_segment
from tests import percentile_model as pm
from tests import time_transform_model as tm
from tests import variance_model as vm
from tests import with_time_model as wm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = wm.header_constants()
LDS_SLOTS = K["PG_WT_LDS_SLOTS"]
DAY_MS = 86_400_000
VALUE_COLS = ("xi", "ri", "rl", "rf", "rd", "xl", "xf", "xd")
TIME_COLS = ("td", "ti", "tl", "tw", "teq", "ts")
RAW = ["rg", "ts", "ri", "rl", "rf", "rd", "ti", "tl", "tw", "teq"]
U, INVALID = capi.PG_ERR_UNSUPPORTED, capi.PG_ERR_INVALID_ARGUMENT


def _data(n, seed=23):
    rng = np.random.default_rng(seed + n)
    f32 = lambda bits: np.array(bits, dtype=np.uint32).view(np.float32)    # noqa: E731
    f64 = lambda bits: np.array(bits, dtype=np.uint64).view(np.float64)    # noqa: E731
    rf = (rng.uniform(-1000.0, 1000.0, n)).astype(np.float32)
    rd = rng.standard_normal(n) * 1e12
    for k, b in enumerate((0x7FC12345, 0xFFC00001, 0x80000000, 0x7F800000)):   # NaN payloads, -0.0, +Inf: the last docs, likely winners of ties
        rf[(n - 1 - k) % n] = f32([b])[0]
    for k, b in enumerate((0x7FF8000000ABCDEF, 0xFFF8000000000001, 0x8000000000000000, 0xFFF0000000000000)):
        rd[(n - 1 - k) % n] = f64([b])[0]
    rd[rng.integers(0, n, max(1, n // 50))] = 2.0**31            # (int) saturates
    rd[rng.integers(0, n, max(1, n // 50))] = -3e18
    tw = rng.integers(-2**62, 2**62, n, dtype=np.int64)
    tw[rng.integers(0, n, max(2, n // 20))] = wm.LONG_MIN        # the extremes, several times each: ties at both ends
    tw[rng.integers(0, n, max(2, n // 20))] = wm.LONG_MAX
    data = {
        "g7": rng.integers(0, 7, n).astype(np.int32), "g20": rng.integers(0, 20, n).astype(np.int32), "g3": rng.integers(0, 3, n).astype(np.int32),
        "rg": (rng.integers(0, 50, n) * 1000 - 7).astype(np.int32), "ts": rng.integers(-3 * DAY_MS, 4 * DAY_MS, n).astype(np.int64),
        "s": rng.integers(0, 1000, n).astype(np.int32), "idx": np.arange(n, dtype=np.int32),
        "kfit": (np.arange(n) % LDS_SLOTS).astype(np.int32), "kover": (np.arange(n) % (LDS_SLOTS + 1)).astype(np.int32),
        "td": rng.integers(-4, 5, n).astype(np.int32) * 1000,     # nine distinct times: most groups tie at their extreme
        "ti": rng.integers(-2**31, 2**31 - 1, n, dtype=np.int64).astype(np.int32), "tl": rng.integers(0, 50, n).astype(np.int64) * 10**9 + 1_700_000_000_000,
        "tw": tw, "teq": np.full(n, 77, dtype=np.int32),
        "xi": rng.integers(-5000, 5000, n).astype(np.int32) * 400_003, "ri": rng.integers(-2**31, 2**31 - 1, n, dtype=np.int64).astype(np.int32),
        "rl": rng.integers(-2**62, 2**62, n, dtype=np.int64), "xl": rng.integers(-300, 300, n).astype(np.int64) * 10**15 + 2**40 + 5,
        "rf": rf, "rd": rd, "xf": rng.choice(rng.uniform(-1e6, 1e6, 97), n).astype(np.float32), "xd": rng.choice(rng.uniform(-1.0, 1.0, 211) * 0.1, n),
        "u1": rng.permutation(n).astype(np.int32), "u2": rng.permutation(n).astype(np.int32), "u3": rng.permutation(n).astype(np.int32),
        "txt": np.array(["t%d" % v for v in rng.integers(0, 5, n)], dtype=object).tolist(),
    }
    schema = {k: "INT" for k in data}
    schema.update(ts="LONG", tl="LONG", tw="LONG", rl="LONG", xl="LONG", rf="FLOAT", xf="FLOAT", rd="DOUBLE", xd="DOUBLE", txt="STRING")
    host = build_segment("wt_%d" % n, data, schema, no_dictionary_columns=RAW)
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
    where = sql.split(" FROM ", 1)[1].split(" GROUP BY ")[0].split(" ORDER BY ")[0].split(" LIMIT ")[0]
    ds = oracle.filter("SELECT COUNT(*) FROM " + where)
    docs, st = ds.doc_ids(), ds.stats()
    ds.free()
    return np.sort(np.asarray(docs, dtype=np.int64)), st.num_entries_scanned_in_filter


def _key_column(text, data):
    if text in data:
        return np.asarray(data[text])
    if text.startswith("divide("):
        return np.asarray(data["rg"], dtype=np.float64) / 1000.0
    return np.array(tm.evaluate(text, data[tm.columns_of(text)[0]]), dtype=np.int64)


def _norm(key):
    return tuple(float(k) if isinstance(k, (int, float, np.integer, np.floating)) else k for k in key)


def _check(seg, sql, kernel=None, num_groups_limit=0, admitted=None, qc=None):
    """Runs `sql` on the GPU and holds every FIRSTWITHTIME / LASTWITHTIME and COUNT(*) of it, its groups and its statistics to the model."""
    host, data, schema, gpu, oracle = seg
    qc = qc or parse_sql(sql)
    qc.num_groups_limit = num_groups_limit
    docs, in_filter = _filter(oracle, sql)
    groups = pm.group_docs([_key_column(g, data) for g in qc.group_by], docs) if qc.group_by else {(): docs}
    groups = {_norm(k): np.sort(v) for k, v in groups.items()}
    if admitted is not None:
        groups = {k: v for k, v in groups.items() if k in admitted}
    b = gpu.execute(qc)
    rows = {_norm(k): v for k, v in b.rows().items()}
    assert set(rows) == set(groups), sql
    read = set()
    for a in qc.aggregations:   # every distinct argument column once
        if a.function in wm.FUNCTIONS:
            read |= set(with_time_arguments(a.column)[:2])
        elif a.column:
            read |= {a.column} if a.column in data else set(re.findall(r"[A-Za-z_]\w*", a.column)) & set(data)
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
            if spec.function not in wm.FUNCTIONS:
                continue
            x, t, declared = with_time_arguments(spec.column)
            want = wm.aggregate(spec.function, schema[x], data[x], data[t], gdocs, declared)
            got = wm.pair_bits(declared, *rows[key][a])
            assert got == want, (sql, key, spec, got, want)
            assert wm.pair_bits(declared, extract_final(spec.function, rows[key][a]), want[1]) == want
    return b


def _both(x, t, declared):
    return f"FIRSTWITHTIME({x}, {t}, '{declared}'), LASTWITHTIME({x}, {t}, '{declared}')"


# ---- doc counts, layouts, declared types ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 2049])
def test_doc_counts_layouts_and_declared_types(segments, n):
    """x as dictionary INT / LONG / FLOAT / DOUBLE and raw INT / LONG / FLOAT / DOUBLE (NaN payloads, -0.0), t as dictionary INT, raw INT, raw
    LONG (packed) and raw LONG with Long.MIN_VALUE / Long.MAX_VALUE (wide), every declared type over every stored type, FIRST and LAST"""
    seg = segments(n)
    for i, x in enumerate(VALUE_COLS):
        declared = seg[2][x]
        t = ("td", "ti", "tl", "tw")[i % 4]
        for where in ("", " WHERE s < 500"):
            _check(seg, f"SELECT {_both(x, t, declared)}, COUNT(*) FROM t{where}", kernel="pg_wt_reg")
            _check(seg, f"SELECT g7, {_both(x, t, declared.lower())} FROM t{where} GROUP BY g7", kernel="pg_wt_lds")
    for declared in wm.TYPES:   # a Java primitive conversion of the stored value
        for stored in ("ri", "rl", "rf", "rd", "xl", "xd"):
            if seg[2][stored] != declared:
                _check(seg, f"SELECT g3, {_both(stored, 'tw', declared)} FROM t WHERE s < 700 GROUP BY g3", kernel="pg_wt_lds")


@pytest.mark.parametrize("n", [65, 2049])
def test_equal_times_give_the_greatest_matching_doc(segments, n):
    """all times equal behind a filter that excludes the last docs: the winner is the greatest MATCHING docId"""
    seg = segments(n)
    host, data, schema, gpu, oracle = seg
    cut = (3 * n) // 4                        # docs cut .. n - 1 do not match
    for sql in (f"SELECT {_both('u2', 'teq', 'INT')} FROM t WHERE idx < {cut}", f"SELECT g7, {_both('u2', 'teq', 'LONG')} FROM t WHERE idx < {cut} GROUP BY g7"):
        b = _check(seg, sql)
        if " GROUP BY " not in sql:
            first, last = b.aggregation_result()
            assert first == last == (int(data["u2"][cut - 1]), 77) and data["u2"][cut - 1] != data["u2"][n - 1]


def test_wide_mode_extremes(segments):
    """Long.MIN_VALUE and Long.MAX_VALUE are ordinary times: they win (several docs tie at each) and the empty marker is not confused with them"""
    seg = segments(2049)
    host, data, schema, gpu, oracle = seg
    b = _check(seg, f"SELECT {_both('ri', 'tw', 'INT')} FROM t", kernel="pg_wt_reg")
    first, last = b.aggregation_result()
    assert first[1] == wm.LONG_MIN and last[1] == wm.LONG_MAX
    assert first[0] == int(data["ri"][np.flatnonzero(data["tw"] == wm.LONG_MIN)[-1]]) and last[0] == int(data["ri"][np.flatnonzero(data["tw"] == wm.LONG_MAX)[-1]])
    # only the extremes match: every key of a pass is 0 (LAST over MIN, FIRST over MAX) or 2^64 - 1
    lo = "SELECT g7, %s FROM t WHERE tw < -9223372036854775807 GROUP BY g7" % _both("rd", "tw", "DOUBLE")
    hi = "SELECT g7, %s FROM t WHERE tw > 9223372036854775806 GROUP BY g7" % _both("rf", "tw", "FLOAT")
    for sql in (lo, hi, lo.replace("g7, ", "").replace(" GROUP BY g7", ""), hi.replace("g7, ", "").replace(" GROUP BY g7", "")):
        _check(seg, sql)


@pytest.mark.parametrize("n", [65, 2049])
def test_packed_bound_from_both_sides(gpu_api, oracle_api, n):
    """a time range one below, at and one above the packed bound of pg_with_time.h: the same pairs from both modes, two passes only above it"""
    d = wm.doc_bits(n)
    bound = wm.packed_max_range(d)
    assert bound == 2**(64 - d) - 2 and wm.packed_ok(bound, d) and not wm.packed_ok(bound + 1, d)
    rng = np.random.default_rng(n)
    pos = rng.integers(0, 4, n)                    # the time of a doc: one of four places of the range, so that groups tie at both ends
    g = rng.integers(0, 5, n).astype(np.int32)
    x = rng.integers(-2**62, 2**62, n, dtype=np.int64)
    passes = {}
    for delta in (-1, 0, 1):
        tmin = -12345
        tmax = tmin + bound + delta
        places = np.array([tmin, tmin + 1, tmax - 1, tmax], dtype=np.int64)
        t = places[pos]
        t[0], t[n - 1] = tmin, tmax                # the range is exactly [tmin, tmax]
        data = {"x": x, "t": t, "g": g, "s": (np.arange(n) % 10).astype(np.int32)}
        schema = {"x": "LONG", "t": "LONG", "g": "INT", "s": "INT"}
        host = build_segment("wt_bound_%d_%d" % (n, delta + 1), data, schema, no_dictionary_columns=["x", "t"])
        seg = (host, data, schema, NativeSegment(gpu_api, host), NativeSegment(oracle_api, host))
        try:
            b = _check(seg, f"SELECT {_both('x', 't', 'LONG')} FROM t WHERE s < 8", kernel="pg_wt_reg")
            c = _check(seg, f"SELECT g, {_both('x', 't', 'LONG')} FROM t WHERE s < 8 GROUP BY g", kernel="pg_wt_lds")
            passes[delta] = (b.stats.algorithmic_bytes, c.stats.algorithmic_bytes)
        finally:
            seg[3].destroy()
            seg[4].destroy()
    assert passes[-1] == passes[0]                 # packed: one pass
    assert passes[1][0] > passes[0][0] and passes[1][1] > passes[0][1]   # wide: the match words and the time column twice


# ---- slots -------------------------------------------------------------------------------------------------------------------------------------------
def test_two_aggregations_share_a_slot(segments):
    seg = segments(2049)
    two = _check(seg, "SELECT g7, LASTWITHTIME(ri, td, 'INT'), LASTWITHTIME(rd, td, 'DOUBLE') FROM t WHERE s < 800 GROUP BY g7", kernel="pg_wt_lds")
    one = _check(seg, "SELECT g7, LASTWITHTIME(ri, td, 'INT') FROM t WHERE s < 800 GROUP BY g7", kernel="pg_wt_lds")
    both = _check(seg, "SELECT g7, LASTWITHTIME(ri, td, 'INT'), FIRSTWITHTIME(ri, td, 'INT') FROM t WHERE s < 800 GROUP BY g7", kernel="pg_wt_lds")
    # one slot per (time column, direction): a second value column adds its gathered values only, a second direction reads no further column
    n_rows = len(one.rows())
    assert two.stats.algorithmic_bytes == one.stats.algorithmic_bytes + 8 * n_rows
    assert both.stats.algorithmic_bytes == one.stats.algorithmic_bytes + 8 * 3 * n_rows
    for key, (a, b) in two.rows().items():
        assert a[1] == b[1] and a == one.rows()[key][0]            # the same winner doc
    # the slot count decides the tier: LDS_SLOTS groups fit LDS with two aggregations over one slot, not with two slots
    seg = segments(20011)
    _check(seg, "SELECT kfit, LASTWITHTIME(ri, tl, 'INT'), LASTWITHTIME(rl, tl, 'LONG') FROM t GROUP BY kfit", kernel="pg_wt_lds")
    _check(seg, "SELECT kfit, LASTWITHTIME(ri, tl, 'INT'), FIRSTWITHTIME(rl, tl, 'LONG') FROM t GROUP BY kfit", kernel="pg_wt_hbm")


# ---- tiers -------------------------------------------------------------------------------------------------------------------------------------------
def test_tier_boundary_and_the_hbm_budget(segments, gpu_knobs, gpu_api):
    assert LDS_SLOTS == 16384
    seg = segments(20011)
    fit = "SELECT kfit, LASTWITHTIME(rd, tl, 'DOUBLE') FROM t WHERE s < 900 GROUP BY kfit"
    over = "SELECT kover, LASTWITHTIME(rd, tl, 'DOUBLE') FROM t WHERE s < 900 GROUP BY kover"
    wide = "SELECT kover, FIRSTWITHTIME(rf, tw, 'FLOAT'), COUNT(*) FROM t GROUP BY kover"
    _check(seg, fit, kernel="pg_wt_lds")          # the last table that fits the workgroup's LDS
    _check(seg, over, kernel="pg_wt_hbm")         # one group more
    _check(seg, wide, kernel="pg_wt_hbm")         # two planes, no match words
    _check(seg, fit.replace("tl", "tw"), kernel="pg_wt_lds")   # wide mode in LDS
    table_bytes = (LDS_SLOTS + 1) * 8
    gpu_knobs(PG_WT_HBM_MAX_BYTES=table_bytes)
    _check(seg, over, kernel="pg_wt_hbm")         # exactly at the budget
    _refused(gpu_api, seg[3], parse_sql(wide), U, "more than PG_WT_HBM_MAX_BYTES")   # the doc plane counts
    gpu_knobs(PG_WT_HBM_MAX_BYTES=table_bytes - 1)
    _refused(gpu_api, seg[3], parse_sql(over), U, "more than PG_WT_HBM_MAX_BYTES")
    _check(seg, fit, kernel="pg_wt_lds")          # the LDS tier does not ask the budget


# ---- query shapes ------------------------------------------------------------------------------------------------------------------------------------
SHAPES = [
    "SELECT g7, g20, LASTWITHTIME(xd, ts, 'DOUBLE'), FIRSTWITHTIME(ri, ti, 'LONG'), COUNT(*) FROM t WHERE s < 800 GROUP BY g7, g20",
    "SELECT rg, LASTWITHTIME(rf, td, 'FLOAT'), LASTWITHTIME(xi, tw, 'INT') FROM t WHERE s BETWEEN 100 AND 700 GROUP BY rg",    # a raw group key; a packed and a wide slot
    "SELECT rg / 1000, FIRSTWITHTIME(rd, tl, 'DOUBLE'), COUNT(*) FROM t WHERE s < 900 GROUP BY rg / 1000",                     # an expression key
    "SELECT toEpochDays(ts), g3, LASTWITHTIME(xf, ts, 'FLOAT'), FIRSTWITHTIME(rl, td, 'LONG') FROM t GROUP BY toEpochDays(ts), g3",   # a time-bucket key
    "SELECT g7, LASTWITHTIME(xd, ts, 'DOUBLE') FROM t WHERE s > 5000 GROUP BY g7",                                             # a filter matching nothing: no group
    "SELECT g7, FIRSTWITHTIME(g7, g7, 'INT'), LASTWITHTIME(s, s, 'LONG') FROM t GROUP BY g7",                                  # x = t, dictionary time columns
]


@pytest.mark.parametrize("n", [2049, 20011])
@pytest.mark.parametrize("sql", SHAPES)
def test_shapes(segments, n, sql):
    _check(segments(n), sql)


def test_filter_matching_nothing_without_group_by(segments):
    b = _check(segments(2049), "SELECT LASTWITHTIME(ri, td, 'INT'), FIRSTWITHTIME(rl, tw, 'LONG'), LASTWITHTIME(rf, tl, 'FLOAT'), FIRSTWITHTIME(xd, ti, 'DOUBLE') FROM t WHERE s > 5000",
               kernel="pg_wt_reg")
    got = [wm.pair_bits(d, *p) for d, p in zip(wm.TYPES, b.aggregation_result())]
    assert got == [(-2**31, wm.LONG_MIN), (wm.LONG_MIN, wm.LONG_MAX), (0x7FC00000, wm.LONG_MIN), (0x7FF8000000000000, wm.LONG_MAX)]


def test_num_groups_limit(segments):
    seg = segments(20011)
    plain = parse_sql("SELECT g7, g20, COUNT(*) FROM t WHERE s < 900 GROUP BY g7, g20")
    plain.num_groups_limit = 13
    admitted = {_norm(k) for k in seg[3].execute(plain).rows()}
    assert len(admitted) == 13
    b = _check(seg, "SELECT g7, g20, LASTWITHTIME(rd, tw, 'DOUBLE'), COUNT(*) FROM t WHERE s < 900 GROUP BY g7, g20", num_groups_limit=13, admitted=admitted)
    assert b.stats.num_groups_limit_reached == 1


def test_order_by_one_is_not_trimmed(segments):
    seg = segments(20011)
    sql = "SELECT g7, g20, LASTWITHTIME(xd, ts, 'DOUBLE'), COUNT(*) FROM t GROUP BY g7, g20 ORDER BY last_with_time(xd, ts, 'double') DESC LIMIT 1"
    qc = parse_sql(sql)
    qc.min_segment_group_trim_size = 1
    assert qc.resolved_order_by() == [(capi.ORDER_BY_AGGREGATION, 0, False)]
    b = _check(seg, sql, qc=qc)
    assert len(b.rows()) == 140 and qc.limit == 1
    qc = parse_sql("SELECT g7, g20, LASTWITHTIME(xd, ts, 'DOUBLE'), COUNT(*) FROM t GROUP BY g7, g20 ORDER BY COUNT(*) DESC LIMIT 1")
    qc.min_segment_group_trim_size = 1
    assert len(seg[3].execute(qc).rows()) == 5


def test_next_to_sum_percentile_variance_and_an_expression_aggregation(segments):
    """the frames nest: the expression pass outside, this pass inside it, the variance's and the PERCENTILE's inside that"""
    seg = segments(20011)
    host, data, schema, gpu, oracle = seg
    sql = ("SELECT g7, LASTWITHTIME(rd, ts, 'DOUBLE'), SUM(s), PERCENTILE(xi, 50), VAR_POP(xd), SUM(ri * xd), COUNT(*), FIRSTWITHTIME(xl, tw, 'INT'), MAX(s) "
           "FROM t WHERE s < 800 GROUP BY g7")
    b = _check(seg, sql)
    assert b.stats.kernel.decode().startswith("pg_expr_") and b.stats.percentile_passes == 1
    alone = gpu.execute("SELECT g7, SUM(s), PERCENTILE(xi, 50), VAR_POP(xd), SUM(ri * xd), MAX(s) FROM t WHERE s < 800 GROUP BY g7").rows()
    for key, v in b.rows().items():
        w = alone[key]
        assert v[1] == w[0] and pm.same_runs(v[2], w[1]) and v[3][0] == w[2][0] and vm.same_bits(v[3][2], w[2][2]) and vm.same_bits(v[4], w[3]) and v[7] == w[4]
    b = _check(seg, "SELECT LASTWITHTIME(rf, td, 'FLOAT'), STDDEV_POP(rl), PERCENTILE(xd, 99), SUM(ri), COUNT(*) FROM t")   # without the expression: this pass is the outer one
    assert b.stats.kernel.decode() == "pg_wt_reg"


def test_star_tree_route_is_not_taken(gpu_api):
    from tests.fixtures import synth_star_segment
    host = synth_star_segment(num_docs=20_000)
    seg = NativeSegment(gpu_api, host)
    try:
        plain = seg.execute("SELECT h1, COUNT(*), SUM(m) FROM gpuBench GROUP BY h1")
        assert plain.stats.star_tree_index >= 0
        b = seg.execute("SELECT h1, COUNT(*), SUM(m), LASTWITHTIME(m, m, 'LONG') FROM gpuBench GROUP BY h1")
        assert b.stats.star_tree_index == -1 and b.stats.num_docs_scanned == 20_000
        for key, (count, total, pair) in b.rows().items():
            assert (count, total) == tuple(plain.rows()[key]) and pair[0] == pair[1]
    finally:
        seg.destroy()


# ---- the data table ----------------------------------------------------------------------------------------------------------------------------------
def test_data_table_bytes_and_names(segments, monkeypatch):
    """A column is an OBJECT of ObjectSerDeUtils type 27 / 28 / 29 / 30 holding ValueLongPair#toBytes — the value big-endian (4 or 8 bytes), then
    the time as a big-endian long; its name is getType().getName().toLowerCase() + "(" + the argument list + ")" """
    inner = dt.deserialize_object
    monkeypatch.setattr(dt, "deserialize_object", lambda kind, b: ("ValueLongPair", kind, bytes(b)) if kind in (27, 28, 29, 30) else inner(kind, b))
    host, data, schema, gpu, oracle = segments(2049)
    aggs = [("LASTWITHTIME", "ri", "ts", "INT"), ("FIRSTWITHTIME", "rl", "tw", "LONG"), ("LASTWITHTIME", "rd", "td", "FLOAT"), ("FIRSTWITHTIME", "rd", "tl", "DOUBLE")]
    sql = "SELECT g3, COUNT(*), %s FROM t WHERE s < 500 GROUP BY g3" % ", ".join(f"{f}({x},{t},'{d}')" for f, x, t, d in aggs)
    r = gpu.execute_native(sql, keep_device_table=False)
    t = dt.parse_data_table_v4(r.data_table_v4())
    r.free()
    assert t["names"] == ["g3", "count(*)", "lastwithtime(ri,ts,'INT')", "firstwithtime(rl,tw,'LONG')", "lastwithtime(rd,td,'FLOAT')", "firstwithtime(rd,tl,'DOUBLE')"]
    assert t["types"] == ["INT", "LONG", "OBJECT", "OBJECT", "OBJECT", "OBJECT"] and len(t["rows"]) == 3
    docs, _ = _filter(oracle, sql)
    for row in t["rows"]:
        gdocs = docs[np.asarray(data["g3"])[docs] == row[0]]
        assert row[1] == len(gdocs)
        for cell, (f, x, tc, d) in zip(row[2:], aggs):
            want = wm.aggregate(f, schema[x], data[x], data[tc], gdocs, d)
            assert cell == ("ValueLongPair", wm.OBJECT_TYPE[d], wm.to_bytes(want, d)) and len(cell[2]) == (12 if d in ("INT", "FLOAT") else 16), (row[0], f, x)
    r = gpu.execute_native("SELECT FIRST_WITH_TIME(xf, ts, 'float') FROM t WHERE s > 5000", keep_device_table=False)
    t = dt.parse_data_table_v4(r.data_table_v4())
    r.free()
    assert t["names"] == ["firstwithtime(xf,ts,'float')"]
    assert [list(row) for row in t["rows"]] == [[("ValueLongPair", 29, bytes.fromhex("7fc00000" "7fffffffffffffff"))]]


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------
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


def _raw_query(function, column, group_by=()):
    qc = parse_sql("SELECT COUNT(*) FROM t" + (" GROUP BY " + ", ".join(group_by) if group_by else ""))
    qc.aggregations = [AggregationSpec(function, column)]
    return qc


def test_refusals(gpu_api):
    from pinot_amd.segment import build_mv_column
    host, data, schema = _data(2049, seed=3)
    rng = np.random.default_rng(1)
    n = host.total_docs
    host.columns["mv"] = build_mv_column("mv", [list(rng.integers(0, 20, rng.integers(1, 4))) for _ in range(n)], "INT")
    nulls = np.frombuffer(formats.serialize_roaring(np.array([3, 77, 2000], dtype=np.int64)), dtype=np.uint8)
    host.columns["xi"].null_vector = nulls
    host.columns["td"].null_vector = nulls
    host.columns["g20"].null_vector = nulls
    seg = NativeSegment(gpu_api, host)
    try:
        for fn in ("FIRSTWITHTIME", "LASTWITHTIME"):
            for declared in ("BOOLEAN", "STRING", "boolean", "BIG_DECIMAL", "TIMESTAMP", "JSON", "BYTES"):
                _refused(gpu_api, seg, parse_sql(f"SELECT {fn}(ri, ts, '{declared}') FROM t"), U, f"{fn} with the declared type '{declared.upper()}'")
            _refused(gpu_api, seg, parse_sql(f"SELECT {fn}(txt, ts, 'INT') FROM t"), U, f"{fn} over the STRING column txt")
            _refused(gpu_api, seg, parse_sql(f"SELECT {fn}(ri, txt, 'INT') FROM t"), U, f"{fn} over the STRING time column txt")
            _refused(gpu_api, seg, parse_sql(f"SELECT {fn}(mv, ts, 'INT') FROM t"), U, f"{fn} over the multi-value column mv")
            _refused(gpu_api, seg, parse_sql(f"SELECT {fn}(ri, mv, 'INT') FROM t"), U, f"{fn} over the multi-value time column mv")
            _refused(gpu_api, seg, parse_sql(f"SELECT {fn}(ri, rd, 'INT') FROM t"), U, f"{fn} with the DOUBLE time column rd")
            _refused(gpu_api, seg, parse_sql(f"SELECT {fn}(ri, xf, 'INT') FROM t"), U, f"{fn} with the FLOAT time column xf")
            _refused(gpu_api, seg, parse_sql(f"SELECT g7, {fn}(ri + xi, ts, 'INT') FROM t GROUP BY g7"), U, f"{fn} over an expression")
            # malformed argument lists
            _refused(gpu_api, seg, _raw_query(fn, "ri,ts"), INVALID, f"{fn} takes 3 arguments")
            _refused(gpu_api, seg, _raw_query(fn, "ri,ts,'INT','x'"), INVALID, f"{fn} takes 3 arguments")
            _refused(gpu_api, seg, _raw_query(fn, "ri"), INVALID, f"{fn} takes 3 arguments")
            _refused(gpu_api, seg, _raw_query(fn, "ri,ts,INT"), INVALID, "must be a quoted data type literal")
            _refused(gpu_api, seg, _raw_query(fn, "ri,ts,'FOO'"), INVALID, "'FOO' is no data type")
            _refused(gpu_api, seg, _raw_query(fn, "ri,,'INT'"), INVALID, "an empty argument")
            _refused(gpu_api, seg, _raw_query(fn, "ri,ts,'INT"), INVALID, "unterminated quote")
            _refused(gpu_api, seg, _raw_query(fn, "'ri',ts,'INT'"), INVALID, "must be a column")
            _refused(gpu_api, seg, _raw_query(fn, None), INVALID, "needs its argument list")
            _refused(gpu_api, seg, _raw_query(fn, "ri,nope,'INT'"), capi.PG_ERR_NOT_FOUND, "column not found: nope")
        _refused(gpu_api, seg, parse_sql("SELECT g7, LASTWITHTIME(ri, ts + 1, 'INT') FROM t GROUP BY g7"), U, "LASTWITHTIME over an expression")
        _refused(gpu_api, seg, parse_sql("SELECT mv, LASTWITHTIME(xd, ts, 'DOUBLE') FROM t GROUP BY mv"), U, "next to the multi-value group-by column mv")
        for x, t, text in (("xi", "ts", "LASTWITHTIME over xi, which holds nulls"), ("ri", "td", "LASTWITHTIME over td, which holds nulls"),
                           ("ri", "ts", "grouped by g20, which holds nulls")):
            qc = parse_sql(f"SELECT g20, LASTWITHTIME({x}, {t}, 'INT') FROM t GROUP BY g20")
            qc.flags |= capi.QUERY_FLAG_NULL_HANDLING
            _refused(gpu_api, seg, qc, U, text)
        qc = parse_sql("SELECT g7, LASTWITHTIME(ri, ts, 'INT'), SUM(ri) FROM t GROUP BY g7")   # columns without nulls run under the flag
        qc.flags |= capi.QUERY_FLAG_NULL_HANDLING
        assert len(seg.execute(qc).rows()) == 7
        _refused(gpu_api, seg, parse_sql("SELECT u1, u2, u3, LASTWITHTIME(xd, ts, 'DOUBLE') FROM t GROUP BY u1, u2, u3"), U, "group key space over 2^32")
        five = ", ".join(f"{f}(ri, {t}, 'INT')" for f, t in (("LASTWITHTIME", "td"), ("LASTWITHTIME", "ti"), ("LASTWITHTIME", "tl"), ("LASTWITHTIME", "tw"), ("FIRSTWITHTIME", "td")))
        _refused(gpu_api, seg, parse_sql(f"SELECT {five} FROM t"), U, "more than 4 distinct (time column, direction) pairs")
        eight = ", ".join(f"LASTWITHTIME({x}, ts, '{schema[x]}')" for x in VALUE_COLS)
        assert len(seg.execute(f"SELECT {eight} FROM t").aggregation_result()) == 8
        _refused(gpu_api, seg, parse_sql(f"SELECT {eight}, LASTWITHTIME(s, ts, 'INT') FROM t"), U, "more than 8 FIRSTWITHTIME / LASTWITHTIME aggregations")
        # a result carrying one is merged on the Java side
        a = seg.execute_native("SELECT g7, COUNT(*), LASTWITHTIME(xd, ts, 'DOUBLE') FROM t GROUP BY g7")
        b = seg.execute_native("SELECT g7, COUNT(*), LASTWITHTIME(xd, ts, 'DOUBLE') FROM t GROUP BY g7")
        with pytest.raises(capi.NativeError) as e:
            a.merge(b)
        assert e.value.status == U and "merged on the Java side" in e.value.message and "LASTWITHTIME" in e.value.message
        a.free()
        b.free()
    finally:
        seg.destroy()


# ---- the build ---------------------------------------------------------------------------------------------------------------------------------------
def test_with_time_kernels_use_no_scratch():
    """the build leaves hipcc's kernel-resource-usage remarks of pg_kernels_withtime.hip behind: no kernel of the path may spill"""
    log = os.path.join(ROOT, "pinot_amd", "csrc", "pg_kernels_withtime.resources.log")
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
    for k in ("pg_wt_reg", "pg_wt_lds", "pg_wt_hbm", "pg_wt_gather"):
        assert usage.get(k) == 0, (k, usage.get(k))
