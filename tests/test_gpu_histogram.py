"""HISTOGRAM on the GPU path (PG_AGG_HISTOGRAM) against tests/histogram_model.py over the ORACLE's match set and group assignment: every
count array exactly the model's, the statistics from the model and the oracle's filter.  The three kernel names of the path (pg_hist_one /
pg_hist_lds / pg_hist_hbm) are tied to the model here, not to the oracle, which has no histogram."""
import math
import os
import re
import struct

import numpy as np
import pytest

from oracle import po_datatable as dt
from pinot_amd import capi, formats
from pinot_amd.executor import Comm, NativeSegment, extract_final, histogram_merge
from pinot_amd.query import CQuery, parse_sql
from pinot_amd.segment import build_column, build_segment
from tests import covariance_model as cm
from tests import histogram_model as hm
from tests import percentile_model as pm
from tests import variance_model as vm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = hm.header_constants()
LDS_SLOTS = K["PG_HIST_LDS_SLOTS"]
TIER_BINS = 64
G_FIT = LDS_SLOTS // TIER_BINS          # the last key space whose table of one 64-bin histogram fits pg_hist_lds
DICT_COLS, RAW_COLS = ("xi", "xl", "xf", "xd"), ("ri", "rl", "rf", "rd")
SCHEMA_OF = {"xi": "INT", "ri": "INT", "xl": "LONG", "rl": "LONG", "xf": "FLOAT", "rf": "FLOAT", "xd": "DOUBLE", "rd": "DOUBLE",
             "one": "DOUBLE", "alt": "INT", "far": "LONG", "ev": "DOUBLE", "el": "LONG", "ef": "FLOAT"}
EDGE_LIST = [0.0, 0.1, 1.0, 2.5, 1000.0]


def _edge_values(n):
    """values equal to each edge of EDGE_LIST and of (0, 1000, 10), one ulp to either side, the zeros and the infinities, cycled over n docs"""
    base = []
    for e in EDGE_LIST + [100.0 * i for i in range(11)]:
        base += [e, math.nextafter(e, -math.inf), math.nextafter(e, math.inf)]
    base += [-0.0, math.inf, -math.inf, 5e-324, -5e-324, 999.9999999999999]
    return np.array([base[i % len(base)] for i in range(n)])


def _data(n, seed=29):
    rng = np.random.default_rng(seed + n)
    data = {
        "g7": rng.integers(0, 7, n).astype(np.int32), "g2": (np.arange(n) % 2).astype(np.int32), "g20": rng.integers(0, 20, n).astype(np.int32),
        "s": rng.integers(0, 1000, n).astype(np.int32), "c_inv1": rng.integers(0, 8, n).astype(np.int32),
        "kfit": (np.arange(n) % G_FIT).astype(np.int32), "kover": (np.arange(n) % (G_FIT + 1)).astype(np.int32),
        "xi": rng.integers(-50, 1051, n).astype(np.int32), "ri": rng.integers(-2**31, 2**31 - 1, n, dtype=np.int64).astype(np.int32) // 1_000_000,
        "xl": rng.integers(-50, 1051, n).astype(np.int64), "rl": rng.integers(-2000, 3000, n).astype(np.int64) * 7 // 10,
        "xf": rng.choice(np.concatenate((rng.uniform(-50.0, 1050.0, 95), [0.1, 0.0])), n).astype(np.float32), "rf": rng.uniform(-50.0, 1050.0, n).astype(np.float32),
        "xd": rng.choice(rng.uniform(-50.0, 1050.0, 211), n), "rd": rng.uniform(-50.0, 1050.0, n),
        "one": np.full(n, 512.5), "alt": np.where(np.arange(n) % 2 == 0, 150, 850).astype(np.int32), "far": np.full(n, 5000, dtype=np.int64) + np.arange(n),
        "ev": _edge_values(n), "el": np.array([(2**53 + 1, 2**53 - 1, 2**53, 2**53 + 2, 0, -1)[i % 6] for i in range(n)], dtype=np.int64),
        "ef": np.where(np.arange(n) % 3 == 0, np.float32(0.1), np.where(np.arange(n) % 3 == 1, np.float32(0.099999994), np.float32(1.0))).astype(np.float32),
        "u1": rng.permutation(n).astype(np.int32), "u2": rng.permutation(n).astype(np.int32), "u3": rng.permutation(n).astype(np.int32),
        "txt": np.array(["t%d" % v for v in rng.integers(0, 5, n)], dtype=object).tolist(),
    }
    schema = {k: "INT" for k in data}
    schema.update(SCHEMA_OF)
    schema.update(txt="STRING")
    host = build_segment("hist_%d" % n, data, schema, inverted_index_columns=["c_inv1"], no_dictionary_columns=["ri", "rl", "rf", "rd", "ev"])
    return host, data, schema


_SEGMENTS = {}
_BINS = {}


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
    _BINS.clear()


def _filter(oracle, sql):
    """(matching docs, numEntriesScannedInFilter) of the query's filter, from the oracle"""
    where = sql.split(" FROM ", 1)[1].split(" GROUP BY ")[0].split(" ORDER BY ")[0].split(" LIMIT ")[0]
    ds = oracle.filter("SELECT COUNT(*) FROM " + where)
    docs, st = ds.doc_ids(), ds.stats()
    ds.free()
    return docs, st.num_entries_scanned_in_filter


def _norm(key):
    return tuple(float(k) if isinstance(k, (int, float, np.integer, np.floating)) else k for k in key)


def _model_bins(host, data, schema, column):
    """(Spec, the model's bin of every doc) of a canonical argument list, computed once per segment"""
    key = (host.total_docs, id(data), column)
    if key not in _BINS:
        x, spec = hm.parse_arguments(column)
        _BINS[key] = (x, spec, np.array([hm.bin_of(spec, v) for v in hm.as_doubles(data[x], schema[x])], dtype=np.int64))
    return _BINS[key]


def _model_array(host, data, schema, column, gdocs):
    _, spec, bins = _model_bins(host, data, schema, column)
    b = bins[gdocs]
    assert (b >= hm.NONE).all(), "the reference throws on this input"
    return tuple(float(c) for c in np.bincount(b[b >= 0], minlength=spec.n_bins))


def _check(seg, sql, kernel=None, qc=None):
    """Runs `sql` on the GPU and holds every HISTOGRAM and COUNT(*) of it, its groups and its statistics to the model."""
    host, data, schema, gpu, oracle = seg
    qc = qc or parse_sql(sql)
    docs, in_filter = _filter(oracle, sql)
    groups = pm.group_docs([np.asarray(data[g]) for g in qc.group_by], docs) if qc.group_by else {(): np.asarray(docs, dtype=np.int64)}
    groups = {_norm(k): v for k, v in groups.items()}
    b = gpu.execute(qc)
    rows = {_norm(k): v for k, v in b.rows().items()}
    assert set(rows) == set(groups), sql
    read = set(qc.group_by)
    for a in qc.aggregations:   # a histogram reads its first argument; an expression's operand columns and a covariance's two arguments count once each
        if a.function == "HISTOGRAM":
            read.add(a.column.split(",")[0])
        elif a.column:
            read |= {a.column} if a.column in data else set(re.findall(r"[A-Za-z_]\w*", a.column)) & set(data)
    assert (b.stats.num_docs_scanned, b.stats.num_entries_scanned_post_filter) == pm.statistics(len(docs), read), sql
    assert b.stats.num_entries_scanned_in_filter == in_filter and b.stats.stats_exact == 1 and b.stats.num_total_docs == host.total_docs, sql
    assert b.stats.star_tree_index == -1
    if kernel is not None:
        assert b.stats.kernel.decode() == kernel, sql
    for key, gdocs in groups.items():
        for a, spec in enumerate(qc.aggregations):
            if spec.function == "COUNT":
                assert rows[key][a] == len(gdocs), (sql, key)
            if spec.function != "HISTOGRAM":
                continue
            want = _model_array(host, data, schema, spec.column, gdocs)
            got = rows[key][a]
            assert isinstance(got, tuple) and got == want, (sql, key, spec.column[:60], got[:12], want[:12])
            assert extract_final("HISTOGRAM", got) == want
    return b


# ---- the first case: fails on a tree without the feature with a SqlError --------------------------------------------------------------------------
def test_histogram_of_a_raw_double_column(segments):
    b = _check(segments(257), "SELECT HISTOGRAM(rd, 0, 1000, 10) FROM t", kernel="pg_hist_one")
    assert sum(b.aggregation_result()[0]) <= 257


# ---- doc counts, layouts, filters ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257, 2047, 2049])
def test_doc_counts_and_column_layouts(segments, n):
    """INT / LONG / FLOAT / DOUBLE arguments, dictionary-encoded and raw; no filter, a scan filter and an index filter; without GROUP BY and
    with one column; the equal-width and the edge form"""
    seg = segments(n)
    for i, col in enumerate(DICT_COLS + RAW_COLS):
        where = ("", " WHERE s < 500", " WHERE c_inv1 IN (1, 5)")[i % 3]
        form = (f"HISTOGRAM({col}, 0, 1000, 10)", f"HISTOGRAM({col}, ARRAY[0, 0.1, 1, 2.5, 1000])")[i % 2]
        other = (f"HISTOGRAM({col}, 0, 1000, 10)", f"HISTOGRAM({col}, ARRAY[0, 0.1, 1, 2.5, 1000])")[(i + 1) % 2]
        for w in {"", where}:
            _check(seg, f"SELECT {form}, COUNT(*) FROM t{w}", kernel="pg_hist_one")
            _check(seg, f"SELECT g7, {other} FROM t{w} GROUP BY g7", kernel="pg_hist_lds")


# ---- bins ---------------------------------------------------------------------------------------------------------------------------------------------------
def _edges(count, infinite):
    body = [repr(-40.0 + 1100.0 * i / (count - 1)) for i in range(count)]
    if infinite:
        body[0], body[-1] = '"-Infinity"', '"Infinity"'
    return "ARRAY[" + ", ".join(body) + "]"


@pytest.mark.parametrize("args", ["0, 1000, 1", "0, 1000, 2", "0, 1000, 10", "-50, 1050, 63", "0, 1000, 64", "-10.5, 990.25, 65", "0, 1000, 1000"]
                         + [_edges(c, inf) for c in (2, 3, 65, 1001) for inf in (False, True)], ids=lambda a: a[:28].replace(" ", ""))
def test_bin_counts_of_both_forms(segments, args):
    """63 / 64 / 65 bins bracket one wavefront's distinct-bin loop; 1 001 edges are staged in LDS beside the table"""
    seg = segments(2049)
    _check(seg, f"SELECT HISTOGRAM(rd, {args}) FROM t", kernel="pg_hist_one")
    _check(seg, f"SELECT HISTOGRAM(xi, {args}), COUNT(*) FROM t WHERE s < 700", kernel="pg_hist_one")
    _check(seg, f"SELECT g7, HISTOGRAM(rf, {args}) FROM t WHERE s < 700 GROUP BY g7", kernel="pg_hist_lds")


def test_skew(segments):
    seg = segments(2049)
    for where in ("", " WHERE s < 500"):
        b = _check(seg, f"SELECT HISTOGRAM(one, 0, 1000, 10), HISTOGRAM(alt, 0, 1000, 10), HISTOGRAM(far, 0, 1000, 10) FROM t{where}", kernel="pg_hist_one")
        one, alt, far = b.aggregation_result()
        assert one[5] == b.stats.num_docs_scanned and sum(one) == one[5]               # every doc in one bin
        assert alt[1] + alt[8] == b.stats.num_docs_scanned and alt[1] > 0 and alt[8] > 0  # alternating two bins
        assert far == (0.0,) * 10                                                        # every doc outside the range
        b = _check(seg, f"SELECT g7, HISTOGRAM(far, 0, 1000, 10), HISTOGRAM(one, ARRAY[0, 512.5, 600]) FROM t{where} GROUP BY g7", kernel="pg_hist_lds")
        assert len(b.rows()) == 7 and all(v[0] == (0.0,) * 10 and v[1][0] == 0.0 and v[1][1] > 0 for v in b.rows().values())   # all-zero arrays, groups still present
    b = _check(seg, "SELECT g7, HISTOGRAM(far, 0, 1000, 10) FROM t GROUP BY g7", kernel="pg_hist_lds")   # COUNT(*) alone names the groups
    assert len(b.rows()) == 7


def test_edge_values(segments):
    """values equal to each edge, to lower and upper, one ulp to either side; a LONG that rounds onto an edge; 0.1f against the edge 0.1; the
    infinities in a DOUBLE column"""
    seg = segments(2049)
    inf_edges = 'ARRAY["-Infinity", 0, 0.1, 1, 2.5, 1000, "Infinity"]'
    for shape in ("SELECT {} FROM t", "SELECT {} FROM t WHERE s < 600", "SELECT g2, {} FROM t GROUP BY g2"):
        _check(seg, shape.format("HISTOGRAM(ev, 0, 1000, 10), HISTOGRAM(ev, ARRAY[0, 0.1, 1, 2.5, 1000])"))
        b = _check(seg, shape.format(f"HISTOGRAM(ev, {inf_edges}), COUNT(*)"))
        for v in b.rows().values():
            assert sum(v[0]) == v[1] and v[0][0] > 0 and v[0][-1] > 0      # -Inf in bin 0, +Inf == upper in the last bin: every doc counts
        _check(seg, shape.format(f"HISTOGRAM(el, 0, {2**53}, 2), HISTOGRAM(el, ARRAY[0, {2**53 - 1}, {2**53}])"))
        _check(seg, shape.format("HISTOGRAM(ef, ARRAY[0, 0.1, 1]), HISTOGRAM(ef, 0.1, 1, 3)"))
    b = _check(seg, f"SELECT HISTOGRAM(el, 0, {2**53}, 2) FROM t")
    assert b.aggregation_result()[0][1] >= 3 * (2049 // 6)             # 2^53 + 1 rounds onto upper and counts in the last bin; 2^53 + 2 lies outside
    b = _check(seg, "SELECT HISTOGRAM(ef, ARRAY[0, 0.1, 1]) FROM t")
    assert b.aggregation_result()[0] == (683.0, 1366.0)               # 0.1f widened lies above the double 0.1; its float predecessor below


# ---- tiers ------------------------------------------------------------------------------------------------------------------------------------------------
def test_tier_boundary_and_the_hbm_budget(segments, gpu_knobs, gpu_api):
    assert G_FIT * TIER_BINS <= LDS_SLOTS < (G_FIT + 1) * TIER_BINS and G_FIT == 256
    seg = segments(2049)
    fit = "SELECT kfit, HISTOGRAM(rd, 0, 1000, 64) FROM t WHERE s < 900 GROUP BY kfit"
    over = "SELECT kover, HISTOGRAM(rd, 0, 1000, 64) FROM t WHERE s < 900 GROUP BY kover"
    _check(seg, fit, kernel="pg_hist_lds")         # the last table that fits the workgroup's LDS
    _check(seg, over, kernel="pg_hist_hbm")        # one group more
    _check(seg, "SELECT kover, HISTOGRAM(xi, 0, 1000, 64), COUNT(*) FROM t GROUP BY kover", kernel="pg_hist_hbm")   # no match words
    _check(seg, "SELECT kover, HISTOGRAM(xd, " + _edges(65, True) + ") FROM t GROUP BY kover", kernel="pg_hist_hbm")   # the edges read from HBM
    table_bytes = (G_FIT + 1) * TIER_BINS * 8
    gpu_knobs(PG_HIST_HBM_MAX_BYTES=table_bytes)
    _check(seg, over, kernel="pg_hist_hbm")        # exactly at the budget
    gpu_knobs(PG_HIST_HBM_MAX_BYTES=table_bytes - 1)
    _refused(gpu_api, seg[3], parse_sql(over), capi.PG_ERR_UNSUPPORTED, "more than PG_HIST_HBM_MAX_BYTES")
    _check(seg, fit, kernel="pg_hist_lds")         # the LDS tier does not ask the budget


def test_a_row_of_the_lds_slots_and_one_more(segments):
    seg = segments(2049)
    _check(seg, f"SELECT HISTOGRAM(rd, 0, 1000, {LDS_SLOTS}) FROM t WHERE s < 900", kernel="pg_hist_one")
    _check(seg, f"SELECT HISTOGRAM(rd, 0, 1000, {LDS_SLOTS + 1}) FROM t WHERE s < 900", kernel="pg_hist_hbm")
    _check(seg, f"SELECT HISTOGRAM(rd, 0, 1000, {LDS_SLOTS - 10}), HISTOGRAM(xi, 0, 1000, 10) FROM t", kernel="pg_hist_one")     # the row is the concatenation
    _check(seg, f"SELECT HISTOGRAM(rd, 0, 1000, {LDS_SLOTS - 10}), HISTOGRAM(xi, 0, 1000, 11) FROM t", kernel="pg_hist_hbm")
    _check(seg, "SELECT HISTOGRAM(xd, 0, 1000, 65536) FROM t", kernel="pg_hist_hbm")                                            # the most bins of one histogram


# ---- several histograms in one query ------------------------------------------------------------------------------------------------------------------------
def test_several_histograms_in_one_query(segments, gpu_api):
    seg = segments(2049)
    two = _check(seg, "SELECT g7, HISTOGRAM(rd, 0, 1000, 10), HISTOGRAM(rd, ARRAY[0, 10, 500, 1000]) FROM t WHERE s < 800 GROUP BY g7", kernel="pg_hist_lds")
    four = "HISTOGRAM(rd, 0, 1000, 10), HISTOGRAM(xi, 0, 1000, 10), HISTOGRAM(xi, 0, 1000, 11), HISTOGRAM(rf, ARRAY[0, 10, 500, 1000])"
    _check(seg, f"SELECT {four} FROM t", kernel="pg_hist_one")
    _check(seg, f"SELECT g7, {four}, COUNT(*) FROM t WHERE s < 800 GROUP BY g7", kernel="pg_hist_lds")
    # the same pair twice shares its slots: one array, the pass reads the same bytes; an equal pair does not count against the limit
    twice = _check(seg, "SELECT g7, HISTOGRAM(rd, 0, 1000, 10), HISTOGRAM( rd, 0.0, 1e3, 10 ), HISTOGRAM(rd, ARRAY[0, 10, 500, 1000]) FROM t WHERE s < 800 GROUP BY g7")
    assert twice.stats.algorithmic_bytes == two.stats.algorithmic_bytes
    for key, v in twice.rows().items():
        assert v[0] == v[1] == two.rows()[key][0] and v[2] == two.rows()[key][1]
    _check(seg, f"SELECT {four}, HISTOGRAM(xi, 0, 1000, 10) FROM t", kernel="pg_hist_one")
    _refused(gpu_api, seg[3], parse_sql(f"SELECT {four}, HISTOGRAM(xi, 0, 1000, 12) FROM t"), capi.PG_ERR_UNSUPPORTED, "more than 4 distinct (column, bin specification) pairs")


def test_next_to_the_other_side_passes(segments):
    """the frames nest: the expression pass outside, then FIRSTWITHTIME's, the covariance's, SKEWNESS / KURTOSIS', this one, the variance's and
    the PERCENTILE's inside it"""
    seg = segments(2049)
    host, data, schema, gpu, oracle = seg
    others = "VAR_POP(rd), COVAR_POP(xd, ri), PERCENTILE(xi, 50), SUM(ri * xd), MAX(s), KURTOSIS(rd), FIRSTWITHTIME(xi, u1, 'INT')"
    sql = f"SELECT g7, HISTOGRAM(rd, 0, 1000, 10), {others}, COUNT(*), HISTOGRAM(xl, ARRAY[0, 500, 1000]) FROM t WHERE s < 800 GROUP BY g7"
    b = _check(seg, sql)
    assert b.stats.kernel.decode().startswith("pg_expr_") and b.stats.percentile_passes == 1
    alone = gpu.execute(f"SELECT g7, {others} FROM t WHERE s < 800 GROUP BY g7").rows()
    docs, _ = _filter(oracle, sql)
    for key, v in b.rows().items():
        gdocs = docs[np.asarray(data["g7"])[docs] == key[0]]
        assert v[1] == alone[key][0] == vm.exact_tuple(vm.as_doubles(np.asarray(data["rd"])[gdocs], "DOUBLE"))
        assert v[2] == alone[key][1] == cm.exact_tuple(cm.as_doubles(np.asarray(data["xd"])[gdocs], "DOUBLE"), cm.as_doubles(np.asarray(data["ri"])[gdocs], "INT"))
        assert pm.same_runs(v[3], alone[key][2]) and vm.same_bits(v[4], alone[key][3]) and v[5] == alone[key][4] and v[6] == alone[key][5] and v[7] == alone[key][6]
    b = _check(seg, "SELECT HISTOGRAM(rf, 0, 1000, 10), VAR_POP(rf), PERCENTILE(rd, 99), COUNT(*), SUM(s) FROM t")   # without the outer passes this one is the outer one
    assert b.stats.kernel.decode() == "pg_hist_one"


def test_order_by_a_histogram_is_not_trimmed(segments):
    seg = segments(2049)
    sql = "SELECT g7, g20, HISTOGRAM(xd, 0, 1000, 10), COUNT(*) FROM t GROUP BY g7, g20 ORDER BY HISTOGRAM(xd, 0, 1000, 10) DESC LIMIT 1"
    qc = parse_sql(sql)
    qc.min_segment_group_trim_size = 1
    assert qc.resolved_order_by() == [(capi.ORDER_BY_AGGREGATION, 0, False)]
    b = _check(seg, sql, qc=qc)
    assert len(b.rows()) > 100 and qc.limit == 1        # every group: trimming by a histogram is left to the broker, LIMIT travels unchanged
    qc = parse_sql("SELECT g7, g20, HISTOGRAM(xd, 0, 1000, 10), COUNT(*) FROM t GROUP BY g7, g20 ORDER BY COUNT(*) DESC LIMIT 1")
    qc.min_segment_group_trim_size = 1
    rows = seg[3].execute(qc).rows()
    assert len(rows) == 5                               # max(5 x limit, minSegmentGroupTrimSize), ordered by the remaining aggregation
    for key, (h, count) in rows.items():
        assert sum(h) <= count


def test_filter_matching_nothing(segments):
    seg = segments(2049)
    b = _check(seg, "SELECT HISTOGRAM(xd, 0, 1000, 10), HISTOGRAM(ri, ARRAY[0, 1, 2]) FROM t WHERE s > 5000", kernel="pg_hist_one")
    assert b.aggregation_result() == [(0.0,) * 10, (0.0, 0.0)]        # numBins zeros
    assert len(_check(seg, "SELECT g7, HISTOGRAM(xd, 0, 1000, 10) FROM t WHERE s > 5000 GROUP BY g7").rows()) == 0   # with GROUP BY: no group


def test_star_tree_route_is_not_taken(gpu_api):
    from tests.fixtures import synth_star_segment
    host = synth_star_segment(num_docs=20_000)
    seg = NativeSegment(gpu_api, host)
    try:
        plain = seg.execute("SELECT h1, COUNT(*), SUM(m) FROM gpuBench GROUP BY h1")
        assert plain.stats.star_tree_index >= 0
        b = seg.execute("SELECT h1, COUNT(*), SUM(m), HISTOGRAM(m, ARRAY[\"-Infinity\", 0, \"Infinity\"]) FROM gpuBench GROUP BY h1")
        assert b.stats.star_tree_index == -1 and b.stats.num_docs_scanned == 20_000
        for key, (count, total, h) in b.rows().items():
            assert (count, total) == tuple(plain.rows()[key]) and sum(h) == count
    finally:
        seg.destroy()


# ---- the golden queries themselves ----------------------------------------------------------------------------------------------------------------------------
def test_the_golden_queries(gpu_api):
    g = hm.golden()
    data, types = hm.golden_columns(g)
    data["ceilKey"] = np.ceil(data["intColumn"] / 400.0).astype(np.int32)     # CEIL(DIV(intColumn,400)) as a column: expression keys are another path's subject
    host = build_segment("hist_golden", data, dict(types, ceilKey="INT"), no_dictionary_columns=["longColumn"])
    seg = NativeSegment(gpu_api, host)
    try:
        ran = 0
        for case in g["cases"]:
            if "(" in case["x"]:      # the ADD(...) argument: an expression, refused on this path (the model test computes it)
                continue
            for where, want in ((case.get("where"), case["expected"]), (g["filter"], case.get("expected_with_filter"))):
                if want is None:
                    continue
                sql = f"SELECT HISTOGRAM({case['x']}, {case['args']}) FROM testTable" + (f" WHERE {where}" if where else "")
                b = seg.execute(sql)
                got = b.aggregation_result()[0]
                assert got == tuple(float(v) for v in want) and b.stats.kernel.decode() == "pg_hist_one", sql
                ran += 1
                if where is None and "expected_four_segments" in case:
                    assert histogram_merge(histogram_merge(got, got), histogram_merge(got, got)) == tuple(float(v) for v in case["expected_four_segments"])
        assert ran >= 17
        gb = g["group_by"]
        rows = seg.execute(f"SELECT ceilKey, HISTOGRAM({gb['x']}, {gb['args']}) FROM testTable GROUP BY ceilKey").rows()
        assert {int(k[0]): v[0] for k, v in rows.items()} == {int(k): tuple(float(e) for e in v) for k, v in gb["expected"].items()}
    finally:
        seg.destroy()


# ---- the data table -----------------------------------------------------------------------------------------------------------------------------------------
def test_data_table_bytes_and_names(segments, monkeypatch):
    """A column is an OBJECT of ObjectSerDeUtils type 3, the DoubleArrayList PERCENTILE already writes: int size, the doubles, big-endian; its
    name is histogram(x), without the bin arguments"""
    inner = dt.deserialize_object
    monkeypatch.setattr(dt, "deserialize_object", lambda kind, b: ("DoubleArrayList", struct.unpack_from(">%dd" % struct.unpack_from(">i", b)[0], b, 4)) if kind == 3 else inner(kind, b))
    host, data, schema, gpu, oracle = segments(2049)
    sql = "SELECT g2, COUNT(*), HISTOGRAM(rd, 0, 1000, 10), HISTOGRAM( xi , ARRAY[\"-Infinity\", 0, 1000]) FROM t WHERE s < 500 GROUP BY g2"
    qc = parse_sql(sql)
    r = gpu.execute_native(sql, keep_device_table=False)
    t = dt.parse_data_table_v4(r.data_table_v4())
    r.free()
    assert t["names"] == ["g2", "count(*)", "histogram(rd)", "histogram(xi)"]
    assert t["types"] == ["INT", "LONG", "OBJECT", "OBJECT"] and len(t["rows"]) == 2
    docs, _ = _filter(oracle, sql)
    for row in t["rows"]:
        gdocs = docs[np.asarray(data["g2"])[docs] == row[0]]
        assert row[1] == len(gdocs)
        for cell, spec in zip(row[2:], qc.aggregations[1:]):
            assert cell == ("DoubleArrayList", _model_array(host, data, schema, spec.column, gdocs)), (row[0], spec.column)
    r = gpu.execute_native("SELECT HISTOGRAM(xd, 0, 1000, 3) FROM t WHERE s > 5000", keep_device_table=False)
    t = dt.parse_data_table_v4(r.data_table_v4())
    r.free()
    assert t["names"] == ["histogram(xd)"] and [list(row) for row in t["rows"]] == [[("DoubleArrayList", (0.0, 0.0, 0.0))]]


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------------
def _refused(gpu_api, seg, qc, status, text, calls=("query_supported", "query_exec")):
    for call in calls:
        cq = CQuery(qc)
        h = capi.C.c_void_p()
        with pytest.raises(capi.NativeError) as e:
            if call == "query_supported":
                gpu_api.call(call, seg.handle, cq.ptr())
            else:
                gpu_api.call(call, seg.handle, cq.ptr(), capi.C.byref(h))
        assert e.value.status == status and text in e.value.message, (call, e.value.message)


def _with_column(column):
    qc = parse_sql("SELECT HISTOGRAM(xd, 0, 1, 2) FROM t")
    qc.aggregations[0].column = column
    return qc


def test_the_inputs_on_which_the_reference_throws(gpu_api):
    """a matching NaN, and 0.9999999999999999 under (0, 1, 3): refused by pg_query_exec alone, each with its text; the same queries run when a
    filter excludes that doc"""
    n = 300
    d = np.linspace(0.0, 0.9, n)
    nan = d.copy()
    nan[5] = math.nan
    top = d.copy()
    top[9] = 0.9999999999999999
    data = {"nan": nan, "top": top, "fnan": nan.astype(np.float32), "s": np.arange(n).astype(np.int32), "g": (np.arange(n) % 3).astype(np.int32)}
    schema = {"nan": "DOUBLE", "top": "DOUBLE", "fnan": "FLOAT", "s": "INT", "g": "INT"}
    seg = NativeSegment(gpu_api, build_segment("hist_throws", data, schema, no_dictionary_columns=["nan", "top", "fnan"]))
    try:
        U = capi.PG_ERR_UNSUPPORTED
        for agg in ("HISTOGRAM(nan, 0, 1, 3)", "HISTOGRAM(nan, ARRAY[0, 0.5, 1])", "HISTOGRAM(fnan, ARRAY[\"-Infinity\", 0.5, \"Infinity\"])"):
            for shape in ("SELECT {} FROM t{}", "SELECT g, {} FROM t{} GROUP BY g"):
                qc = parse_sql(shape.format(agg, ""))
                gpu_api.call("query_supported", seg.handle, CQuery(qc).ptr())      # the plan knows no values
                _refused(gpu_api, seg, qc, U, "a matching doc whose value is NaN", calls=("query_exec",))
                b = seg.execute(shape.format(agg, " WHERE s > 5"))
                assert sum(sum(v[0]) for v in b.rows().values()) == n - 6
        for bins in (3, 7):
            for shape in ("SELECT {} FROM t{}", "SELECT g, {} FROM t{} GROUP BY g"):
                qc = parse_sql(shape.format(f"HISTOGRAM(top, 0, 1, {bins})", ""))
                gpu_api.call("query_supported", seg.handle, CQuery(qc).ptr())
                _refused(gpu_api, seg, qc, U, "rounds up to numBins", calls=("query_exec",))
                b = seg.execute(shape.format(f"HISTOGRAM(top, 0, 1, {bins})", " WHERE s <> 9"))
                assert sum(sum(v[0]) for v in b.rows().values()) == n - 1
        b = seg.execute("SELECT HISTOGRAM(top, 0, 1, 4), HISTOGRAM(top, ARRAY[0, 0.3333333333333333, 0.6666666666666666, 1]) FROM t")   # nothing rounds up here
        assert [sum(h) for h in b.aggregation_result()] == [n, n] and b.aggregation_result()[0][3] == 1 + sum(1 for v in d if v >= 0.75)
    finally:
        seg.destroy()


def test_plan_time_refusals(gpu_api):
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
    try:
        U, I = capi.PG_ERR_UNSUPPORTED, capi.PG_ERR_INVALID_ARGUMENT
        _refused(gpu_api, seg, parse_sql("SELECT HISTOGRAM(txt, 0, 1, 2) FROM t"), U, "HISTOGRAM over the STRING column txt")
        _refused(gpu_api, seg, parse_sql("SELECT g7, histogram(by, ARRAY[0, 1]) FROM t GROUP BY g7"), U, "HISTOGRAM over the BYTES column by")
        _refused(gpu_api, seg, parse_sql("SELECT HISTOGRAM(mv, 0, 1, 2) FROM t"), U, "HISTOGRAM over the multi-value column mv")
        _refused(gpu_api, seg, parse_sql("SELECT g7, HISTOGRAM(ri * xd, 0, 1, 2) FROM t GROUP BY g7"), U, "HISTOGRAM over an expression")
        _refused(gpu_api, seg, parse_sql("SELECT mv, HISTOGRAM(xd, 0, 1, 2) FROM t GROUP BY mv"), U, "next to the multi-value group-by column mv")
        _refused(gpu_api, seg, parse_sql("SELECT HISTOGRAM(nope, 0, 1, 2) FROM t"), capi.PG_ERR_NOT_FOUND, "column not found: nope")
        for col, text in (("xi", "HISTOGRAM over xi, which holds nulls"), ("xd", "grouped by g20, which holds nulls")):
            qc = parse_sql(f"SELECT g20, HISTOGRAM({col}, 0, 1000, 10) FROM t GROUP BY g20")
            qc.flags |= capi.QUERY_FLAG_NULL_HANDLING
            _refused(gpu_api, seg, qc, U, text)
        qc = parse_sql("SELECT g7, HISTOGRAM(xd, 0, 1000, 10), SUM(ri) FROM t GROUP BY g7")   # columns without nulls run under the flag
        qc.flags |= capi.QUERY_FLAG_NULL_HANDLING
        assert len(seg.execute(qc).rows()) == 7
        _refused(gpu_api, seg, parse_sql("SELECT u1, u2, u3, HISTOGRAM(xd, 0, 1, 2) FROM t GROUP BY u1, u2, u3"), U, "group key space over 2^32")
        _refused(gpu_api, seg, _with_column("xd,'-Infinity','1','2'"), U, "equal-width bins between non-finite bounds")
        _refused(gpu_api, seg, _with_column("xd,'0','Infinity','2'"), U, "equal-width bins between non-finite bounds")
        _refused(gpu_api, seg, parse_sql("SELECT HISTOGRAM(xd, 0, 1, 65537) FROM t"), U, "more than 65536 bins in one histogram")
        # the malformed lists, with the reference's texts (parse_sql raises the same before a query is built: the lists are set by hand)
        for column, text in (("xd", "Histogram expects 2 or 4 arguments, got: 1;"), ("xd,'0','1'", "Histogram expects 2 or 4 arguments, got: 3;"),
                             ("xd,'7'", "Please use the format of `Histogram(columnName, ARRAY[1,10,100])` to specify the bin edges"),
                             ("xd,arrayvalueconstructor('0')", "The number of bin edges must be greater than 1"),
                             ("xd,arrayvalueconstructor('0','0','1')", "The bin edges must be strictly increasing"),
                             ("xd,'1000','1000','10'", "The right most edge must be greater than left most edge, given 1000.0 and 1000.0"),
                             ("xd,'0','1000','-1'", "The number of bins must be greater than zero, given -1"), ("xd,'zero','1','2'", 'For input string: "zero"')):
            _refused(gpu_api, seg, _with_column(column), I, text)
        # a result carrying one is merged on the Java side
        a = seg.execute_native("SELECT g7, COUNT(*), HISTOGRAM(xd, 0, 1000, 10) FROM t GROUP BY g7")
        b = seg.execute_native("SELECT g7, COUNT(*), HISTOGRAM(xd, 0, 1000, 10) FROM t GROUP BY g7")
        with pytest.raises(capi.NativeError) as e:
            a.merge(b)
        assert e.value.status == U and "DoubleVectorOpUtils#vectorAdd" in e.value.message
        # ... also across devices: the refusal comes before any communication (a world of one rank)
        comm = Comm.init_rank(gpu_api, 0, 1, 0, Comm.unique_id(gpu_api))
        with pytest.raises(capi.NativeError) as e:
            a.all_reduce(comm)
        assert e.value.status == U and "DoubleVectorOpUtils#vectorAdd" in e.value.message
        comm.destroy()
        a.free()
        b.free()
    finally:
        seg.destroy()


# ---- the build ----------------------------------------------------------------------------------------------------------------------------------------------
def test_histogram_kernels_use_no_scratch():
    """the build leaves hipcc's kernel-resource-usage remarks of pg_kernels_hist.hip behind: no kernel of the path may spill"""
    log = os.path.join(ROOT, "pinot_amd", "csrc", "pg_kernels_hist.resources.log")
    assert os.path.exists(log), "the build writes the resource log next to the library"
    usage, cur = {}, None
    for line in open(log):
        m = re.search(r"Function Name: (\w+)", line)
        if m:
            cur = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and cur:
            usage[cur] = int(m.group(1))
    for k in ("pg_hist_one", "pg_hist_lds", "pg_hist_hbm"):
        assert usage.get(k) == 0, (k, usage.get(k))
