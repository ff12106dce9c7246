"""Exact PERCENTILE(col, p) on the GPU path (PG_AGG_PERCENTILE) against tests/percentile_model.py over the ORACLE's match set: final values
bit for bit, intermediates as equal (value, count) runs, numDocsScanned / numEntriesScannedPostFilter from the model and
numEntriesScannedInFilter from the oracle's filter.  The three kernel names of the path (pg_pctl_lds / pg_pctl_hbm / pg_pctl_sort) are tied to
the model here, not to the oracle, which has no percentile."""
import struct

import numpy as np
import pytest

from oracle import po_datatable as dt
from pinot_amd import capi, formats
from pinot_amd.executor import CancelToken, NativeSegment, percentile_expand, percentile_final
from pinot_amd.query import AggregationSpec, CQuery, QueryContext, parse_sql
from pinot_amd.segment import build_segment
from tests import percentile_model as pm
from tests.fixtures import SV_FILTER, sv_segment
from tests.kernel_inventory import snapshot_doc_ids

pytestmark = pytest.mark.gpu
CFG3_FILTER = " WHERE c_inv1 IN (0,1,2,3) AND c_inv2 IN (0,1) AND r_int BETWEEN 250000 AND 749999"   # BASELINE config 3's filter


def _f32(bits):
    return np.array([bits], dtype=np.uint32).view(np.float32)[0]


def _data(n, seed=5):
    rng = np.random.default_rng(seed + n)
    rf = rng.choice(np.array([0.0, -0.0, 1.5, -2.25, np.nan, np.inf, -np.inf, 3e10, -7e-3], dtype=np.float32), n)
    rf[rng.integers(0, n, 5)] = _f32(0x7FC00123)   # a NaN payload: one value with every other NaN
    rd = rng.choice(np.array([0.0, -0.0, 0.1, np.nan, -1e300, 7.0, np.inf], dtype=np.float64), n)
    rd[rng.integers(0, n, max(n // 100, 3))] = rng.standard_normal(max(n // 100, 3))
    rl = rng.integers(-400, 400, n).astype(np.int64) * 0x1_0000_0003
    rl[rng.integers(0, n, 7)] = 2**53 + 1            # LONGs that are no doubles
    rl[rng.integers(0, n, 7)] = 2**53 + 3
    one_big = np.zeros(n, dtype=np.int32)            # one group holding all but one doc
    one_big[n // 2] = 1
    data = {
        "g7": rng.integers(0, 7, n).astype(np.int32), "g20": rng.integers(0, 20, n).astype(np.int32), "g3": rng.integers(0, 3, n).astype(np.int32),
        "gbig": one_big, "rg": (rng.integers(0, 50, n) * 1000 - 7).astype(np.int32),
        "rs": np.array(["k%d" % v for v in rng.integers(0, 11, n)], dtype=object).tolist(),
        "v1": np.full(n, 42, dtype=np.int32),                               # cardinality 1: 1 bit
        "v7": rng.permutation(np.arange(n) % 100).astype(np.int32) * 3,     # 100 values (every one present from 100 docs on): 7 bits
        "v20": rng.integers(0, 1 << 30, n).astype(np.int32),                # ~n values: 20 bits at 700 001 docs
        "v3": rng.integers(0, 3, n).astype(np.int32) - 1,                   # 3 values: counters near n / 3
        "veq": (rng.integers(0, 7, n) * 0).astype(np.int32) + 5,
        "ld": rng.integers(0, 300, n).astype(np.int64) * 10**10,            # dictionary-encoded LONG
        "ri": rng.integers(-2**31, 2**31 - 1, n, dtype=np.int64).astype(np.int32), "rl": rl, "rf": rf, "rd": rd,
        "c_inv1": rng.integers(0, 8, n).astype(np.int32), "c_inv2": rng.integers(0, 4, n).astype(np.int32),
        "r_int": rng.integers(0, 1_000_000, n).astype(np.int32), "s": rng.integers(0, 1000, n).astype(np.int32),
        "txt": np.array(["t%d" % v for v in rng.integers(0, 5, n)], dtype=object).tolist(),
    }
    data["veq"] = data["g7"] * 11   # every value of a g7 group is equal
    schema = {k: "INT" for k in data}
    schema.update(ld="LONG", rl="LONG", rf="FLOAT", rd="DOUBLE", rs="STRING", txt="STRING")
    host = build_segment("pctl_%d" % n, data, schema, inverted_index_columns=["c_inv1", "c_inv2"],
                         no_dictionary_columns=["rg", "rs", "ri", "rl", "rf", "rd", "r_int"])
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


def _check(seg, sql, kernel=None, num_groups_limit=0, admitted=None):
    """Runs `sql` on the GPU in both result forms and holds every PERCENTILE and COUNT(*) of it, its groups and its statistics to the model."""
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
    read = set(qc.group_by) | {a.column for a in qc.aggregations if a.column}
    assert (b.stats.num_docs_scanned, b.stats.num_entries_scanned_post_filter) == pm.statistics(len(docs), read), sql
    assert b.stats.num_entries_scanned_in_filter == in_filter and b.stats.stats_exact == 1 and b.stats.num_total_docs == host.total_docs, sql
    if kernel is not None:
        assert b.stats.kernel.decode() == kernel, sql
    qf = parse_sql(sql)
    qf.num_groups_limit = num_groups_limit
    qf.flags |= capi.QUERY_FLAG_FINAL_PERCENTILE
    finals = gpu.execute(qf).rows()
    assert set(finals) == set(groups), sql
    for key, gdocs in groups.items():
        for a, spec in enumerate(qc.aggregations):
            if spec.function == "COUNT":
                assert rows[key][a] == len(gdocs) == finals[key][a], (sql, key)
            if spec.function != "PERCENTILE":
                continue
            d = pm.as_doubles(np.asarray(data[spec.column])[gdocs], schema[spec.column])
            assert pm.same_runs(rows[key][a], pm.runs(d)), (sql, key, spec)
            want = pm.final(d, spec.percentile)
            assert pm.same_double(finals[key][a], want), (sql, key, spec, finals[key][a], want)
            assert pm.same_double(percentile_final(rows[key][a], spec.percentile), want), (sql, key, spec)
    return b


# ---- the reference's goldens ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sv(gpu_api, oracle_api, sv_data):
    host = sv_segment(sv_data)
    data = {k: (v.tolist() if v.dtype.kind == "U" else v) for k, v in sv_data.items()}
    schema = {k: ("STRING" if isinstance(v, list) else "INT") for k, v in data.items()}
    g, o = NativeSegment(gpu_api, host), NativeSegment(oracle_api, host)
    yield host, data, schema, g, o
    g.destroy()
    o.destroy()


@pytest.mark.parametrize("p", [50, 90, 95, 99])
def test_reference_goldens_per_segment(sv, p):
    """testPercentile's queries on one segment (the model over four copies of it is pinned to the reference by tests/test_percentile_model.py)"""
    q = f"SELECT PERCENTILE{p}(column1), PERCENTILE(column3, {p}) FROM testTable"
    for tail in ("", SV_FILTER, " GROUP BY column9", SV_FILTER + " GROUP BY column9"):
        b = _check(sv, q + tail)
        assert b.stats.kernel.decode().startswith("pg_pctl_")
    host, data, schema, gpu, oracle = sv
    b = gpu.execute(q + SV_FILTER)
    assert (b.stats.num_docs_scanned * 4, b.stats.num_entries_scanned_in_filter * 4, b.stats.num_entries_scanned_post_filter * 4) == (24516, 252256, 49032)
    b = gpu.execute(q + SV_FILTER + " GROUP BY column9")
    assert b.stats.num_entries_scanned_post_filter * 4 == 73548


# ---- tiers --------------------------------------------------------------------------------------------------------------------------------------
def test_tiers_and_their_boundaries(segments, gpu_knobs, gpu_api):
    seg = segments(2047)
    sql = "SELECT g7, PERCENTILE(v7, 50), PERCENTILE(v7, 99.9) FROM t WHERE s < 900 GROUP BY g7"   # G x C = 7 x 100 counters
    _check(seg, sql, kernel="pg_pctl_lds")
    gpu_knobs(PG_PCTL_LDS_MAX_KEYS=700)
    _check(seg, sql, kernel="pg_pctl_lds")           # exactly at the LDS cap
    gpu_knobs(PG_PCTL_LDS_MAX_KEYS=699)
    _check(seg, sql, kernel="pg_pctl_hbm")           # one above it
    gpu_knobs(PG_PCTL_LDS_MAX_KEYS=699, PG_PCTL_HBM_MAX_BYTES=2800)
    _check(seg, sql, kernel="pg_pctl_hbm")           # exactly at the HBM budget
    gpu_knobs(PG_PCTL_LDS_MAX_KEYS=699, PG_PCTL_HBM_MAX_BYTES=2799)
    _check(seg, sql, kernel="pg_pctl_sort")          # one above it
    # the sort tier's work area over its budget: refused by exec(), which alone knows the matches; supported() lets the shape through
    gpu_knobs(PG_PCTL_LDS_MAX_KEYS=699, PG_PCTL_HBM_MAX_BYTES=2799, PG_PCTL_SORT_MAX_BYTES=1024)
    with pytest.raises(capi.NativeError) as e:
        seg[3].execute(sql)
    assert e.value.status == capi.PG_ERR_UNSUPPORTED and "PG_PCTL_SORT_MAX_BYTES" in e.value.message
    gpu_api.call("query_supported", seg[3].handle, CQuery(parse_sql(sql)).ptr())


@pytest.mark.parametrize("n", [2047, 49929, 700001])
def test_default_tiers(segments, n):
    seg = segments(n)
    _check(seg, "SELECT g7, g20, COUNT(*), PERCENTILE(v7, 95) FROM t WHERE s >= 100 GROUP BY g7, g20", kernel="pg_pctl_lds")    # 14 000 counters
    _check(seg, "SELECT g7, g20, g3, PERCENTILE(v7, 95) FROM t WHERE s >= 100 GROUP BY g7, g20, g3", kernel="pg_pctl_hbm")     # 42 000 counters
    _check(seg, "SELECT g3, PERCENTILE(v20, 50), PERCENTILE(v20, 0) FROM t GROUP BY g3", kernel="pg_pctl_lds" if n == 2047 else "pg_pctl_hbm")


# ---- shapes -------------------------------------------------------------------------------------------------------------------------------------
SHAPES = [
    "SELECT PERCENTILE(v7, 50) FROM t",
    "SELECT PERCENTILE(v1, 50), PERCENTILE(v1, 100), COUNT(*) FROM t WHERE s < 500",
    "SELECT PERCENTILE(v20, 99.9) FROM t WHERE c_inv1 IN (1, 5)",                                  # an index-only filter
    "SELECT g7, PERCENTILE(ld, 90) FROM t WHERE s BETWEEN 100 AND 700 GROUP BY g7",                 # a scan filter
    "SELECT g7, PERCENTILE(v7, 95) FROM t" + CFG3_FILTER + " GROUP BY g7",
    "SELECT g7, g20, g3, PERCENTILE(v3, 33.3) FROM t" + CFG3_FILTER + " GROUP BY g7, g20, g3",
    "SELECT rg, PERCENTILE(ri, 50), PERCENTILE(ri, 95) FROM t WHERE s < 800 GROUP BY rg",          # a raw group column, a raw INT value column
    "SELECT rs, g3, rg, PERCENTILE(rl, 50), COUNT(*) FROM t GROUP BY rs, g3, rg",                  # raw STRING / dictionary / raw INT keys, LONGs above 2^53
    "SELECT g3, PERCENTILE(rf, 0), PERCENTILE(rf, 50), PERCENTILE(rf, 100) FROM t WHERE c_inv2 = 1 GROUP BY g3",   # -0.0, NaN
    "SELECT PERCENTILE(rd, 30), PERCENTILE(rd, 99.9), PERCENTILE(rd, 100) FROM t WHERE s > 10",
    "SELECT g7, PERCENTILE(v7, 50) FROM t WHERE s > 5000 GROUP BY g7",                            # a filter matching nothing
    "SELECT PERCENTILE(v7, 50), PERCENTILE(rd, 50) FROM t WHERE s > 5000",                        # ... without GROUP BY: Double.NEGATIVE_INFINITY
    "SELECT g7, PERCENTILE(veq, 95) FROM t GROUP BY g7",                                          # a group whose values are all equal
    "SELECT gbig, PERCENTILE(v7, 50), PERCENTILE(v3, 99) FROM t GROUP BY gbig",                   # one group holding all but one doc
]


@pytest.mark.parametrize("n", [2047, 49929])
@pytest.mark.parametrize("sql", SHAPES)
def test_shapes(segments, n, sql):
    _check(segments(n), sql)


@pytest.mark.parametrize("n", [2047, 49929])
@pytest.mark.parametrize("sql", SHAPES)
def test_shapes_in_the_sort_tier(segments, gpu_knobs, n, sql):
    gpu_knobs(PG_PCTL_HBM_MAX_BYTES=4)   # every table of two counters or more is over the budget
    b = _check(segments(n), sql)
    assert b.stats.kernel.decode() == ("pg_pctl_lds" if "(v1," in sql else "pg_pctl_sort")   # a lone counter still fits


def test_filter_matching_one_doc(segments):
    seg = segments(49929)
    doc = int(np.flatnonzero(seg[1]["gbig"] == 1)[0])
    b = _check(seg, "SELECT g7, PERCENTILE(v20, 50), PERCENTILE(rd, 100) FROM t WHERE gbig = 1 GROUP BY g7")
    assert b.stats.num_docs_scanned == 1 and list(b.rows()) == [(int(seg[1]["g7"][doc]),)]


def test_large_counters_and_wide_dictionary(segments):
    """700 001 docs: a 3-value column (counters near 2^18 through the wave-level combining of the HBM tier and through LDS), a 20-bit column"""
    seg = segments(700001)
    _check(seg, "SELECT PERCENTILE(v3, 50), PERCENTILE(v3, 0), PERCENTILE(v3, 100) FROM t", kernel="pg_pctl_lds")
    _check(seg, "SELECT g7, g20, PERCENTILE(v3, 66.7) FROM t" + CFG3_FILTER + " GROUP BY g7, g20", kernel="pg_pctl_lds")
    _check(seg, "SELECT g3, PERCENTILE(v20, 95) FROM t WHERE s < 990 GROUP BY g3", kernel="pg_pctl_hbm")
    _check(seg, "SELECT PERCENTILE(rl, 99.9), PERCENTILE(rf, 50) FROM t")
    # 420 groups x ~700 000 values: ~1.2 GB of counters, over the default HBM budget
    _check(seg, "SELECT g7, g20, g3, PERCENTILE(v20, 95), PERCENTILE(v20, 50) FROM t WHERE s < 990 GROUP BY g7, g20, g3", kernel="pg_pctl_sort")
    _check(seg, "SELECT g7, g20, g3, PERCENTILE(v20, 0), COUNT(*) FROM t GROUP BY g7, g20, g3", kernel="pg_pctl_sort")   # no match words


def test_hbm_tier_combining(segments, gpu_knobs):
    gpu_knobs(PG_PCTL_LDS_MAX_KEYS=1)
    _check(segments(700001), "SELECT PERCENTILE(v3, 50) FROM t", kernel="pg_pctl_hbm")   # 3 counters, ~233 000 each: every wavefront folds its 64 docs
    _check(segments(49929), "SELECT g7, PERCENTILE(v7, 95), PERCENTILE(rd, 50) FROM t WHERE s < 700 GROUP BY g7", kernel="pg_pctl_hbm")


def test_single_doc_segment(gpu_api, oracle_api):
    data = {"g": np.array([3], dtype=np.int32), "v": np.array([-17], dtype=np.int32), "r": np.array([2.5], dtype=np.float64)}
    schema = {"g": "INT", "v": "INT", "r": "DOUBLE"}
    host = build_segment("one", data, schema, no_dictionary_columns=["r"])
    seg = (host, data, schema, NativeSegment(gpu_api, host), NativeSegment(oracle_api, host))
    try:
        _check(seg, "SELECT PERCENTILE(v, 0), PERCENTILE(v, 50), PERCENTILE(r, 100) FROM t")
        _check(seg, "SELECT g, PERCENTILE(v, 99.9), PERCENTILE(r, 1) FROM t GROUP BY g")
    finally:
        seg[3].destroy()
        seg[4].destroy()


def test_upsert_snapshot(gpu_api, oracle_api):
    host, data, schema = _data(49929, seed=9)
    g, o = NativeSegment(gpu_api, host), NativeSegment(oracle_api, host)
    keep = snapshot_doc_ids(host.total_docs)
    g.set_queryable_doc_ids(keep)
    o.set_queryable_doc_ids(keep)
    try:
        seg = (host, data, schema, g, o)
        b = _check(seg, "SELECT PERCENTILE(v7, 50), PERCENTILE(rd, 95) FROM t")
        assert b.stats.num_docs_scanned == len(keep)
        _check(seg, "SELECT g7, PERCENTILE(v20, 95), COUNT(*) FROM t WHERE s < 600 GROUP BY g7")
    finally:
        g.destroy()
        o.destroy()


# ---- several percentiles, other aggregations ---------------------------------------------------------------------------------------------------------
def test_several_percentiles_next_to_other_aggregations(segments):
    seg = segments(49929)
    host, data, schema, gpu, oracle = seg
    ps = ", ".join(f"PERCENTILE(v7, {p})" for p in (0, 50, 95, 99.9, 100))
    sql = f"SELECT g7, {ps}, COUNT(*), SUM(s), MAX(s), PERCENTILE(rd, 50) FROM t WHERE s < 800 GROUP BY g7"
    b = _check(seg, sql)
    # one counting pass per distinct percentile COLUMN: five percentiles of v7 and one of rd are two passes (pg_exec_stats.percentile_passes,
    # counted where the passes are launched), with and without the profile flag
    assert b.stats.percentile_passes == 2
    assert gpu.execute(parse_sql(sql), profile=True).stats.percentile_passes == 2
    assert gpu.execute("SELECT g7, PERCENTILE(v7, 50) FROM t GROUP BY g7").stats.percentile_passes == 1
    assert gpu.execute("SELECT g7, COUNT(*) FROM t GROUP BY g7").stats.percentile_passes == 0
    plain = oracle.execute("SELECT g7, COUNT(*), SUM(s), MAX(s) FROM t WHERE s < 800 GROUP BY g7").rows()
    rows = b.rows()
    for key, want in plain.items():
        assert rows[key][5:8] == want, key
        # p50 / p95 / p99.9 of one column come from ONE counting pass: the aggregations over v7 hold the same runs
        for a in range(1, 5):
            assert pm.same_runs(rows[key][a], rows[key][0])
    # 17 percentiles of one column: more than one selection launch takes
    many = ", ".join(f"PERCENTILE(v7, {p})" for p in np.linspace(0, 100, 17))
    _check(seg, f"SELECT g3, {many} FROM t GROUP BY g3")


def test_num_groups_limit(segments):
    seg = segments(49929)
    host, data, schema, gpu, oracle = seg
    plain = parse_sql("SELECT g7, g20, COUNT(*) FROM t WHERE s < 900 GROUP BY g7, g20")
    plain.num_groups_limit = 13
    admitted = set(gpu.execute(plain).rows())
    assert len(admitted) == 13
    b = _check(seg, "SELECT g7, g20, PERCENTILE(v7, 95), COUNT(*) FROM t WHERE s < 900 GROUP BY g7, g20", num_groups_limit=13, admitted=admitted)
    assert b.stats.num_groups_limit_reached == 1


def test_order_by_a_percentile_is_not_trimmed(segments):
    seg = segments(49929)
    qc = parse_sql("SELECT g7, g20, PERCENTILE(v7, 95), COUNT(*) FROM t GROUP BY g7, g20 ORDER BY PERCENTILE(v7, 95) DESC LIMIT 1")
    qc.min_segment_group_trim_size = 1
    assert len(seg[3].execute(qc).rows()) == 140        # every group: trimming by a PERCENTILE is left to the broker
    qc = parse_sql("SELECT g7, g20, PERCENTILE(v7, 95), COUNT(*) FROM t GROUP BY g7, g20 ORDER BY COUNT(*) DESC LIMIT 1")
    qc.min_segment_group_trim_size = 1
    rows = seg[3].execute(qc).rows()
    assert len(rows) == 5                               # max(5 x limit, minSegmentGroupTrimSize), ordered by the remaining aggregation
    for key, (runs, count) in rows.items():
        assert int(np.sum(runs[1])) == count


# ---- the data table ---------------------------------------------------------------------------------------------------------------------------------
def test_data_table_round_trip(segments, monkeypatch):
    """A PERCENTILE column is an OBJECT holding a DoubleArrayList: object type 3, a big-endian int size, big-endian doubles
    (ObjectSerDeUtils.java:482-511)"""
    inner = dt.deserialize_object

    def deserialize(kind, b):
        if kind == 3:
            n = struct.unpack_from(">i", b, 0)[0]
            assert len(b) == 4 + 8 * n
            return np.array(struct.unpack_from(f">{n}d", b, 4), dtype=np.float64)
        return inner(kind, b)
    monkeypatch.setattr(dt, "deserialize_object", deserialize)
    host, data, schema, gpu, oracle = segments(2047)
    r = gpu.execute_native("SELECT g3, COUNT(*), PERCENTILE(rd, 50), PERCENTILE95(v7) FROM t WHERE s < 500 GROUP BY g3", keep_device_table=False)
    t = dt.parse_data_table_v4(r.data_table_v4())
    rows = r.block().rows()
    r.free()
    # (the name: the reference chooses "percentile50(rd)" / "percentile(rd, 50.0)" by the SPELLING of the query, which the ABI does not carry;
    # the library writes the legacy form for an integral p — a documented divergence, DESIGN.md §4.5, not parity)
    assert t["names"][:2] == ["g3", "count(*)"] and t["types"] == ["INT", "LONG", "OBJECT", "OBJECT"]
    assert len(t["rows"]) == len(rows) == 3
    for g3, count, l_rd, l_v7 in t["rows"]:
        assert count == rows[(g3,)][0] == len(l_rd) == len(l_v7)
        assert np.array_equal(pm.order_keys(l_rd), pm.order_keys(percentile_expand(rows[(g3,)][1])))
        assert np.array_equal(l_v7, percentile_expand(rows[(g3,)][2]))
    qf = parse_sql("SELECT PERCENTILE(v7, 99.9) FROM t")
    r = gpu.execute_native(qf, keep_device_table=False)
    assert len(dt.parse_data_table_v4(r.data_table_v4())["rows"]) == 1
    r.free()
    qf.flags |= capi.QUERY_FLAG_FINAL_PERCENTILE
    r = gpu.execute_native(qf, keep_device_table=False)
    with pytest.raises(capi.NativeError) as e:
        r.data_table_v4()
    assert e.value.status == capi.PG_ERR_INVALID_ARGUMENT and "PG_QUERY_FLAG_FINAL_PERCENTILE" in e.value.message
    r.free()


# ---- raw FLOAT / DOUBLE group-by columns, a star-tree segment ---------------------------------------------------------------------------------------------
def test_raw_float_and_double_group_keys(segments):
    """the groups' keys come back as values (IEEE bits: every NaN one key, -0.0 and 0.0 two) and are joined to the percentile pass by them"""
    host, data, schema, gpu, oracle = segments(49929)
    for col in ("rf", "rd"):
        sql = f"SELECT {col}, COUNT(*), PERCENTILE(v7, 50), PERCENTILE(v7, 99.9) FROM t WHERE s < 900 GROUP BY {col}"
        docs, _ = _filter(oracle, sql)
        keys = pm.order_keys(pm.as_doubles(np.asarray(data[col])[docs], schema[col]))
        rows = gpu.execute(sql).rows()
        assert len(rows) == len(np.unique(keys))
        by_key = {}
        for k, v in rows.items():
            kv = float("nan") if k[0] == "NaN" else (-0.0 if k[0] == "-0.0" else float(k[0]))
            by_key[int(pm.order_keys(np.array([kv]))[0])] = v
        for key in np.unique(keys):
            gdocs = docs[keys == key]
            count, runs50, runs999 = by_key[int(key)]
            d = pm.as_doubles(np.asarray(data["v7"])[gdocs], "INT")
            assert count == len(gdocs) and pm.same_runs(runs50, pm.runs(d)) and pm.same_runs(runs999, pm.runs(d))


def test_star_tree_route_is_not_taken(gpu_api):
    from tests.fixtures import synth_star_segment
    host = synth_star_segment(num_docs=20_000)
    seg = NativeSegment(gpu_api, host)
    try:
        plain = seg.execute("SELECT h1, COUNT(*), SUM(m) FROM gpuBench GROUP BY h1")
        assert plain.stats.star_tree_index >= 0                      # the star-tree answers the query without a percentile ...
        b = seg.execute("SELECT h1, COUNT(*), SUM(m), PERCENTILE(m, 50) FROM gpuBench GROUP BY h1")
        assert b.stats.star_tree_index == -1 and b.stats.num_docs_scanned == 20_000   # ... never the one with it
        for key, (count, total, runs) in b.rows().items():
            assert (count, total) == tuple(plain.rows()[key]) and int(np.sum(runs[1])) == count
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


def test_refusals(gpu_api, oracle_api):
    from pinot_amd.segment import build_mv_column
    host, data, schema = _data(2047, seed=3)
    rng = np.random.default_rng(1)
    host.columns["mv"] = build_mv_column("mv", [list(rng.integers(0, 20, rng.integers(1, 4))) for _ in range(host.total_docs)], "INT")
    nulls = np.frombuffer(formats.serialize_roaring(np.array([3, 77, 2000], dtype=np.int64)), dtype=np.uint8)
    host.columns["v7"].null_vector = nulls
    host.columns["g20"].null_vector = nulls
    seg = NativeSegment(gpu_api, host)
    try:
        U, I = capi.PG_ERR_UNSUPPORTED, capi.PG_ERR_INVALID_ARGUMENT
        _refused(gpu_api, seg, parse_sql("SELECT PERCENTILE(txt, 50) FROM t"), U, "PERCENTILE over the STRING column txt")
        _refused(gpu_api, seg, parse_sql("SELECT PERCENTILE(rs, 50) FROM t"), U, "PERCENTILE over the STRING column rs")
        _refused(gpu_api, seg, parse_sql("SELECT PERCENTILE(mv, 50) FROM t"), U, "PERCENTILE over the multi-value column mv")
        _refused(gpu_api, seg, parse_sql("SELECT mv, PERCENTILE(v3, 50) FROM t GROUP BY mv"), U, "next to the multi-value group-by column mv")
        for col, text in (("v7", "PERCENTILE over v7, which holds nulls"), ("v3", "grouped by g20, which holds nulls")):
            qc = parse_sql(f"SELECT g20, PERCENTILE({col}, 50) FROM t GROUP BY g20")
            qc.flags |= capi.QUERY_FLAG_NULL_HANDLING
            _refused(gpu_api, seg, qc, U, text)
        qc = parse_sql("SELECT g7, PERCENTILE(v3, 50), SUM(v7) FROM t GROUP BY g7")   # columns without nulls run under the flag
        qc.flags |= capi.QUERY_FLAG_NULL_HANDLING
        assert len(seg.execute(qc).rows()) == 7
        for p in (100.5, -0.1, float("nan")):
            qc = QueryContext(aggregations=[AggregationSpec("PERCENTILE", "v3", 0, p)])
            _refused(gpu_api, seg, qc, I, "the percentile must be in [0, 100]")
        # agg_params == NULL
        cq = CQuery(parse_sql("SELECT PERCENTILE(v3, 50) FROM t"))
        cq.query.agg_params = None
        with pytest.raises(capi.NativeError) as e:
            gpu_api.call("query_supported", seg.handle, cq.ptr())
        assert e.value.status == I and "PERCENTILE without agg_params" in e.value.message
        # a result carrying a PERCENTILE is merged by value on the Java side
        a = seg.execute_native("SELECT g7, COUNT(*), PERCENTILE(v3, 50) FROM t GROUP BY g7")
        b = seg.execute_native("SELECT g7, COUNT(*), PERCENTILE(v3, 50) FROM t GROUP BY g7")
        with pytest.raises(capi.NativeError) as e:
            a.merge(b)
        assert e.value.status == U and "PERCENTILE results are merged by value" in e.value.message
        a.free()
        b.free()
        # cancellation: the token is polled before the ordinary part is planned
        token = CancelToken(gpu_api)
        token.request()
        with pytest.raises(capi.NativeError) as e:
            seg.execute_native("SELECT g7, PERCENTILE(v3, 50) FROM t GROUP BY g7", cancel=token)
        assert e.value.status == capi.PG_ERR_CANCELLED
        token.reset()
        r = seg.execute_native("SELECT g7, PERCENTILE(v3, 50) FROM t GROUP BY g7", cancel=token)
        assert len(r.block().rows()) == 7
        r.free()
        token.destroy()
    finally:
        seg.destroy()
