"""SELECT DISTINCT on the GPU path (PG_QUERY_FLAG_DISTINCT) against the test-side model (tests/distinct_model.py) over the ORACLE's match
set, and against the oracle's own GROUP BY where the two coincide: rows, numDocsScanned, numEntriesScannedPostFilter and — where the
reference's count is reproduced — numEntriesScannedInFilter."""
import ctypes as C

import numpy as np
import pytest

from oracle import po_datatable as dt
from pinot_amd import capi
from pinot_amd.executor import CancelToken, NativeSegment, _key_repr
from pinot_amd.query import CQuery, parse_sql
from pinot_amd.segment import build_segment, decode_column
from tests import distinct_model as dm
from tests.fixtures import SV_FILTER, sv_segment

pytestmark = pytest.mark.gpu
UNBOUNDED = capi.LIMIT_UNBOUNDED


@pytest.fixture(scope="module")
def sv(gpu_api, oracle_api, sv_data):
    host = sv_segment(sv_data)
    g, o = NativeSegment(gpu_api, host), NativeSegment(oracle_api, host)
    yield host, g, o
    g.destroy()
    o.destroy()


def _synth(n=2_000_000, seed=5):
    rng = np.random.default_rng(seed)
    data = {
        "g1": rng.integers(0, 100, n).astype(np.int32),
        "g2": rng.integers(0, 50, n).astype(np.int32),
        "u": rng.integers(0, 1_000_000, n).astype(np.int32),
        "f": rng.integers(0, 16, n).astype(np.int32),
        "s": rng.integers(0, 1_000_000, n).astype(np.int32),
        "ri": rng.integers(-500, 500, n).astype(np.int32),
        "rl": rng.integers(-400, 400, n).astype(np.int64) * 0x1_0000_0003,
        "rf": rng.choice(np.array([0.0, -0.0, 1.5, -2.25, np.nan, np.inf, 3e10], dtype=np.float32), n),
        "rd": rng.choice(np.array([0.0, -0.0, 0.1, np.nan, -1e300, 7.0], dtype=np.float64), n),
        "rs": np.array(["k%d" % v for v in rng.integers(0, 300, n)], dtype=object).tolist(),
    }
    data["rd"][rng.integers(0, n, 20)] = np.frombuffer(np.array([0x7FF8000000000123], dtype=np.uint64).tobytes(), dtype=np.float64)[0]  # another NaN
    schema = {"g1": "INT", "g2": "INT", "u": "INT", "f": "INT", "s": "INT", "ri": "INT", "rl": "LONG", "rf": "FLOAT", "rd": "DOUBLE", "rs": "STRING"}
    return build_segment("distinct_0", data, schema, inverted_index_columns=["f"], no_dictionary_columns=["ri", "rl", "rf", "rd", "rs"]), data


@pytest.fixture(scope="module")
def synth(gpu_api, oracle_api):
    host, data = _synth()
    g, o = NativeSegment(gpu_api, host), NativeSegment(oracle_api, host)
    yield host, data, g, o
    g.destroy()
    o.destroy()


def _ids(host, data, col):
    """per-doc value-ordered ids and their decoded values (the model's input)"""
    c = host.columns[col]
    if c.has_dictionary:
        return decode_column(c, host.total_docs, dict_ids=True).astype(np.int64), list(c.dict_values)
    return dm.raw_ids(np.asarray(data[col]))


def _model(host, data, oracle, sql, dict_path=False):
    qc = parse_sql(sql)
    ids, vals = zip(*[_ids(host, data, c) for c in qc.distinct])
    order = [(qc.distinct.index(t), asc) for t, asc in qc.order_by]
    if dict_path:
        return dm.dictionary_path(len(vals[0]), qc.limit, bool(order) and not order[0][1]), vals
    where = sql.split(" FROM ", 1)[1]
    fsql = "SELECT COUNT(*) FROM " + where.split(" ORDER BY ")[0].split(" LIMIT ")[0]
    docs = oracle.filter(fsql).doc_ids() if " WHERE " in fsql else _all_docs(oracle, host)
    return dm.distinct(ids, docs, qc.limit, order or None), vals


def _all_docs(oracle, host):
    return oracle.filter("SELECT COUNT(*) FROM t").doc_ids()   # no filter: the segment's docs (behind an upsert snapshot: the valid ones)


def _decoded(rows, vals):
    return [tuple(_key_repr(vals[j][i]) if not isinstance(vals[j][i], np.generic) else _key_repr(vals[j][i].item()) for j, i in enumerate(r)) for r in rows]


def _check(gpu, host, data, oracle, sql, dict_path=False, filter_exact=None):
    qc = parse_sql(sql)
    rb = gpu.execute(qc)
    m, vals = _model(host, data, oracle, sql, dict_path)
    got = [tuple(_key_repr(v.item() if isinstance(v, np.generic) else v) for v in r) for r in rb.distinct_rows]
    want = _decoded(m.rows, vals)
    assert len(got) == len(set(got)), "duplicate tuples"
    if qc.order_by and m.tied:
        certain = set(want[:m.n_certain])
        assert len(got) == len(want) and certain <= set(got) and set(got) - certain <= set(_decoded(m.tied, vals)), sql
    elif qc.order_by:
        assert got == want, sql                          # sorted under ORDER BY
    elif qc.limit >= UNBOUNDED:
        assert sorted(map(repr, got)) == sorted(map(repr, want)), sql   # every tuple: a set (key order)
    else:
        assert got == want, sql                          # first-occurrence order
    st = rb.stats
    assert st.num_docs_scanned == m.num_docs_scanned, sql
    assert st.num_entries_scanned_post_filter == m.num_entries_scanned_post_filter, sql
    if filter_exact is not None:
        assert st.stats_exact == 1 and st.num_entries_scanned_in_filter == filter_exact(m), sql
    return rb, m


# ---- goldens: InnerSegmentDistinctSingleValueQueriesTest.java:33-69 ------------------------------------------------------------------
def test_golden_single_column_dictionary_path(sv, sv_data):
    host, g, o = sv
    rb, m = _check(g, host, sv_data, o, "SELECT DISTINCT column1 FROM testTable LIMIT 1000000", dict_path=True, filter_exact=lambda m: 0)
    assert rb.num_groups == 6582
    assert rb.stats.kernel.decode() == "pg_distinct_dictionary"


@pytest.mark.parametrize("sql", ["SELECT DISTINCT column1 FROM testTable ORDER BY column1 DESC LIMIT 7",
                                 "SELECT DISTINCT column5 FROM testTable ORDER BY column5 LIMIT 3"])
def test_dictionary_path_order_by(sv, sv_data, sql):
    host, g, o = sv
    rb, _ = _check(g, host, sv_data, o, sql, dict_path=True, filter_exact=lambda m: 0)
    assert rb.stats.kernel.decode() == "pg_distinct_dictionary"


def test_golden_two_columns(sv, sv_data):
    host, g, o = sv
    rb, _ = _check(g, host, sv_data, o, "SELECT DISTINCT column1, column3 FROM testTable LIMIT 1000000", filter_exact=lambda m: 0)
    assert rb.num_groups == 21968


SV_QUERIES = [
    "SELECT DISTINCT column6, column7 FROM testTable LIMIT 7",
    "SELECT DISTINCT column6, column7 FROM testTable LIMIT 1",
    "SELECT DISTINCT column6, column7 FROM testTable LIMIT 10000",
    f"SELECT DISTINCT column6, column7 FROM testTable LIMIT {UNBOUNDED}",
    "SELECT DISTINCT column6, column5, column11 FROM testTable" + SV_FILTER + " LIMIT 10000",
    "SELECT DISTINCT column11, column5, column17, column18 FROM testTable" + SV_FILTER + f" LIMIT {UNBOUNDED}",
    "SELECT DISTINCT column6, column11 FROM testTable" + SV_FILTER + " ORDER BY column11 DESC, column6 LIMIT 7",
    "SELECT DISTINCT column6, column7, column17 FROM testTable ORDER BY column7 LIMIT 7",
    "SELECT DISTINCT column17, column18 FROM testTable ORDER BY column18 DESC, column17 DESC LIMIT 10000",
]


@pytest.mark.parametrize("sql", SV_QUERIES)
def test_sv_parity(sv, sv_data, sql):
    host, g, o = sv
    _check(g, host, sv_data, o, sql)


@pytest.mark.parametrize("limit", [1, 7, 10000, UNBOUNDED])
def test_index_only_filter_early_stop(synth, limit):
    host, data, g, o = synth
    _check(g, host, data, o, f"SELECT DISTINCT g1, g2 FROM t WHERE f IN (1, 3, 5) LIMIT {limit}", filter_exact=lambda m: 0)


@pytest.mark.parametrize("limit", [1, 7, 10000, UNBOUNDED])
def test_lone_scan_early_stop(synth, limit):
    host, data, g, o = synth
    _check(g, host, data, o, f"SELECT DISTINCT u FROM t WHERE s < 300000 LIMIT {limit}",
           filter_exact=lambda m: m.lone_scan_entries_in_filter(host.total_docs))


SYNTH_QUERIES = [
    # LDS tier (5 000 keys) and HBM tier (10^8 keys)
    "SELECT DISTINCT g1, g2 FROM t ORDER BY g1, g2 LIMIT 10000",
    "SELECT DISTINCT g1, g2 FROM t ORDER BY g2 DESC LIMIT 100",
    "SELECT DISTINCT g1, g2 FROM t LIMIT 100",
    "SELECT DISTINCT u, g1 FROM t ORDER BY u DESC LIMIT 100",
    "SELECT DISTINCT u, g1 FROM t WHERE f = 2 ORDER BY g1, u LIMIT 10000",
    "SELECT DISTINCT u, g1 FROM t LIMIT 10000",
    f"SELECT DISTINCT u, g1 FROM t WHERE f = 2 AND s < 500000 LIMIT {UNBOUNDED}",
    "SELECT DISTINCT g1, f, g2 FROM t WHERE s >= 900000 LIMIT 7",
    # raw columns through their value-ordered virtual dictionaries
    "SELECT DISTINCT ri FROM t ORDER BY ri DESC LIMIT 7",
    "SELECT DISTINCT rl, g2 FROM t LIMIT 10000",
    f"SELECT DISTINCT rf FROM t LIMIT {UNBOUNDED}",
    f"SELECT DISTINCT rd, rf FROM t WHERE f < 8 LIMIT {UNBOUNDED}",
    "SELECT DISTINCT rd FROM t ORDER BY rd LIMIT 10",
    "SELECT DISTINCT rs, g1 FROM t LIMIT 10000",
]


@pytest.mark.parametrize("sql", SYNTH_QUERIES)
def test_synth_parity(synth, sql):
    host, data, g, o = synth
    _check(g, host, data, o, sql)


def test_upsert_snapshot(gpu_api, oracle_api):
    host, data = _synth(n=300_000, seed=9)
    g, o = NativeSegment(gpu_api, host), NativeSegment(oracle_api, host)
    valid = np.flatnonzero(np.random.default_rng(3).random(host.total_docs) < 0.4).astype(np.int32)
    g.set_queryable_doc_ids(valid)
    o.set_queryable_doc_ids(valid)
    try:
        # the dictionary path ignores the snapshot (the check is on QueryContext#getFilter())
        _check(g, host, data, o, "SELECT DISTINCT u FROM t LIMIT 50", dict_path=True)
        for sql in ("SELECT DISTINCT g1, g2 FROM t LIMIT 7", "SELECT DISTINCT u, g2 FROM t WHERE f = 1 ORDER BY g2 DESC LIMIT 100",
                    f"SELECT DISTINCT g2 FROM t WHERE s < 10000 LIMIT {UNBOUNDED}"):
            _check(g, host, data, o, sql)
    finally:
        g.destroy()
        o.destroy()


# ---- the oracle's GROUP BY: an unbounded DISTINCT is its key set; LIMIT n its first n groups (po_query.c:425-480) --------------------
@pytest.mark.parametrize("cols,where,limit", [
    ("g1, g2", " WHERE f IN (0, 9)", UNBOUNDED),
    ("u", " WHERE s < 200000", 5000),
    ("g1, u", "", 3000),
])
def test_against_oracle_group_by(synth, cols, where, limit):
    host, data, g, o = synth
    rb = g.execute(f"SELECT DISTINCT {cols} FROM t{where} LIMIT {limit}")
    qg = parse_sql(f"SELECT {cols}, COUNT(*) FROM t{where} GROUP BY {cols}")
    qg.num_groups_limit = 2_000_000_000 if limit == UNBOUNDED else limit
    og = o.execute(qg)
    assert set(rb.distinct_rows) == set(og.group_keys)
    assert len(rb.distinct_rows) == len(og.group_keys)


# ---- boundary ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sql", [
    "SELECT DISTINCT column6, column11 FROM testTable" + SV_FILTER + " ORDER BY column11 DESC, column6 LIMIT 7",
    "SELECT DISTINCT column1, column3 FROM testTable LIMIT 20",
    "SELECT DISTINCT column5 FROM testTable LIMIT 3",
])
def test_data_table(sv, sql):
    host, g, o = sv
    r = g.execute_native(sql, keep_device_table=False)
    try:
        p = dt.parse_data_table_v4(r.data_table_v4())
        rb = r.block()
    finally:
        r.free()
    qc = parse_sql(sql)
    assert p["names"] == qc.distinct
    assert p["types"] == [host.columns[c].data_type for c in qc.distinct]
    want = [tuple(x.item() if isinstance(x, np.generic) else x for x in row) for row in rb.distinct_rows]
    assert [tuple(row) for row in p["rows"]] == want


def _status(api, seg, sql, mutate=None):
    q = parse_sql(sql) if isinstance(sql, str) else sql
    cq = CQuery(q)
    if mutate:
        mutate(cq.query)
    s1 = api.f("query_supported")(seg.handle, cq.ptr())
    h = C.c_void_p()
    s2 = api.f("query_exec")(seg.handle, cq.ptr(), C.byref(h))
    if s2 != 0:
        assert not h.value, "a refused query left a result"
    elif h.value:
        api.call("result_free", h)
    return s1, s2


def test_refusals(gpu_api, synth, sv):
    host, data, g, o = synth
    un = (capi.PG_ERR_UNSUPPORTED, capi.PG_ERR_UNSUPPORTED)
    assert _status(gpu_api, g, "SELECT DISTINCT rs FROM t ORDER BY rs LIMIT 5") == un          # raw STRING in hash order
    assert _status(gpu_api, g, "SELECT DISTINCT u, s FROM t LIMIT 5") == un                    # 10^12 keys > 2^32
    assert _status(gpu_api, g, "SELECT DISTINCT g1 FROM t LIMIT 5", lambda q: setattr(q, "limit", 0)) == un
    assert _status(gpu_api, g, "SELECT DISTINCT g1 FROM t LIMIT 5", lambda q: setattr(q, "limit", -3)) == un

    assert _status(gpu_api, g, "SELECT DISTINCT g1, g2, u, f, s, ri, rl, rf, rd FROM t LIMIT 5") == un   # 9 columns > PG_MAX_GROUP_COLS

    def expr(q):
        arr = (C.c_char_p * 1)(b"g1 + g2")
        expr.keep = arr
        q.group_by_columns = arr
    assert _status(gpu_api, g, "SELECT DISTINCT g1 FROM t LIMIT 5", expr) == un


def test_refusals_multi_value_and_nulls(gpu_api, oracle_api):
    from pinot_amd import formats
    from pinot_amd.segment import build_mv_column
    host, data = _synth(n=50_000, seed=2)
    rng = np.random.default_rng(1)
    host.columns["mv"] = build_mv_column("mv", [list(rng.integers(0, 20, rng.integers(1, 4))) for _ in range(host.total_docs)], "INT")
    nulls = np.flatnonzero(rng.random(host.total_docs) < 0.1).astype(np.uint32)
    host.columns["g1"].null_vector = np.frombuffer(formats.serialize_roaring(nulls), dtype=np.uint8)
    g = NativeSegment(gpu_api, host)
    try:
        un = (capi.PG_ERR_UNSUPPORTED, capi.PG_ERR_UNSUPPORTED)
        assert _status(gpu_api, g, "SELECT DISTINCT mv FROM t LIMIT 5") == un
        q = parse_sql("SELECT DISTINCT g1, g2 FROM t LIMIT 5")
        q.flags |= capi.QUERY_FLAG_NULL_HANDLING
        assert _status(gpu_api, g, q) == un
        assert _status(gpu_api, g, "SELECT DISTINCT g1, g2 FROM t LIMIT 5") == (0, 0)   # the same without null handling: answered
    finally:
        g.destroy()


def test_merge_refused_and_cancel(gpu_api, synth):
    host, data, g, o = synth
    a = g.execute_native("SELECT DISTINCT g1 FROM t WHERE f = 1 LIMIT 5", keep_device_table=False)
    b = g.execute_native("SELECT DISTINCT g1 FROM t WHERE f = 2 LIMIT 5", keep_device_table=False)
    try:
        assert gpu_api.f("result_merge")(a.handle, b.handle) == capi.PG_ERR_UNSUPPORTED
    finally:
        a.free()
        b.free()
    tok = CancelToken(gpu_api)
    try:
        tok.request()
        with pytest.raises(capi.NativeError) as e:
            g.execute_native("SELECT DISTINCT u, g1 FROM t ORDER BY u LIMIT 100", keep_device_table=False, cancel=tok)
        assert e.value.status == capi.PG_ERR_CANCELLED
    finally:
        tok.destroy()
