"""Selection queries on the GPU path (PG_QUERY_FLAG_SELECTION) against the test-side model (tests/selection_model.py) over the ORACLE's
match set and host-decoded columns: rows (any valid subset of the rows tied at the cut), numDocsScanned, numEntriesScannedPostFilter and,
where the reference's count has a closed form, numEntriesScannedInFilter."""
import ctypes as C
import math
import threading

import numpy as np
import pytest

from oracle import po_datatable as dt
from pinot_amd import capi
from pinot_amd.executor import CancelToken, NativeSegment
from pinot_amd.query import CQuery, parse_sql
from pinot_amd.segment import build_segment, decode_column
from tests import selection_model as sm

pytestmark = pytest.mark.gpu
UNBOUNDED = capi.LIMIT_UNBOUNDED
KMAX = 1024   # PG_SELECT_LDS_MAX_K


def _f32(bits):
    return np.array([bits], dtype=np.uint32).view(np.float32)[0]


def _synth(n=3_000_000, seed=11):
    rng = np.random.default_rng(seed)
    rf = rng.choice(np.array([0.0, -0.0, 1.5, -2.25, np.nan, np.inf, -np.inf, 3e10, -7e-3], dtype=np.float32), n)
    rf[rng.integers(0, n, 50)] = _f32(0x7FC00123)   # NaN payloads: one value with every other NaN
    rf[rng.integers(0, n, 50)] = _f32(0xFFC00000)   # a negative NaN
    rf[rng.integers(0, n, 1000)] = rng.standard_normal(1000).astype(np.float32)
    rd = rng.choice(np.array([0.0, -0.0, 0.1, np.nan, -1e300, 7.0, np.inf], dtype=np.float64), n)
    rd[rng.integers(0, n, 20)] = np.array([0x7FF8000000000123], dtype=np.uint64).view(np.float64)[0]
    rd[rng.integers(0, n, 5000)] = rng.standard_normal(5000)
    data = {
        "g1": rng.integers(0, 100, n).astype(np.int32),
        "u": rng.integers(0, 1_000_000, n).astype(np.int32),
        "f": rng.integers(0, 16, n).astype(np.int32),
        "s": rng.integers(0, 1_000_000, n).astype(np.int32),
        "lo": rng.integers(0, 3, n).astype(np.int32),
        "srt": np.sort(rng.integers(0, 50_000, n)).astype(np.int32),
        "ri": rng.integers(-2**31, 2**31 - 1, n, dtype=np.int64).astype(np.int32),
        "rl": rng.integers(-400, 400, n).astype(np.int64) * 0x1_0000_0003,
        "rf": rf,
        "rd": rd,
        "rs": np.array(["k%d" % v for v in rng.integers(0, 3000, n)], dtype=object).tolist(),
    }
    schema = {"g1": "INT", "u": "INT", "f": "INT", "s": "INT", "lo": "INT", "srt": "INT", "ri": "INT", "rl": "LONG", "rf": "FLOAT",
              "rd": "DOUBLE", "rs": "STRING"}
    host = build_segment("selection_0", data, schema, inverted_index_columns=["f"], no_dictionary_columns=["ri", "rl", "rf", "rd", "rs"])
    return host, data


@pytest.fixture(scope="module")
def synth(gpu_api, oracle_api):
    host, data = _synth()
    g, o = NativeSegment(gpu_api, host), NativeSegment(oracle_api, host)
    yield host, data, g, o
    g.destroy()
    o.destroy()


_DECODED = {}
_IDS = {}


def _column(host, data, col):
    """(values per doc, order values per doc) of a column, decoded on the host"""
    key = (id(host), col)
    if key not in _DECODED:
        c = host.columns[col]
        if c.has_dictionary:
            ids = decode_column(c, host.total_docs, dict_ids=True).astype(np.int64)
            dv = np.asarray(c.dict_values, dtype=object)
            _DECODED[key] = (dv[ids], sm.order_values(None, ids))
        else:
            v = np.asarray(data[col], dtype=object) if c.data_type == "STRING" else np.asarray(data[col])
            _DECODED[key] = (v, None if c.data_type == "STRING" else sm.order_values(v, None))
    return _DECODED[key]


def _match_docs(oracle, host, sql):
    where = sql.split(" FROM ", 1)[1]
    fsql = "SELECT COUNT(*) FROM " + where.split(" ORDER BY ")[0].split(" LIMIT ")[0]
    return oracle.filter(fsql).doc_ids()


def _model(host, data, oracle, sql):
    qc = parse_sql(sql)
    out = qc.extract_expressions(host.columns)
    vals = [_column(host, data, c)[0] for c in out]
    order, seen = [], set()
    if qc.limit > 0:
        for text, asc in qc.order_by:
            if text not in seen:
                seen.add(text)
                order.append((out.index(text), asc, _column(host, data, text)[1]))
    docs = _match_docs(oracle, host, sql)
    return sm.selection(vals, docs, qc.limit, len(set(out)), order or None), qc, out


def _order_key(row, qc, out, host, data):
    key, seen = [], set()
    for text, asc in qc.order_by:
        if text in seen:
            continue
        seen.add(text)
        v = row[out.index(text)]
        c = host.columns[text]
        if c.has_dictionary:
            if (id(host), text) not in _IDS:
                _IDS[(id(host), text)] = {x.item() if isinstance(x, np.generic) else x: i for i, x in enumerate(c.dict_values)}
            o = _IDS[(id(host), text)][v.item() if isinstance(v, np.generic) else v]
        else:
            x = float("nan") if v == "NaN" else (-0.0 if v == "-0.0" else v)
            o = int(sm.order_values(np.array([x], dtype=np.float64 if c.data_type in ("FLOAT", "DOUBLE") else np.int64), None)[0])
        key.append(o if asc else -o)
    return tuple(key)


def _check(gpu, host, data, oracle, sql, filter_exact=None, kernel=None):
    m, qc, out = _model(host, data, oracle, sql)
    rb = gpu.execute(qc)
    assert rb.key_columns == out
    got = rb.selection_rows
    if qc.order_by and qc.limit > 0:
        sm.check_ordered(got, [_order_key(r, qc, out, host, data) for r in got], m)
    else:
        assert got == m.rows, sql
    st = rb.stats
    assert st.num_docs_scanned == m.num_docs_scanned, sql
    assert st.num_entries_scanned_post_filter == m.num_entries_scanned_post_filter, sql
    assert st.num_total_docs == host.total_docs
    if filter_exact is not None:
        assert st.stats_exact == 1 and st.num_entries_scanned_in_filter == filter_exact(m), (sql, st.num_entries_scanned_in_filter)
    if kernel:
        assert st.kernel.decode() == kernel, (sql, st.kernel)
    return rb, m


# ---- selection only ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("limit", [1, 10, 25000, UNBOUNDED])
def test_no_filter(synth, limit):
    host, data, g, o = synth
    _check(g, host, data, o, f"SELECT g1, ri, rf, rs FROM t LIMIT {limit}" if limit < UNBOUNDED else f"SELECT g1 FROM t LIMIT {limit}",
           filter_exact=lambda m: 0, kernel="pg_select_gather")


def test_select_star_no_filter(synth):
    host, data, g, o = synth
    rb, _ = _check(g, host, data, o, "SELECT * FROM t LIMIT 10", filter_exact=lambda m: 0)
    assert rb.key_columns == sorted(host.columns)


@pytest.mark.parametrize("limit", [1, 10, 10000, 25000, UNBOUNDED])
def test_index_only_filter(synth, limit):
    host, data, g, o = synth
    _check(g, host, data, o, f"SELECT u, rd, rs FROM t WHERE f IN (1, 3, 5) LIMIT {limit}", filter_exact=lambda m: 0)


@pytest.mark.parametrize("limit", [1, 10, 10000, 25000, 300000])
def test_lone_scan(synth, limit):
    host, data, g, o = synth
    _check(g, host, data, o, f"SELECT u, rl FROM t WHERE s < 100000 LIMIT {limit}",
           filter_exact=lambda m: m.lone_scan_entries_in_filter(host.total_docs))


@pytest.mark.parametrize("where", [" WHERE f = 2 AND s < 500000", " WHERE f = 1 OR s < 1000", " WHERE NOT (g1 < 50) AND (f = 3 OR u > 900000)"])
@pytest.mark.parametrize("limit", [1, 10, 30000])
def test_compound_filters(synth, where, limit):
    host, data, g, o = synth
    rb, _ = _check(g, host, data, o, f"SELECT g1, rf FROM t{where} LIMIT {limit}")
    assert rb.stats.stats_exact == 1   # a segment of 3 x 10^6 docs: the iterator automaton counts the early stop


def test_limit_equal_and_above_matches(synth):
    host, data, g, o = synth
    M = len(_match_docs(o, host, "SELECT g1 FROM t WHERE u = 12345 AND f < 12"))
    assert M > 0
    for limit in (M, M + 5):
        _check(g, host, data, o, f"SELECT g1, s, rs FROM t WHERE u = 12345 AND f < 12 LIMIT {limit}")


# ---- ORDER BY ------------------------------------------------------------------------------------------------------------------------------
ORDERED = [
    "SELECT g1, u, rs FROM t ORDER BY u DESC LIMIT 10",
    "SELECT u, g1 FROM t WHERE s < 300000 ORDER BY g1 DESC, u LIMIT 100",
    "SELECT ri, g1 FROM t ORDER BY ri LIMIT 100",
    "SELECT ri FROM t WHERE f = 7 ORDER BY ri DESC LIMIT 13",
    "SELECT rl, rs FROM t ORDER BY rl DESC LIMIT 50",
    "SELECT rl, rs FROM t WHERE f IN (2, 4) ORDER BY rl LIMIT 50",
    "SELECT rf, g1 FROM t ORDER BY rf LIMIT 37",
    "SELECT rf, g1 FROM t ORDER BY rf DESC, g1 LIMIT 200",
    "SELECT rd, u FROM t ORDER BY rd LIMIT 20",
    "SELECT rd, u FROM t WHERE s >= 500000 ORDER BY rd DESC LIMIT 20",
    "SELECT lo, g1, f, rs FROM t WHERE s < 500000 ORDER BY lo DESC, g1, f DESC LIMIT 1000",
    "SELECT lo, rs, rd FROM t ORDER BY lo LIMIT 10",                # heavy ties: a million rows share the best key
    "SELECT g1, srt FROM t ORDER BY g1, srt DESC LIMIT 30",         # a sorted column after the first
    "SELECT * FROM t WHERE f = 5 ORDER BY rf DESC, ri LIMIT 7",
    "SELECT u FROM t ORDER BY u, u DESC LIMIT 5",
]


@pytest.mark.parametrize("sql", ORDERED)
def test_order_by(synth, sql):
    host, data, g, o = synth
    _check(g, host, data, o, sql, kernel="pg_select_topk_lds")


@pytest.mark.parametrize("k,kernel", [(KMAX - 1, "pg_select_topk_lds"), (KMAX, "pg_select_topk_lds"), (KMAX + 1, "pg_select_sort"),
                                      (50000, "pg_select_sort")])
def test_k_tiers(synth, k, kernel):
    host, data, g, o = synth
    _check(g, host, data, o, f"SELECT u, rf, g1 FROM t WHERE f < 10 ORDER BY u DESC, g1 LIMIT {k}", kernel=kernel)
    _check(g, host, data, o, f"SELECT lo, ri FROM t ORDER BY lo DESC LIMIT {k}", kernel=kernel)


def test_order_by_limit_above_matches(synth):
    host, data, g, o = synth
    M = len(_match_docs(o, host, "SELECT g1 FROM t WHERE u = 777 AND f < 12"))
    for limit in (1, M, M + 1, UNBOUNDED):
        _check(g, host, data, o, f"SELECT g1, rd FROM t WHERE u = 777 AND f < 12 ORDER BY rd DESC LIMIT {limit}")


def test_limit_zero_ignores_order_by(synth):
    host, data, g, o = synth
    rb, _ = _check(g, host, data, o, "SELECT g1, u FROM t WHERE f = 1 ORDER BY rs LIMIT 0", kernel="pg_select_empty")
    assert (rb.stats.num_docs_scanned, rb.stats.num_entries_scanned_in_filter, rb.stats.num_entries_scanned_post_filter) == (0, 0, 0)


# ---- upsert snapshot, data table, threads --------------------------------------------------------------------------------------------------
def test_upsert_snapshot(gpu_api, oracle_api):
    host, data = _synth(n=400_000, seed=3)
    g, o = NativeSegment(gpu_api, host), NativeSegment(oracle_api, host)
    valid = np.flatnonzero(np.random.default_rng(4).random(host.total_docs) < 0.4).astype(np.int32)
    g.set_queryable_doc_ids(valid)
    o.set_queryable_doc_ids(valid)
    try:
        for sql in ("SELECT g1, rs FROM t LIMIT 10", "SELECT u, rf FROM t WHERE f = 3 LIMIT 100", "SELECT u, rf FROM t ORDER BY u DESC LIMIT 10",
                    "SELECT u, rd FROM t WHERE s < 300000 ORDER BY rd LIMIT 2000"):
            _check(g, host, data, o, sql)
    finally:
        g.destroy()
        o.destroy()


@pytest.mark.parametrize("sql", ["SELECT g1, ri, rl, rf, rd, rs FROM t WHERE f = 4 LIMIT 20",
                                 "SELECT rf, u, rs FROM t ORDER BY rf DESC LIMIT 15",
                                 "SELECT * FROM t LIMIT 3"])
def test_data_table(synth, sql):
    host, data, g, o = synth
    r = g.execute_native(sql, keep_device_table=False)
    try:
        p = dt.parse_data_table_v4(r.data_table_v4())
        rb = r.block()
    finally:
        r.free()
    assert p["names"] == rb.key_columns
    assert p["types"] == [host.columns[c].data_type for c in rb.key_columns]
    norm = lambda v: "NaN" if isinstance(v, float) and math.isnan(v) else (v.item() if isinstance(v, np.generic) else v)   # noqa: E731
    want = [tuple(norm(x) for x in row) for row in rb.selection_rows]
    got = [tuple(norm(x) if not (isinstance(x, float) and x == 0.0 and math.copysign(1, x) < 0) else "-0.0" for x in row) for row in p["rows"]]
    assert got == want


def test_threads(synth):
    host, data, g, o = synth
    sqls = ["SELECT u, rs FROM t ORDER BY u DESC LIMIT 10", "SELECT g1, rf FROM t WHERE f = 1 OR s < 1000 LIMIT 10",
            "SELECT ri FROM t WHERE f IN (2, 9) ORDER BY ri LIMIT 2000", "SELECT rf, lo FROM t ORDER BY rf DESC, lo LIMIT 64"]
    want = {s: g.execute(s).selection_rows for s in sqls}
    errors = []

    def work(i):
        try:
            for r in range(4):
                s = sqls[(i + r) % len(sqls)]
                got = g.execute(parse_sql(s)).selection_rows
                if " ORDER BY " in s:   # the same keys in the same order (rows tied at the cut may differ)
                    assert len(got) == len(want[s])
                else:
                    assert got == want[s]
        except Exception as e:   # noqa: BLE001
            errors.append(e)
    ts = [threading.Thread(target=work, args=(i,)) for i in range(6)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors


# ---- refusals, merge, cancellation ---------------------------------------------------------------------------------------------------------
def _status(api, seg, sql, mutate=None):
    q = parse_sql(sql) if isinstance(sql, str) else sql
    cq = CQuery(q, tuple(seg.host.columns))
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


def test_refusals(gpu_api, synth):
    host, data, g, o = synth
    un = (capi.PG_ERR_UNSUPPORTED, capi.PG_ERR_UNSUPPORTED)
    assert _status(gpu_api, g, "SELECT srt, g1 FROM t ORDER BY srt LIMIT 5") == un            # sorted first: the linear operators
    assert _status(gpu_api, g, "SELECT srt, g1 FROM t ORDER BY srt DESC LIMIT 5") == un
    assert _status(gpu_api, g, "SELECT rs FROM t ORDER BY rs LIMIT 5") == un                  # raw STRING
    assert _status(gpu_api, g, "SELECT rl, rd FROM t ORDER BY rl, rd LIMIT 5") == un           # 128-bit key
    assert _status(gpu_api, g, "SELECT rl, g1 FROM t ORDER BY rl, g1 LIMIT 5") == un           # 64 + 7 bits
    assert _status(gpu_api, g, "SELECT g1, u FROM t ORDER BY g1, u, f, lo, s, rs, srt, ri, rf LIMIT 5") == un   # 9 ORDER BY expressions

    def expr(q):
        arr = (C.c_char_p * 1)(b"g1 + u")
        expr.keep = arr
        q.group_by_columns = arr
    assert _status(gpu_api, g, "SELECT g1 FROM t LIMIT 5", expr) == un
    assert _status(gpu_api, g, "SELECT g1 FROM t LIMIT 5", lambda q: setattr(q, "limit", -1)) == (capi.PG_ERR_INVALID_ARGUMENT,) * 2


def test_sort_budget_refusal(gpu_api, synth, gpu_knobs):
    host, data, g, o = synth
    gpu_knobs(PG_SELECT_SORT_MAX_BYTES="1048576")
    s1, s2 = _status(gpu_api, g, "SELECT u FROM t ORDER BY u LIMIT 5000")
    assert (s1, s2) == (0, capi.PG_ERR_UNSUPPORTED)   # only the execution knows the matches
    assert _status(gpu_api, g, "SELECT u FROM t ORDER BY u LIMIT 500") == (0, 0)


def test_refusals_multi_value_and_nulls(gpu_api):
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
        assert _status(gpu_api, g, "SELECT mv FROM t LIMIT 5") == un
        assert _status(gpu_api, g, "SELECT * FROM t LIMIT 5") == un
        q = parse_sql("SELECT g1, u FROM t LIMIT 5")
        q.flags |= capi.QUERY_FLAG_NULL_HANDLING
        assert _status(gpu_api, g, q) == un
        q = parse_sql("SELECT u, f FROM t ORDER BY u LIMIT 5")
        q.flags |= capi.QUERY_FLAG_NULL_HANDLING
        assert _status(gpu_api, g, q) == (0, 0)                                               # no nulls in u, f: answered
        assert _status(gpu_api, g, "SELECT g1, u FROM t LIMIT 5") == (0, 0)                    # without null handling: answered
    finally:
        g.destroy()


def test_merge_refused_and_cancel(gpu_api, synth):
    host, data, g, o = synth
    a = g.execute_native("SELECT g1 FROM t WHERE f = 1 LIMIT 5", keep_device_table=False)
    b = g.execute_native("SELECT g1 FROM t WHERE f = 2 LIMIT 5", keep_device_table=False)
    try:
        assert gpu_api.f("result_merge")(a.handle, b.handle) == capi.PG_ERR_UNSUPPORTED
    finally:
        a.free()
        b.free()
    tok = CancelToken(gpu_api)
    try:
        tok.request()
        with pytest.raises(capi.NativeError) as e:
            g.execute_native("SELECT u, g1 FROM t ORDER BY u LIMIT 100", keep_device_table=False, cancel=tok)
        assert e.value.status == capi.PG_ERR_CANCELLED
    finally:
        tok.destroy()
