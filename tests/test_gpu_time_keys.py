"""GROUP BY and SELECT DISTINCT over time-bucket transforms on the GPU path: timeConvert, toEpoch..., dateTimeConvert (EPOCH to
EPOCH) and dateTrunc as keys.

The yardstick is DESIGN 4.8's TWIN COLUMN: every test segment carries, for each text under test, a raw LONG column holding
tests/time_transform_model.py's evaluate(text) of the same data.  GROUP BY <text> on the GPU must equal GROUP BY <twin> over the same segment — on
the oracle where the oracle knows every aggregation of the query, else on the GPU path's own raw LONG keys (SUM over an expression, PERCENTILE,
DISTINCT: pinned by their own suites): the same keys as longs, the same aggregates bit for bit, the same numDocsScanned and
numEntriesScannedInFilter, and numEntriesScannedPostFilter from percentile_model.statistics over the VALUE column."""
import collections
import dataclasses
import os
import re

import numpy as np
import pytest

from oracle import po_datatable as dt
from pinot_amd import capi, formats
from pinot_amd.executor import NativeSegment
from pinot_amd.query import AggregationSpec, CQuery, QueryContext, parse_sql
from pinot_amd.segment import build_segment
from tests import expression_model as em
from tests import percentile_model as pm
from tests import test_gpu_expressions as tge
from tests import time_transform_cases as cases
from tests import time_transform_model as tm
from tests.kernel_inventory import snapshot_doc_ids

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# one doc; a partial second word; either side of the kernel's four-word iteration; either side of a 2 048-doc wave tile of the id pack
SIZES = [1, 65, 255, 257, 2047, 2049]
HOUR = "datetimeconvert(ts,'1:MILLISECONDS:EPOCH','1:HOURS:EPOCH','1:HOURS')"
QUARTER_HOUR = "datetimeconvert(tsd,'1:MILLISECONDS:EPOCH','1:MILLISECONDS:EPOCH','15:MINUTES')"
# every family; ts: raw LONG, tsd: dictionary-encoded LONG, sec: raw INT, secd: dictionary-encoded INT (uid: one day per doc)
TEXTS = [
    "toepochhours(ts)", "toepochdays(ts)", "toepochdays(uid)", "toepochdaysbucket(ts,'1000000')", "toepochminutesrounded(tsd,'5')", "toepochsecondsbucket(sec,'-30')",
    "timeconvert(ts,'MILLISECONDS','DAYS')", "timeconvert(sec,'SECONDS','MILLISECONDS')", "timeconvert(secd,'seconds','Hours')",
    HOUR, QUARTER_HOUR, "datetimeconvert(sec,'1:SECONDS:EPOCH','5:MINUTES:EPOCH','1:DAYS')", "datetimeconvert(secd,'EPOCH|SECONDS|60','EPOCH|HOURS','HOURS|6')",
    "datetrunc('second',ts)", "datetrunc('minute',tsd)", "datetrunc('hour',ts,'MILLISECONDS','+07:09')", "datetrunc('day',ts)", "datetrunc('week',ts)",
    "datetrunc('month',ts)", "datetrunc('quarter',tsd)", "datetrunc('year',ts)", "datetrunc('week',sec,'SECONDS')",
    "datetrunc('month',secd,'SECONDS','-03:30','DAYS')", "datetrunc('year',sec,'SECONDS','+13:00','MILLISECONDS')",
]
ARITHMETIC = "divide(rg,'1000')"   # an arithmetic key next to a time key: its twin is a raw DOUBLE column
NO_DICT = ["ts", "sec", "uid", "ri", "rd", "rg"]
YEAR_MS = 365 * tm.DAY_MS


def _data(n, seed=5):
    rng = np.random.default_rng(seed + n)
    # instants of about three years on either side of 1970, and of 2001: negative ones, zero, week / month / year boundaries in between
    ts = np.where(rng.integers(0, 2, n) == 0, rng.integers(-3 * YEAR_MS, 3 * YEAR_MS, n), 998449445321 + rng.integers(-2 * YEAR_MS, 2 * YEAR_MS, n)).astype(np.int64)
    ts[rng.integers(0, n, 3)] = 0
    ts[rng.integers(0, n, 3)] = -1
    pool = np.concatenate([rng.integers(-2 * YEAR_MS, 2 * YEAR_MS, 20), 998449445321 + rng.integers(-YEAR_MS, YEAR_MS, 20), [0, -1, -900_000, 900_000]]).astype(np.int64)
    sec = np.where(rng.integers(0, 2, n) == 0, rng.integers(-90_000_000, 90_000_000, n), 998449445 + rng.integers(-40_000_000, 40_000_000, n)).astype(np.int32)
    sec[rng.integers(0, n, 2)] = 0
    data = {
        "ts": ts, "tsd": rng.choice(pool, n), "sec": sec, "secd": rng.choice((pool[:30] // 1000).astype(np.int32), n),
        "uid": ((np.arange(n, dtype=np.int64) - n // 2) * 3 * tm.DAY_MS + 12_345),
        "g7": rng.integers(0, 7, n).astype(np.int32), "g3": rng.integers(0, 3, n).astype(np.int32), "s": rng.integers(0, 1000, n).astype(np.int32),
        "c_inv1": rng.integers(0, 8, n).astype(np.int32), "ri": rng.integers(-1000, 1000, n).astype(np.int32), "rd": rng.uniform(-1e3, 1e3, n),
        "rg": (rng.integers(0, 50, n) * 1000 - 7).astype(np.int32), "di": rng.integers(-500, 500, n).astype(np.int32),
    }
    schema = {k: "INT" for k in data}
    schema.update(ts="LONG", tsd="LONG", uid="LONG", rd="DOUBLE")
    twins = {}
    for i, text in enumerate(TEXTS):
        twins[text] = "k%d" % i
        data["k%d" % i] = np.array(tm.evaluate(text, data[tm.columns_of(text)[0]]), dtype=np.int64)
        schema["k%d" % i] = "LONG"
    twins[ARITHMETIC] = "kx"
    with np.errstate(all="ignore"):
        data["kx"] = np.asarray(em.evaluate(ARITHMETIC, data, schema), dtype=np.float64)
    schema["kx"] = "DOUBLE"
    host = build_segment("timekey_%d" % n, data, schema, inverted_index_columns=["c_inv1"], no_dictionary_columns=NO_DICT + list(twins.values()))
    return host, data, schema, twins


_SEGMENTS = {}


@pytest.fixture(scope="module")
def segments(gpu_api, oracle_api):
    def get(n):
        if n not in _SEGMENTS:
            host, data, schema, twins = _data(n)
            _SEGMENTS[n] = (host, data, schema, twins, NativeSegment(gpu_api, host), NativeSegment(oracle_api, host))
        return _SEGMENTS[n]
    yield get
    for s in _SEGMENTS.values():
        s[4].destroy()
        s[5].destroy()
    _SEGMENTS.clear()


def _key(c):
    return ("d", float(c)) if isinstance(c, (float, np.floating)) else int(c) if isinstance(c, (int, np.integer)) else c


def _key_rows(b):
    """[(key tuple, results)] in result order; LONG keys as Python ints"""
    cols = b.columns
    return [(tuple(_key(c) for c in k), [c[i] for c in cols]) for i, k in enumerate(b.group_keys)]


def _same_value(a, b):
    if isinstance(a, tuple) and len(a) == 2 and isinstance(a[0], np.ndarray):   # PERCENTILE: (values, counts) runs
        return pm.same_runs(a, b)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same_value(x, y) for x, y in zip(a, b))
    if isinstance(a, float):
        return pm.same_double(a, b)
    return a == b


def _twin_query(qc, twins):
    name = lambda g: twins.get(g, g)   # noqa: E731
    return dataclasses.replace(qc, group_by=[name(g) for g in qc.group_by], distinct=[name(g) for g in qc.distinct],
                               select_columns=[name(g) for g in qc.select_columns], order_by=[(name(text), asc) for text, asc in qc.order_by])


def _operands(text):
    return tm.columns_of(text) if text in TEXTS else em.columns_of(text)


def _columns_read(qc):
    read = set()
    for g in qc.group_by or qc.distinct:
        read |= set(_operands(g)) if "(" in g else {g}
    for a in qc.aggregations:
        if "(" in (a.column or ""):
            read |= set(em.columns_of(a.column))
        elif a.column:
            read.add(a.column)
    return read


def _check(seg, sql, reference="oracle", ordered=False, **params):
    """`sql` with time keys on the GPU against its twin (the same query over the twin columns) on `reference`"""
    host, data, schema, twins, gpu, oracle = seg
    qc = sql if isinstance(sql, QueryContext) else parse_sql(sql)
    for k, v in params.items():
        setattr(qc, k, v)
    assert any(g in TEXTS for g in qc.group_by), (sql, qc.group_by)
    assert all(g in twins for g in qc.group_by if "(" in g), (sql, qc.group_by)
    b = gpu.execute(qc)
    w = (oracle if reference == "oracle" else gpu).execute(_twin_query(qc, twins))
    got, want = _key_rows(b), _key_rows(w)
    assert len({k for k, _ in got}) == len(got), sql
    for j, g in enumerate(qc.group_by):
        if g in TEXTS:
            assert all(isinstance(k[j], int) for k, _ in got), (sql, g)       # LONG values, not doubles
    if ordered:
        assert [k for k, _ in got] == [k for k, _ in want], sql
    assert {k for k, _ in got} == {k for k, _ in want}, sql
    wd = dict(want)
    for k, r in got:
        assert _same_value(r, wd[k]), (sql, k, r, wd[k])
    assert b.stats.num_docs_scanned == w.stats.num_docs_scanned, sql
    assert b.stats.num_entries_scanned_in_filter == w.stats.num_entries_scanned_in_filter and b.stats.stats_exact == w.stats.stats_exact == 1, sql
    assert (b.stats.num_docs_scanned, b.stats.num_entries_scanned_post_filter) == pm.statistics(w.stats.num_docs_scanned, _columns_read(qc)), sql
    assert b.stats.star_tree_index == -1 and b.stats.num_total_docs == host.total_docs
    assert b.stats.num_groups_limit_reached == w.stats.num_groups_limit_reached, sql
    return b, w


# ---- every family, every kind of value column ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_every_text_as_a_key(segments, n):
    seg = segments(n)
    for text in TEXTS:
        b, _ = _check(seg, f"SELECT {text}, COUNT(*), SUM(s), MAX(ri) FROM t GROUP BY {text}")
        # ... and the keys are the model's values of the data
        assert {k[0] for k, _ in _key_rows(b)} == set(tm.evaluate(text, seg[1][tm.columns_of(text)[0]])), text


@pytest.mark.parametrize("n", SIZES)
def test_one_bucket_and_one_bucket_per_doc(segments, n):
    seg = segments(n)
    b, _ = _check(seg, "SELECT toepochdaysbucket(ts,'1000000'), COUNT(*), SUM(s) FROM t GROUP BY toepochdaysbucket(ts,'1000000')")
    assert [k for k, _ in _key_rows(b)] == [(0,)] and b.columns[0][0] == n
    b, _ = _check(seg, "SELECT toepochdays(uid), COUNT(*), SUM(s) FROM t GROUP BY toepochdays(uid)")
    assert len(b.group_keys) == n          # as many distinct values as docs: beyond the dense tables


@pytest.mark.parametrize("n", SIZES)
def test_key_shapes(segments, n):
    seg = segments(n)
    # behind a filter; next to a plain dictionary key, a plain raw key, an arithmetic key and another time key
    _check(seg, "SELECT dateTrunc('day', ts), COUNT(*), SUM(s), MIN(di), AVG(s) FROM t WHERE s < 700 GROUP BY dateTrunc('day', ts)")
    _check(seg, "SELECT g7, toEpochHours(ts), COUNT(*), MAX(ri) FROM t WHERE c_inv1 IN (1, 5) GROUP BY g7, toEpochHours(ts)")
    _check(seg, "SELECT DATE_TRUNC('month', ts), rg, COUNT(*), MINMAXRANGE(di) FROM t GROUP BY DATE_TRUNC('month', ts), rg")
    _check(seg, "SELECT toEpochHours(ts), rg / 1000, COUNT(*), SUM(s) FROM t WHERE s BETWEEN 100 AND 900 GROUP BY toEpochHours(ts), rg / 1000")
    _check(seg, "SELECT dateTrunc('week', ts), dateTrunc('quarter', tsd), g3, COUNT(*) FROM t GROUP BY dateTrunc('week', ts), dateTrunc('quarter', tsd), g3")
    _check(seg, "SELECT dateTrunc('year', ts), ts, COUNT(*) FROM t GROUP BY dateTrunc('year', ts), ts")     # the value column a plain key as well: counted once
    # behind an expression predicate (the oracle has no such leaf: the twin runs on the GPU path as well)
    _check(seg, f"SELECT {HOUR}, g3, COUNT(*), SUM(s) FROM t WHERE ri * rd > 0 AND s < 900 GROUP BY {HOUR}, g3", reference="gpu")


@pytest.mark.parametrize("n", SIZES)
def test_next_to_sum_of_an_expression_and_a_percentile(segments, n):
    seg = segments(n)
    _check(seg, "SELECT dateTrunc('month', ts), SUM(ri * rd), COUNT(*) FROM t WHERE s < 800 GROUP BY dateTrunc('month', ts)", reference="gpu")
    b, _ = _check(seg, "SELECT dateTrunc('week', ts), g3, PERCENTILE(di, 95), COUNT(*), MAX(s) FROM t GROUP BY dateTrunc('week', ts), g3", reference="gpu")
    assert b.stats.percentile_passes == 1
    _check(seg, f"SELECT {QUARTER_HOUR}, SUM(add(di,s)), PERCENTILE(rd, 50) FROM t WHERE s >= 50 GROUP BY {QUARTER_HOUR}", reference="gpu")


def test_negative_and_zero_instants(segments):
    """truncation toward zero in the epoch functions, a true floor in dateTrunc: -1 ms is day 0 to toEpochDays and 1969-12-31 to dateTrunc"""
    seg = segments(2049)
    ts = seg[1]["ts"]
    assert (ts < 0).sum() > 100 and (ts == 0).sum() >= 1 and (ts == -1).sum() >= 1
    near = ts[(ts >= -tm.DAY_MS) & (ts < tm.DAY_MS)]
    assert (near < 0).any() and (near >= 0).any()
    b, _ = _check(seg, "SELECT toEpochDays(ts), COUNT(*) FROM t WHERE ts BETWEEN -86400000 AND 86399999 GROUP BY toEpochDays(ts)")
    assert dict(_key_rows(b)) == {(k,): [c] for k, c in collections.Counter(-1 if x == -tm.DAY_MS else 0 for x in near.tolist()).items()}
    b, _ = _check(seg, "SELECT dateTrunc('day', ts), COUNT(*) FROM t WHERE ts BETWEEN -86400000 AND 86399999 GROUP BY dateTrunc('day', ts)")
    assert dict(_key_rows(b)) == {(-tm.DAY_MS,): [int((near < 0).sum())], (0,): [int((near >= 0).sum())]}


@pytest.mark.parametrize("n", [257, 2049])
def test_order_by_the_key_and_segment_trim(segments, n):
    seg = segments(n)
    # (every ORDER BY names all the keys: which of two groups that tie survives a trim is not pinned)
    for tail in ("ORDER BY dateTrunc('month', ts), g3 LIMIT 2", "ORDER BY datetrunc('month',ts) DESC, g3 DESC LIMIT 1", "ORDER BY g3 DESC, DATE_TRUNC( 'month', ts ) LIMIT 1"):
        for mst in (1, 7):
            qc = parse_sql("SELECT dateTrunc('month', ts), g3, COUNT(*), SUM(s) FROM t WHERE s < 900 GROUP BY dateTrunc('month', ts), g3 " + tail)
            assert qc.resolved_order_by() is not None
            b, w = _check(seg, qc, ordered=False, min_segment_group_trim_size=mst)
            assert len(b.group_keys) == len(w.group_keys) == min(max(5 * qc.limit, mst), len(w.group_keys))


def test_num_groups_limit(segments):
    seg = segments(2049)
    for sql in ("SELECT toEpochDays(uid), COUNT(*) FROM t GROUP BY toEpochDays(uid)", "SELECT toEpochHours(ts), g7, COUNT(*), SUM(s) FROM t WHERE s < 900 GROUP BY toEpochHours(ts), g7"):
        b, _ = _check(seg, sql, num_groups_limit=13)
        assert len(b.group_keys) == 13 and b.stats.num_groups_limit_reached == 1


def test_upsert_snapshot(gpu_api, oracle_api):
    host, data, schema, twins = _data(2049, seed=9)
    g, o = NativeSegment(gpu_api, host), NativeSegment(oracle_api, host)
    keep = snapshot_doc_ids(host.total_docs)
    g.set_queryable_doc_ids(keep)
    o.set_queryable_doc_ids(keep)
    try:
        seg = (host, data, schema, twins, g, o)
        b, _ = _check(seg, "SELECT dateTrunc('week', ts), COUNT(*), SUM(s) FROM t GROUP BY dateTrunc('week', ts)")
        assert b.stats.num_docs_scanned == len(keep)
        _check(seg, "SELECT toEpochHours(ts), g7, COUNT(*) FROM t WHERE s < 600 GROUP BY toEpochHours(ts), g7")
    finally:
        g.destroy()
        o.destroy()


# ---- DISTINCT -------------------------------------------------------------------------------------------------------------------------------------
def _distinct_rows(b):
    return [tuple(_key(c) for c in k) for k in b.distinct_rows]


@pytest.mark.parametrize("n", SIZES)
def test_distinct(segments, n):
    """SELECT DISTINCT <time key>, col and its GROUP-BY-without-aggregations spelling against the DISTINCT twin, ordered and in docId order"""
    host, data, schema, twins, gpu, oracle = segments(n)
    for where, tail in ((" WHERE s < 800", " ORDER BY g3 DESC, dateTrunc('month', ts) LIMIT 10"), ("", " ORDER BY dateTrunc('month', ts) DESC, g3 LIMIT 4"),
                        (" WHERE s < 800", " LIMIT 7"), ("", " LIMIT 100000")):
        qd = parse_sql("SELECT DISTINCT dateTrunc('month', ts), g3 FROM t" + where + tail)
        qg = parse_sql("SELECT dateTrunc('month', ts), g3 FROM t" + where + " GROUP BY dateTrunc('month', ts), g3" + tail)
        assert qg.has_group_by and qg.group_by == qd.distinct == ["datetrunc('month',ts)", "g3"] and not qg.aggregations
        qg.distinct, qg.group_by = qg.group_by, []       # the broker's rewrite of a GROUP BY without aggregations
        want = gpu.execute(_twin_query(qd, twins))
        for q in (qd, qg):
            b = gpu.execute(q)
            assert _distinct_rows(b) == _distinct_rows(want), tail
            assert all(isinstance(r[0], int) for r in _distinct_rows(b))
            assert b.stats.num_docs_scanned == want.stats.num_docs_scanned and b.stats.num_entries_scanned_in_filter == want.stats.num_entries_scanned_in_filter
            assert b.stats.num_entries_scanned_post_filter == b.stats.num_docs_scanned * len({"ts", "g3"})
    # an unbounded DISTINCT is the oracle's key set over the twin
    b = gpu.execute(f"SELECT DISTINCT toEpochHours(ts), {QUARTER_HOUR} FROM t LIMIT 100000")
    w = oracle.execute(_twin_query(parse_sql(f"SELECT toEpochHours(ts), {QUARTER_HOUR}, COUNT(*) FROM t GROUP BY toEpochHours(ts), {QUARTER_HOUR}"), twins))
    assert sorted(_distinct_rows(b)) == sorted(k for k, _ in _key_rows(w))
    assert b.stats.num_entries_scanned_post_filter == b.stats.num_docs_scanned * 2


# ---- results --------------------------------------------------------------------------------------------------------------------------------------
def test_data_table_names_and_types(segments):
    host, data, schema, twins, gpu, oracle = segments(2047)
    r = gpu.execute_native("SELECT DATE_TRUNC('day', ts), g3, toEpochMinutesRounded(tsd, 5), rg / 1000, COUNT(*) FROM t WHERE s < 500 "
                           "GROUP BY DATE_TRUNC('day', ts), g3, toEpochMinutesRounded(tsd, 5), rg / 1000", keep_device_table=False)
    t = dt.parse_data_table_v4(r.data_table_v4())
    rows = r.block().rows()
    r.free()
    assert t["names"] == ["datetrunc('day',ts)", "g3", "toepochminutesrounded(tsd,'5')", "divide(rg,'1000')", "count(*)"]
    assert t["types"] == ["LONG", "INT", "LONG", "DOUBLE", "LONG"] and len(t["rows"]) == len(rows) > 3
    for a, g3, c, d, count in t["rows"]:
        assert isinstance(a, int) and isinstance(c, int) and isinstance(d, float) and rows[(a, g3, c, d)] == [count]
        assert a % tm.DAY_MS == 0 and c % 5 == 0
    r = gpu.execute_native("SELECT DISTINCT timeConvert(ts,'MILLISECONDS','DAYS'), g3 FROM t ORDER BY timeConvert(ts,'MILLISECONDS','DAYS') LIMIT 3", keep_device_table=False)
    t = dt.parse_data_table_v4(r.data_table_v4())
    r.free()
    assert t["names"] == ["timeconvert(ts,'MILLISECONDS','DAYS')", "g3"] and t["types"] == ["LONG", "INT"] and len(t["rows"]) == 3
    assert [row[0] for row in t["rows"]] == sorted(row[0] for row in t["rows"]) and t["rows"][0][0] == min(tm.evaluate("timeconvert(ts,'MILLISECONDS','DAYS')", data["ts"]))


def test_merge_of_two_results(segments):
    """pg_result_merge treats a result keyed by a time key as one keyed by a raw LONG column of the same values that is grouped through its
    virtual dictionary (a raw column among several keys): merged alike, or refused alike.  (A LONE raw LONG column takes the hash route over
    its raw values, which a derived column, having none, never does: a lone time key is checked against itself.)"""
    host, data, schema, twins, gpu, oracle = segments(2047)

    def merged_twice(q):
        a = b = None
        try:
            a, b = gpu.execute_native(q), gpu.execute_native(q)
            a.merge(b)
            return ("merged", _key_rows(a.block()))
        except capi.NativeError as e:
            return ("refused", e.status)
        finally:
            for r in (a, b):
                if r is not None:
                    r.free()

    for sql in ("SELECT dateTrunc('month', ts), g7, COUNT(*), SUM(s) FROM t WHERE s < 800 GROUP BY dateTrunc('month', ts), g7",
                "SELECT toEpochHours(ts), g3, COUNT(*), MAX(ri) FROM t GROUP BY toEpochHours(ts), g3"):
        qc = parse_sql(sql)
        outcomes = [merged_twice(q) for q in (qc, _twin_query(qc, twins))]
        assert outcomes[0][0] == outcomes[1][0], (sql, outcomes)
        if outcomes[0][0] == "merged":
            once = dict(_key_rows(gpu.execute(qc)))
            assert dict(outcomes[0][1]).keys() == dict(outcomes[1][1]).keys() == once.keys()
            for k, r in outcomes[0][1]:
                assert _same_value(r, dict(outcomes[1][1])[k]) and r[0] == 2 * once[k][0], (sql, k)
        else:
            assert outcomes[0][1] == outcomes[1][1], (sql, outcomes)
    # a lone time key: a dense table over its virtual dictionary's ids, which merges element-wise
    qc = parse_sql("SELECT dateTrunc('month', ts), COUNT(*), SUM(s) FROM t WHERE s < 800 GROUP BY dateTrunc('month', ts)")
    kind, rows = merged_twice(qc)
    once = dict(_key_rows(gpu.execute(qc)))
    assert kind == "merged" and dict(rows).keys() == once.keys()
    assert all(r == [2 * once[k][0], 2 * once[k][1]] for k, r in rows)


def test_second_call_builds_nothing(gpu_api, segments):
    host, data, schema, twins, _, oracle = segments(2047)
    gpu = NativeSegment(gpu_api, host)
    try:
        before = gpu.device_bytes()
        first = gpu.execute("SELECT dateTrunc('day', ts), COUNT(*), SUM(s) FROM t GROUP BY dateTrunc('day', ts)")
        built = gpu.device_bytes() - before
        assert built > 0                                   # the bit-packed ids of the derived column
        again = gpu.execute("SELECT DATE_TRUNC('day', ts), COUNT(*), SUM(s) FROM t GROUP BY DATE_TRUNC('day', ts)")
        gpu.execute("SELECT DISTINCT dateTrunc('day', ts) FROM t LIMIT 5")
        gpu_api.call("query_supported", gpu.handle, CQuery(parse_sql("SELECT dateTrunc('day', ts), MAX(s) FROM t GROUP BY dateTrunc('day', ts)")).ptr())
        assert gpu.device_bytes() - before == built        # one text, one column: nothing was built again
        assert dict(_key_rows(first)) == dict(_key_rows(again))
        gpu.execute("SELECT dateTrunc('day', ts, 'MILLISECONDS'), COUNT(*) FROM t GROUP BY dateTrunc('day', ts, 'MILLISECONDS')")   # another text: another column
        assert gpu.device_bytes() - before == 2 * built
    finally:
        gpu.destroy()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------
def _keys(*texts, **kw):
    return QueryContext(group_by=list(texts), aggregations=[AggregationSpec("COUNT")], has_group_by=True, **kw)


def test_refusals(gpu_api):
    from pinot_amd.segment import build_column, build_mv_column
    host, data, schema, twins = _data(2047, seed=3)
    rng = np.random.default_rng(1)
    n = host.total_docs
    host.columns["by"] = build_column("by", [b"ab%d" % (i % 5) for i in range(n)], "BYTES", dictionary=False)
    host.columns["txt"] = build_column("txt", ["t%d" % (i % 5) for i in range(n)], "STRING")
    host.columns["rf"] = build_column("rf", rng.uniform(0, 1e6, n).astype(np.float32), "FLOAT", dictionary=False)
    host.columns["mv"] = build_mv_column("mv", [list(rng.integers(0, 20, rng.integers(1, 4))) for _ in range(n)], "INT")
    host.columns["tsd"].null_vector = np.frombuffer(formats.serialize_roaring(np.array([3, 77, 2000], dtype=np.int64)), dtype=np.uint8)
    seg = NativeSegment(gpu_api, host)
    refused = lambda qc, status, text: tge._refused(gpu_api, seg, qc, status, text)   # noqa: E731: through pg_query_supported and pg_query_exec
    try:
        U, I, N = capi.PG_ERR_UNSUPPORTED, capi.PG_ERR_INVALID_ARGUMENT, capi.PG_ERR_NOT_FOUND
        # by the text alone: every case of the parser's list, as a GROUP BY key and (one of each status) as a DISTINCT column
        for text, status, piece in cases.REFUSED:
            refused(_keys(text), status, piece)
        for text, status, piece in (cases.REFUSED[0], cases.REFUSED[-1]):
            refused(QueryContext(distinct=[text], flags=capi.QUERY_FLAG_DISTINCT), status, piece)
        # by the value column
        refused(_keys("toepochhours(rd)"), U, "time function over the DOUBLE column rd")
        refused(_keys("datetrunc('day',rf)"), U, "time function over the FLOAT column rf")
        refused(_keys("timeconvert(txt,'SECONDS','DAYS')"), U, "time function over the STRING column txt")
        refused(_keys(HOUR.replace("(ts,", "(by,")), U, "time function over the BYTES column by")
        refused(_keys("datetrunc('day',mv)"), U, "time function over the multi-value column mv")
        refused(_keys("datetrunc('day',nosuch)"), N, "column not found: nosuch")
        refused(QueryContext(distinct=["toepochdays(nosuch)"], flags=capi.QUERY_FLAG_DISTINCT), N, "column not found: nosuch")
        # a time function nested inside arithmetic, and the functions that stay refused everywhere: the arithmetic parser's texts
        refused(_keys("add(datetrunc('day',ts),'1')"), U, "the function datetrunc")
        refused(_keys("mult(toepochhours(ts),'2')"), U, "the function toepochhours")
        refused(_keys("mod(ts,'3')"), U, "the function mod")
        refused(_keys("abs(ts)"), U, "the function abs")
        # null handling, multi-value neighbours, the limit of four expression keys (both kinds counted)
        for q in (_keys("datetrunc('quarter',tsd)"), parse_sql("SELECT DISTINCT toEpochMinutesRounded(tsd, 5) FROM t")):
            q.flags |= capi.QUERY_FLAG_NULL_HANDLING
            refused(q, U, "expression over tsd, which holds nulls")
        q = _keys("datetrunc('day',ts)", "g7")                   # columns without nulls run under the flag
        q.flags |= capi.QUERY_FLAG_NULL_HANDLING
        assert len(seg.execute(q).rows()) > 7
        assert len(seg.execute(_keys("datetrunc('quarter',tsd)")).rows()) > 3   # ... and the column with nulls without it
        refused(_keys("datetrunc('day',ts)", "mv"), U, "multi-value group-by column mv next to the expression key datetrunc('day',ts)")
        refused(parse_sql("SELECT DISTINCT toEpochHours(ts), mv FROM t"), U, "multi-value group-by column mv next to the expression key")
        refused(_keys("toepochhours(ts)", "toepochdays(ts)", "add(ri,'1')", "datetrunc('day',ts)", "add(ri,'2')"), U, "more than 4 expressions among the group-by / DISTINCT keys")
        assert len(seg.execute(_keys("toepochdays(ts)", "add(g3,'1')", "datetrunc('year',ts)", "add(g3,'2')")).rows()) > 3
        # in WHERE, inside an aggregation and in a selection a time function stays with the Java plan, with the texts of before
        refused(parse_sql("SELECT COUNT(*) FROM t WHERE toEpochHours(ts) > 5"), U, "the function toepochhours")
        refused(parse_sql("SELECT g3, SUM(dateTrunc('day', ts)) FROM t GROUP BY g3"), U, "the function datetrunc")
        q = parse_sql("SELECT dateTrunc('day', ts), g7 FROM t LIMIT 5")
        assert q.flags & capi.QUERY_FLAG_SELECTION
        refused(q, U, "selection of the expression datetrunc('day',ts)")
        refused(parse_sql("SELECT g7 FROM t ORDER BY toEpochHours(ts) LIMIT 5"), U, "selection of the expression toepochhours(ts)")
    finally:
        seg.destroy()


def test_key_kernel_uses_no_scratch_and_no_lds():
    """the build leaves hipcc's kernel-resource-usage remarks of pg_kernels_timekey.hip behind: pg_time_keys may not spill, and uses no LDS"""
    log = os.path.join(ROOT, "pinot_amd", "csrc", "pg_kernels_timekey.resources.log")
    if not os.path.exists(log):
        pytest.skip("library was built without the resource log")
    usage, cur = {}, None
    for line in open(log):
        m = re.search(r"Function Name: (\w+)", line)
        if m:
            cur = m.group(1)
        m = re.search(r"(ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and cur:
            usage[(cur, m.group(1)[:3])] = int(m.group(2))
    assert usage.get(("pg_time_keys", "Scr")) == 0 and usage.get(("pg_time_keys", "LDS")) == 0, usage
