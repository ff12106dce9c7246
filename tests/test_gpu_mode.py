"""MODE on the GPU path (PG_AGG_MODE) against tests/mode_model.py over the ORACLE's match set and group assignment: every map bit for bit
the model's — keys exact in the column's stored type —, every final value (PG_QUERY_FLAG_FINAL_MODE) the model's under the defined tie and
AVG rules, the statistics from the model and the oracle's filter.  MODE runs on PERCENTILE's counting path: the tiers, their knobs and the
reported kernel names are pg_pctl_lds / pg_pctl_hbm / pg_pctl_sort."""
import math
import os
import re

import numpy as np
import pytest

from oracle import po_datatable as dt
from pinot_amd import capi, formats
from pinot_amd.executor import Comm, GroupByCombineOperator, NativeSegment, extract_final, mode_merge
from pinot_amd.query import CQuery, parse_sql
from pinot_amd.segment import build_column, build_segment
from tests import mode_model as mm
from tests import percentile_model as pm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DICT_COLS, RAW_COLS = ("xi", "xl", "xf", "xd"), ("ri", "rl", "rf", "rd")
TYPE_OF = {"xi": "INT", "ri": "INT", "xl": "LONG", "rl": "LONG", "xf": "FLOAT", "rf": "FLOAT", "xd": "DOUBLE", "rd": "DOUBLE"}
BIG = 2**53
SPECIAL = [0.0, -0.0, math.inf, -math.inf, 0.1, 2.5, -7.25, 1e30]   # each several times; one NaN, which never ties at the top


def _floats(n, rng, both_zeros=True):
    """(a dictionary built by pinot_amd.segment holds one zero: -0.0 == 0.0 there; the raw columns carry both)"""
    v = np.array([SPECIAL[i] for i in rng.integers(0, len(SPECIAL), n)])
    if not both_zeros:
        v[v == 0.0] = 0.0
    v[: max(1, n // 3)] = 2.5       # 2.5 is the mode
    if n > 8:
        v[n // 2] = math.nan
    return v


def _ties(n, values, per):
    """i % 1000, with the first per x len(values) docs cycling over `values`: those tie at the greatest count"""
    a = np.arange(n) % 1000
    k = min(n, per * len(values))
    a[:k] = np.array(values)[np.arange(k) % len(values)]
    return a.astype(np.int32)


def _data(n, seed=41):
    rng = np.random.default_rng(seed + n)
    longs = np.array([BIG + 1, BIG + 2, BIG + 3, -BIG - 1, 5, -5])
    t65 = np.where(np.arange(n) < 65 * 31, np.arange(n) % 65, 1000 + np.arange(n))
    data = {
        "g7": rng.integers(0, 7, n).astype(np.int32), "g2": (np.arange(n) % 2).astype(np.int32), "g20": rng.integers(0, 20, n).astype(np.int32),
        "s": rng.integers(0, 1000, n).astype(np.int32),
        "xi": rng.integers(-20, 21, n).astype(np.int32), "ri": (rng.integers(-2**31, 2**31 - 1, n, dtype=np.int64) // 200_000_000).astype(np.int32),
        "xl": longs[rng.integers(0, len(longs), n)].astype(np.int64), "rl": longs[rng.integers(0, 3, n)].astype(np.int64),
        "xf": _floats(n, rng, False).astype(np.float32), "rf": _floats(n, rng).astype(np.float32), "xd": _floats(n, rng, False), "rd": _floats(n, rng),
        "t2": _ties(n, [7, 777], 100), "t3": _ties(n, [5, 500, 900], 100), "t65": t65.astype(np.int32),
        "distinct": rng.permutation(n).astype(np.int32), "one": np.full(n, 42, dtype=np.int32),
        "half": np.where(np.arange(n) % 2 == 0, 0.5, 0.25), "third": np.array([(0.1, 0.2, 0.3)[i % 3] for i in range(n)]),   # an exact and an inexact AVG sum
        "u1": rng.permutation(n).astype(np.int32), "u2": rng.permutation(n).astype(np.int32), "u3": rng.permutation(n).astype(np.int32),
        "txt": np.array(["t%d" % v for v in rng.integers(0, 5, n)], dtype=object).tolist(),
    }
    schema = {k: "INT" for k in data}
    schema.update(TYPE_OF)
    schema.update(txt="STRING", half="DOUBLE", third="DOUBLE")
    return build_segment("mode_%d" % n, data, schema, no_dictionary_columns=list(RAW_COLS) + ["third"]), data, schema


def _wide(n=8200):
    data = {"w64": np.arange(n) % 64, "w65": np.arange(n) % 65, "w1025": np.arange(n) % 1025, "w4097": np.arange(n) % 4097,
            "far": np.where(np.arange(n) % 4 == 0, 3, np.where(np.arange(n) % 4 == 1, 9_000_000, 5000 + np.arange(n))), "s": np.arange(n) % 1000}
    data = {k: v.astype(np.int32) for k, v in data.items()}
    return build_segment("mode_wide", data, {k: "INT" for k in data}), data, {k: "INT" for k in data}


_SEGMENTS = {}
_MAPS = {}


@pytest.fixture(scope="module")
def segments(gpu_api, oracle_api):
    def get(n):
        if n not in _SEGMENTS:
            host, data, schema = _wide() if n == "wide" else _data(n)
            _SEGMENTS[n] = (host, data, schema, NativeSegment(gpu_api, host), NativeSegment(oracle_api, host))
        return _SEGMENTS[n]
    yield get
    for _, _, _, g, o in _SEGMENTS.values():
        g.destroy()
        o.destroy()
    _SEGMENTS.clear()
    _MAPS.clear()


def _filter(oracle, sql):
    where = sql.split(" FROM ", 1)[1].split(" GROUP BY ")[0].split(" ORDER BY ")[0].split(" LIMIT ")[0]
    ds = oracle.filter("SELECT COUNT(*) FROM " + where)
    docs, st = ds.doc_ids(), ds.stats()
    ds.free()
    return docs, st.num_entries_scanned_in_filter


def _norm(key):
    return tuple(float(k) if isinstance(k, (int, float, np.integer, np.floating)) else k for k in key)


def _column_of(spec):
    return spec.column.split(",")[0]


def _reducer_of(spec):
    return mm.parse_arguments(spec.column)[1]


def _check(seg, sql, kernel=None):
    """Runs `sql` twice — intermediate and PG_QUERY_FLAG_FINAL_MODE — and holds every MODE and COUNT(*) of it, its groups and its statistics
    to the model; returns the intermediate block."""
    host, data, schema, gpu, oracle = seg
    qc = parse_sql(sql)
    docs, in_filter = _filter(oracle, sql)
    groups = pm.group_docs([np.asarray(data[g]) for g in qc.group_by], docs) if qc.group_by else {(): np.asarray(docs, dtype=np.int64)}
    groups = {_norm(k): v for k, v in groups.items()}
    b = gpu.execute(qc)
    qf = parse_sql(sql)
    qf.flags = qc.flags
    qf.flags |= capi.QUERY_FLAG_FINAL_MODE
    f = gpu.execute(qf)
    rows, finals = {_norm(k): v for k, v in b.rows().items()}, {_norm(k): v for k, v in f.rows().items()}
    assert set(rows) == set(groups) and set(finals) == set(groups), sql
    read = set(qc.group_by)
    for a in qc.aggregations:
        if a.function == "MODE":
            read.add(_column_of(a))
        elif a.column:
            read |= {a.column} if a.column in data else set(re.findall(r"[A-Za-z_]\w*", a.column.split(",'")[0])) & set(data)
    for blk in (b, f):
        assert (blk.stats.num_docs_scanned, blk.stats.num_entries_scanned_post_filter) == pm.statistics(len(docs), read), sql
        assert blk.stats.num_entries_scanned_in_filter == in_filter and blk.stats.stats_exact == 1 and blk.stats.num_total_docs == host.total_docs, sql
        assert blk.stats.star_tree_index == -1
        if kernel is not None:
            assert blk.stats.kernel.decode() == kernel, sql
    for key, gdocs in groups.items():
        for a, spec in enumerate(qc.aggregations):
            if spec.function == "COUNT":
                assert rows[key][a] == len(gdocs) == finals[key][a], (sql, key)
            if spec.function != "MODE":
                continue
            col = _column_of(spec)
            want = mm.value_map(np.asarray(data[col])[gdocs], schema[col])
            got = rows[key][a]
            assert mm.same_map(got, want), (sql, key, spec.column, got[1][:6], want[1][:6])
            want_final = mm.final(want, _reducer_of(spec))
            assert mm.same_double(finals[key][a], want_final), (sql, key, spec.column, finals[key][a], want_final)
            assert mm.same_double(extract_final("MODE", got, spec.column), want_final)
    return b


# ---- the first case: fails on a tree without the feature with a SqlError --------------------------------------------------------------------------
def test_mode_of_a_raw_double_column(segments):
    b = _check(segments(257), "SELECT MODE(rd) FROM t", kernel="pg_pctl_lds")
    assert b.aggregation_result()[0][0] == "DOUBLE" and extract_final("MODE", b.aggregation_result()[0], "rd") == 2.5


# ---- doc counts, layouts, filters, group shapes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 2047, 2049])
def test_doc_counts_and_column_layouts(segments, n):
    """INT / LONG / FLOAT / DOUBLE arguments, dictionary-encoded and raw (a LONG beyond 2^53 with its key exact, -0.0 / 0.0, +-Inf, a NaN that
    is not tied); no filter, a range filter and a filter matching nothing; no GROUP BY, one and two group columns; the three reducers"""
    seg = segments(n)
    for i, col in enumerate(DICT_COLS + RAW_COLS):
        red = ("", ", 'MIN'", ", 'MAX'", ", 'AVG'")[i % 4]
        _check(seg, f"SELECT MODE({col}{red}), COUNT(*) FROM t")
        _check(seg, f"SELECT MODE({col}, 'AVG'), MODE({col}, 'MAX'), MODE({col}) FROM t WHERE s < 500")
        _check(seg, f"SELECT MODE({col}{red}) FROM t WHERE s > 5000")                                  # no doc: an empty map, -Infinity
        _check(seg, f"SELECT g7, MODE({col}{red}) FROM t WHERE s BETWEEN 100 AND 800 GROUP BY g7")
        _check(seg, f"SELECT g7, g2, MODE({col}, 'MAX'), MODE({col}, 'AVG') FROM t GROUP BY g7, g2")
    if n >= 65:
        host, data, schema, gpu, _ = seg
        m = gpu.execute("SELECT MODE(xl) FROM t").aggregation_result()[0]
        assert m[0] == "LONG" and {BIG + 1, BIG + 2, BIG + 3} <= {k for k, _ in m[1]} and all(type(k) is int for k, _ in m[1])   # no key through a double
        m = gpu.execute("SELECT MODE(rd) FROM t").aggregation_result()[0]
        assert [math.copysign(1.0, k) for k, _ in m[1] if k == 0.0] == [-1.0, 1.0] and sum(1 for k, _ in m[1] if k != k) == (1 if n > 8 else 0)


# ---- constructed ties -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [None, 64])
@pytest.mark.parametrize("col", ["t2", "t3", "t65", "distinct", "one", "half", "third"])
def test_constructed_ties(segments, gpu_knobs, col, split):
    """two, three and 65 tied values (their ids in different 64-id chunks, and with PG_MODE_SPLIT_IDS=64 in different wavefront shares of a
    split row), all values distinct (every id ties), one value only; each under MIN / MAX / AVG, as map and as final.  `third` ties 0.1, 0.2
    and 0.3, whose exact sum is no double: the model's single rounding decides."""
    if split:
        gpu_knobs(PG_MODE_SPLIT_IDS=split)
    seg = segments(2049)
    host, data, schema, gpu, _ = seg
    b = _check(seg, f"SELECT MODE({col}), MODE({col}, 'MAX'), MODE({col}, 'AVG') FROM t")
    m = b.aggregation_result()[0]
    top = max(c for _, c in m[1])
    assert sum(1 for _, c in m[1] if c == top) == {"t2": 2, "t3": 3, "t65": 65, "distinct": 2049, "one": 1, "half": 1, "third": 3}[col]
    _check(seg, f"SELECT MODE({col}, 'AVG'), MODE({col}) FROM t WHERE s < 700")
    _check(seg, f"SELECT g2, MODE({col}, 'AVG'), MODE({col}, 'MAX') FROM t GROUP BY g2")
    _check(seg, f"SELECT g7, g20, MODE({col}, 'AVG'), MODE({col}) FROM t WHERE s < 700 GROUP BY g7, g20")
    if col == "half":   # 1 025 x 0.5 against 1 024 x 0.25 without a filter; tied 2 : 2 on four docs
        _check(seg, "SELECT MODE(half, 'AVG') FROM t WHERE u1 < 4")


# ---- the tiers from both sides ----------------------------------------------------------------------------------------------------------------------------
def test_tiers_and_their_boundaries(segments, gpu_knobs, gpu_api):
    seg = segments(2047)
    sql = "SELECT g7, MODE(xi, 'AVG'), MODE(xi), MODE(t3, 'AVG'), COUNT(*) FROM t WHERE s < 900 GROUP BY g7"   # xi: G x C = 7 x 41 counters
    want = _check(seg, sql, kernel="pg_pctl_lds").rows()
    one = "SELECT g7, MODE(xi, 'AVG'), MODE(xi, 'MAX') FROM t WHERE s < 900 GROUP BY g7"
    _check(seg, one, kernel="pg_pctl_lds")
    gpu_knobs(PG_PCTL_LDS_MAX_KEYS=287)
    _check(seg, one, kernel="pg_pctl_lds")           # exactly at the LDS cap
    gpu_knobs(PG_PCTL_LDS_MAX_KEYS=286)
    _check(seg, one, kernel="pg_pctl_hbm")           # one above it
    assert _check(seg, sql).rows() == want
    gpu_knobs(PG_PCTL_LDS_MAX_KEYS=286, PG_PCTL_HBM_MAX_BYTES=1148)
    _check(seg, one, kernel="pg_pctl_hbm")           # exactly at the HBM budget
    gpu_knobs(PG_PCTL_LDS_MAX_KEYS=286, PG_PCTL_HBM_MAX_BYTES=1147)
    _check(seg, one, kernel="pg_pctl_sort")          # one above it: a MODE-only query through the sort tier
    assert _check(seg, sql, kernel="pg_pctl_sort").rows() == want
    _check(seg, "SELECT MODE(rd, 'MAX'), MODE(t65, 'AVG'), MODE(distinct, 'AVG') FROM t", kernel="pg_pctl_sort")   # 65 and 2 047 ties compacted from the runs
    _check(seg, "SELECT MODE(distinct, 'AVG') FROM t WHERE s > 5000", kernel="pg_pctl_sort")
    gpu_knobs(PG_PCTL_LDS_MAX_KEYS=286, PG_PCTL_HBM_MAX_BYTES=1147, PG_PCTL_SORT_MAX_BYTES=1024)
    with pytest.raises(capi.NativeError) as e:
        seg[3].execute(one)
    assert e.value.status == capi.PG_ERR_UNSUPPORTED and "PG_PCTL_SORT_MAX_BYTES" in e.value.message and "MODE(xi)" in e.value.message
    gpu_api.call("query_supported", seg[3].handle, CQuery(parse_sql(one)).ptr())


# ---- the wide-row split --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [None, 64, 4096])
def test_wide_rows_without_group_by(segments, gpu_knobs, split):
    """cardinalities 64, 65, 1 025 (one above the default share of 1 024 ids: the first row cut in two), 4 097; `far` ties its lowest and its highest id of 4 102, in
    different shares under every setting but 4096.  (The statistics do not say which shape ran: the knob moves the switch across each width.)"""
    if split:
        gpu_knobs(PG_MODE_SPLIT_IDS=split)
    seg = segments("wide")
    for col in ("w64", "w65", "w1025", "w4097", "far"):
        _check(seg, f"SELECT MODE({col}), MODE({col}, 'MAX'), MODE({col}, 'AVG') FROM t", kernel="pg_pctl_lds")
        _check(seg, f"SELECT MODE({col}, 'AVG') FROM t WHERE s < 333", kernel="pg_pctl_lds")
    gpu_knobs(PG_MODE_SPLIT_IDS=split or 1024, PG_PCTL_LDS_MAX_KEYS=64)
    _check(seg, "SELECT MODE(far, 'AVG'), MODE(w4097, 'AVG'), MODE(w65) FROM t", kernel="pg_pctl_hbm")


# ---- sharing and nesting ---------------------------------------------------------------------------------------------------------------------------------------
def test_one_counting_pass_per_column_and_the_nesting(segments):
    seg = segments(2049)
    host, data, schema, gpu, oracle = seg
    b = _check(seg, "SELECT MODE(xd), MODE(xd, 'MAX'), PERCENTILE(xd, 50) FROM t WHERE s < 800")
    assert b.stats.percentile_passes == 1
    docs, _ = _filter(oracle, "SELECT COUNT(*) FROM t WHERE s < 800")
    assert pm.same_runs(b.aggregation_result()[2], pm.runs(np.asarray(data["xd"])[docs]))
    b = _check(seg, "SELECT g7, PERCENTILE(ri, 95), MODE(ri, 'AVG'), MODE(xi) FROM t GROUP BY g7")
    assert b.stats.percentile_passes == 2
    # each flag governs its own function: final PERCENTILE values next to MODE maps, and the reverse
    for flag, kinds in ((capi.QUERY_FLAG_FINAL_PERCENTILE, (float, tuple)), (capi.QUERY_FLAG_FINAL_MODE, (tuple, float))):
        qc = parse_sql("SELECT PERCENTILE(rd, 50), MODE(rd) FROM t")
        qc.flags |= flag
        got = gpu.execute(qc).aggregation_result()
        assert isinstance(got[0], kinds[0]) and isinstance(got[1], kinds[1]), (flag, got)
    # next to a HISTOGRAM, a variance and an expression aggregation: the passes nest, the MODE innermost
    b = _check(seg, "SELECT g7, HISTOGRAM(ri, -20, 20, 5), VAR_POP(xi), SUM(xi + ri), MODE(xi, 'AVG'), COUNT(*) FROM t WHERE s < 600 GROUP BY g7")
    assert b.stats.percentile_passes == 1


def test_order_by_mode_leaves_the_segment_untrimmed(segments):
    seg = segments(2049)
    b = _check(seg, "SELECT g20, MODE(xi, 'MAX'), COUNT(*) FROM t GROUP BY g20 ORDER BY MODE(xi, 'MAX') DESC, g20 LIMIT 3")
    assert len(b.rows()) == 20


def test_multi_segment_merge_in_the_python_executor(segments):
    a, b = segments(2047), segments(2049)
    sql = "SELECT g7, MODE(xl, 'AVG'), MODE(rf, 'MAX'), COUNT(*) FROM t WHERE s < 900 GROUP BY g7"
    blocks = [a[3].execute(sql), b[3].execute(sql)]
    merged = GroupByCombineOperator(blocks).merge()
    final = GroupByCombineOperator(blocks).final()
    for key, vals in merged.items():
        for i, (col, red) in enumerate((("xl", "AVG"), ("rf", "MAX"))):
            docs = [np.flatnonzero((np.asarray(s[1]["g7"]) == key[0]) & (np.asarray(s[1]["s"]) < 900)) for s in (a, b)]
            want = mm.merge(mm.value_map(np.asarray(a[1][col])[docs[0]], TYPE_OF[col]), mm.value_map(np.asarray(b[1][col])[docs[1]], TYPE_OF[col]))
            assert mm.same_map(vals[i], want) and mm.same_double(final[key][i], mm.final(want, red)), (key, col)
    with pytest.raises(ValueError) as e:
        mode_merge(blocks[0].rows()[next(iter(merged))][0], blocks[0].rows()[next(iter(merged))][1])
    assert "Long2LongOpenHashMap, Float2LongOpenHashMap" in str(e.value)


# ---- the data table -----------------------------------------------------------------------------------------------------------------------------------------
def test_data_table_bytes_and_names(segments, monkeypatch):
    """A column is an OBJECT of ObjectSerDeUtils type 23 .. 26; its name is mode(x), without the reducer; an empty map is type 23"""
    inner = dt.deserialize_object
    seen = []

    def deserialize(kind, b):
        if 23 <= kind <= 26:
            seen.append((kind, bytes(b)))
            return mm.deserialize(kind, bytes(b))
        return inner(kind, b)
    monkeypatch.setattr(dt, "deserialize_object", deserialize)
    host, data, schema, gpu, oracle = segments(2049)
    sql = "SELECT g2, COUNT(*), MODE(xi), MODE( rl , 'MAX'), MODE(xf, 'AVG'), MODE(rd) FROM t WHERE s < 500 GROUP BY g2"
    r = gpu.execute_native(sql, keep_device_table=False)
    t = dt.parse_data_table_v4(r.data_table_v4())
    r.free()
    assert t["names"] == ["g2", "count(*)", "mode(xi)", "mode(rl)", "mode(xf)", "mode(rd)"]
    assert t["types"] == ["INT", "LONG", "OBJECT", "OBJECT", "OBJECT", "OBJECT"] and len(t["rows"]) == 2
    docs, _ = _filter(oracle, sql)
    wants = []
    for row in t["rows"]:
        gdocs = docs[np.asarray(data["g2"])[docs] == row[0]]
        for cell, col in zip(row[2:], ("xi", "rl", "xf", "rd")):
            want = mm.value_map(np.asarray(data[col])[gdocs], schema[col])
            assert mm.same_map(cell, want), (row[0], col)
            wants.append(mm.serialize(want))
    assert [k for k, _ in seen] == [23, 24, 25, 26] * 2 and seen == wants   # the bytes are the model's serializer's
    del seen[:]
    r = gpu.execute_native("SELECT MODE(xd, 'AVG') FROM t WHERE s > 5000", keep_device_table=False)
    t = dt.parse_data_table_v4(r.data_table_v4())
    r.free()
    assert t["names"] == ["mode(xd)"] and [list(row) for row in t["rows"]] == [[("INT", ())]] and seen == [(23, b"\0\0\0\0")]
    qc = parse_sql("SELECT MODE(xd) FROM t")
    qc.flags |= capi.QUERY_FLAG_FINAL_MODE
    r = gpu.execute_native(qc, keep_device_table=False)
    with pytest.raises(capi.NativeError) as e:
        r.data_table_v4()
    assert e.value.status == capi.PG_ERR_INVALID_ARGUMENT and "PG_QUERY_FLAG_FINAL_MODE" in e.value.message
    r.free()


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
    qc = parse_sql("SELECT MODE(xd) FROM t")
    qc.aggregations[0].column = column
    return qc


def test_plan_time_refusals_and_the_merge_refusal(gpu_api):
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
        _refused(gpu_api, seg, parse_sql("SELECT MODE(txt) FROM t"), U, "MODE over the STRING column txt")
        _refused(gpu_api, seg, parse_sql("SELECT g7, mode(by, 'MAX') FROM t GROUP BY g7"), U, "MODE over the BYTES column by")
        _refused(gpu_api, seg, parse_sql("SELECT MODE(mv) FROM t"), U, "MODE over the multi-value column mv")
        _refused(gpu_api, seg, parse_sql("SELECT g7, MODE(ri * xd, 'AVG') FROM t GROUP BY g7"), U, "MODE over an expression")
        _refused(gpu_api, seg, parse_sql("SELECT mv, MODE(xd) FROM t GROUP BY mv"), U, "MODE next to the multi-value group-by column mv")
        _refused(gpu_api, seg, parse_sql("SELECT MODE(nope) FROM t"), capi.PG_ERR_NOT_FOUND, "column not found: nope")
        for col, text in (("xi", "MODE over xi, which holds nulls"), ("xd", "MODE grouped by g20, which holds nulls")):
            qc = parse_sql(f"SELECT g20, MODE({col}, 'AVG') FROM t GROUP BY g20")
            qc.flags |= capi.QUERY_FLAG_NULL_HANDLING
            _refused(gpu_api, seg, qc, U, text)
        qc = parse_sql("SELECT g7, MODE(xd), SUM(ri) FROM t GROUP BY g7")   # columns without nulls run under the flag
        qc.flags |= capi.QUERY_FLAG_NULL_HANDLING
        assert len(seg.execute(qc).rows()) == 7
        _refused(gpu_api, seg, parse_sql("SELECT u1, u2, u3, MODE(xd) FROM t GROUP BY u1, u2, u3"), U, "MODE: group key space over 2^32")
        for column, text in (("xd,'MIN','MAX'", "Mode expects at most 2 arguments, got: 3"), ("xd,'avg'", "MultiModeReducerType.avg"),
                             ("xd,'MEDIAN'", "No enum constant org.apache.pinot.core.query.aggregation.function.ModeAggregationFunction.MultiModeReducerType.MEDIAN"),
                             ("xd,MAX", "quoted MultiModeReducerType"), ("xd,", "empty argument"), ("xd,'MAX", "unterminated quote")):
            _refused(gpu_api, seg, _with_column(column), I, text)
        a = seg.execute_native("SELECT g7, COUNT(*), MODE(xd) FROM t GROUP BY g7")
        b = seg.execute_native("SELECT g7, COUNT(*), MODE(xd) FROM t GROUP BY g7")
        with pytest.raises(capi.NativeError) as e:
            a.merge(b)
        assert e.value.status == U and "merged by value on the Java side" in e.value.message and "MODE" in e.value.message
        comm = Comm.init_rank(gpu_api, 0, 1, 0, Comm.unique_id(gpu_api))
        with pytest.raises(capi.NativeError) as e:
            a.all_reduce(comm)
        assert e.value.status == U and "merged by value on the Java side" in e.value.message
        comm.destroy()
        a.free()
        b.free()
    finally:
        seg.destroy()


# ---- the build ----------------------------------------------------------------------------------------------------------------------------------------------
def test_mode_kernels_use_no_scratch():
    """the build leaves hipcc's kernel-resource-usage remarks behind: neither the selection kernels nor the generalised run compaction may spill"""
    for name, kernels in (("pg_kernels_mode", ("pg_mode_select", "pg_mode_finish", "pg_mode_sort_select")), ("pg_kernels_percentile", ("pg_pctl_runs", "pg_pctl_sort_runs"))):
        log = os.path.join(ROOT, "pinot_amd", "csrc", name + ".resources.log")
        assert os.path.exists(log), "the build writes the resource log next to the library"
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
