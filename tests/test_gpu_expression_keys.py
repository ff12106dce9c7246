"""GROUP BY and SELECT DISTINCT over arithmetic expressions on the GPU path.

The yardstick is a TWIN COLUMN: every test segment carries, for each expression text under test, a raw DOUBLE column holding
tests/expression_model.py's evaluate(text) of the same data.  GROUP BY <text> on the GPU must equal GROUP BY <twin> over the same segment —
on the oracle (pinned to the reference for raw DOUBLE keys) where the oracle knows every aggregation of the query, else on the GPU path's own
raw DOUBLE keys (SUM(expr) and PERCENTILE next to the key, DISTINCT: pinned by their own suites): the same keys compared as
Double.doubleToLongBits (so that 0.0 / -0.0 and the NaNs are told apart as the reference tells them), the same aggregates bit for bit, the same
numDocsScanned and numEntriesScannedInFilter, and numEntriesScannedPostFilter from percentile_model.statistics over the OPERAND columns."""
import dataclasses
import json
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
from tests.fixtures import sv_segment
from tests.kernel_inventory import snapshot_doc_ids

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPECTED = json.load(open(os.path.join(ROOT, "tests", "golden", "expression_group_by_expected.json")))["group_by_udf_order_by_udf"]
# one doc; a partial second word; either side of the kernel's four-word iteration; either side of a 2 048-doc wave tile of the id pack
SIZES = [1, 65, 255, 257, 2047, 2049]
NO_DICT = ["rid", "rg", "rs", "rdk", "ri", "rl", "rf", "rd", "za"]


def _operand_texts():
    """the expressions of test_gpu_expressions.OPERANDS (all four types, dictionary-encoded and raw, literals on either side, nesting)"""
    out = []
    for sql in tge.OPERANDS:
        for a in parse_sql(sql).aggregations:
            if "(" in (a.column or "") and a.column not in out:
                out.append(a.column)
    return out


OPERAND_TEXTS = _operand_texts()
# ... and the texts of the other cases: a coarse key, signed zeros, the non-finite values, one key per doc
EXTRA_TEXTS = ["sub(g20,'100000')", "divide(rg,'1000')", "mult(ri,'0')", "div(za,zz)", "add(rid,'0.5')", "times(g7,g3)", "minus(s,g7)"]
TEXTS = OPERAND_TEXTS + [t for t in EXTRA_TEXTS if t not in OPERAND_TEXTS]


def _evaluate(text, data, schema):
    with np.errstate(all="ignore"):
        return np.asarray(em.evaluate(text, data, schema), dtype=np.float64)


def _data(n, seed=11):
    _, data, schema = tge._data(n, seed)
    data, schema = dict(data), dict(schema)
    rng = np.random.default_rng(1000 + n)
    data["za"] = rng.choice(np.array([-2, 0, 3], dtype=np.int32), n)   # zeros in both columns of div(za,zz): +Inf, -Inf and NaN
    data["zz"] = rng.choice(np.array([0, 1], dtype=np.int32), n)
    schema.update(za="INT", zz="INT")
    twins = {}
    for i, text in enumerate(TEXTS):
        twins[text] = "k%d" % i
        data["k%d" % i] = _evaluate(text, data, schema)
        schema["k%d" % i] = "DOUBLE"
    host = build_segment("exprkey_%d" % n, data, schema, inverted_index_columns=["c_inv1"], no_dictionary_columns=NO_DICT + list(twins.values()))
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


def _bits(v):
    """Double.doubleToLongBits"""
    v = np.float64(v)
    return 0x7FF8000000000000 if np.isnan(v) else int(v.view(np.uint64))


def _key_rows(b):
    """[(key tuple, results)] in result order; DOUBLE value keys as their long bits"""
    vcols = b.group_value_columns
    keys = []
    for i, k in enumerate(b.group_keys):
        keys.append(tuple(("bits", _bits(vcols[j][i])) if j in vcols and vcols[j].dtype == np.float64 else c for j, c in enumerate(k)))
    cols = b.columns
    return [(k, [c[i] for c in cols]) for i, k in enumerate(keys)]


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


def _columns_read(qc):
    read = set()
    for g in qc.group_by or qc.distinct:
        read |= set(em.columns_of(g)) if "(" in g else {g}
    for a in qc.aggregations:
        if "(" in (a.column or ""):
            read |= set(em.columns_of(a.column))
        elif a.column:
            read.add(a.column)
    return read


def _check(seg, sql, reference="oracle", ordered=False, **params):
    """`sql` with expression keys on the GPU against its twin (the same query over the twin columns) on `reference`"""
    host, data, schema, twins, gpu, oracle = seg
    qc = sql if isinstance(sql, QueryContext) else parse_sql(sql)
    for k, v in params.items():
        setattr(qc, k, v)
    assert any("(" in g for g in qc.group_by), sql
    assert all(g in twins for g in qc.group_by if "(" in g), (sql, qc.group_by)
    b = gpu.execute(qc)
    w = (oracle if reference == "oracle" else gpu).execute(_twin_query(qc, twins))
    got, want = _key_rows(b), _key_rows(w)
    assert len({k for k, _ in got}) == len(got), sql
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


# ---- the reference's golden ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sv(gpu_api, sv_data):
    host = sv_segment(sv_data)
    g = NativeSegment(gpu_api, host)
    yield host, g
    g.destroy()


@pytest.mark.parametrize("which", ["query", "query_space_tab"])
def test_group_by_udf_order_by_udf_golden(sv, which):
    """InterSegmentGroupBySingleValueQueriesTest.java:227-241: keys 140528.0, 194355.0, 532157.0 with counts 28, 12, 12 over four copies of
    the segment — 7, 3, 3 per segment; numDocsScanned 120 000 = 4 x 30 000"""
    host, gpu = sv
    assert [4 * c for c in EXPECTED["counts_per_segment"]] == EXPECTED["counts_over_four_segments"]
    qc = parse_sql(EXPECTED[which])
    assert qc.group_by == [EXPECTED["column_names"][0]] and qc.resolved_order_by() == [(capi.ORDER_BY_GROUP_KEY, 0, True)]
    b = gpu.execute(qc)                                   # untrimmed: every group of the segment, the broker orders them
    rows = sorted(((k[0], r[0]) for k, r in b.rows().items()))
    assert rows[:3] == list(zip(EXPECTED["keys"], EXPECTED["counts_per_segment"]))
    assert b.stats.num_docs_scanned == EXPECTED["num_docs_scanned_per_segment"] == host.total_docs
    assert b.stats.num_entries_scanned_post_filter == host.total_docs   # one operand column
    qc.min_segment_group_trim_size = 1                    # trimmed by the segment: max(5 x 3, 1) = 15 groups, the smallest keys
    t = gpu.execute(qc)
    assert sorted(((k[0], r[0]) for k, r in t.rows().items())) == rows[:15]
    r = gpu.execute_native(qc, keep_device_table=False)
    table = dt.parse_data_table_v4(r.data_table_v4())
    r.free()
    assert table["names"] == EXPECTED["column_names"] and table["types"] == EXPECTED["column_types"]
    assert sorted(tuple(x) for x in table["rows"])[:3] == list(zip(EXPECTED["keys"], EXPECTED["counts_per_segment"]))


# ---- operands -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_operands_as_keys(segments, n):
    seg = segments(n)
    for text in OPERAND_TEXTS:
        _check(seg, f"SELECT {text}, COUNT(*) FROM t GROUP BY {text}")


@pytest.mark.parametrize("n", SIZES)
def test_key_shapes(segments, n):
    seg = segments(n)
    # one expression key alone, with a dictionary column, with a raw column; two expression keys; with and without a filter
    _check(seg, "SELECT sub(g20,'100000'), COUNT(*), SUM(s), MAX(ri), AVG(s), MIN(rd) FROM t GROUP BY sub(g20,'100000')")
    # (a SUM over a floating-point column, or over LONGs beyond 2^53, is one exactly rounded sum on the GPU path and a sum in doc order on the
    # oracle: its twin is the GPU's)
    _check(seg, "SELECT sub(g20,'100000'), COUNT(*), SUM(rd), AVG(rf), SUM(rl) FROM t GROUP BY sub(g20,'100000')", reference="gpu")
    _check(seg, "SELECT g7, rg / 1000, COUNT(*), MIN(dd) FROM t WHERE s < 700 GROUP BY g7, rg / 1000")
    _check(seg, "SELECT rg / 1000, rg, rs, COUNT(*), MINMAXRANGE(di) FROM t WHERE c_inv1 IN (1, 5) GROUP BY rg / 1000, rg, rs")
    _check(seg, "SELECT g7 * g3, s - g7, COUNT(*), SUM(di), MAX(rl) FROM t WHERE s BETWEEN 100 AND 900 GROUP BY g7 * g3, s - g7")
    _check(seg, "SELECT g7 * g3, g7, COUNT(*) FROM t GROUP BY g7 * g3, g7")          # an operand that is a plain key as well: counted once
    # behind an expression predicate (the oracle has no such leaf: the twin runs on the GPU path as well)
    _check(seg, "SELECT sub(g20,'100000'), g3, COUNT(*), SUM(s) FROM t WHERE ri * rd > 0 AND s < 900 GROUP BY sub(g20,'100000'), g3", reference="gpu")


@pytest.mark.parametrize("n", SIZES)
def test_next_to_sum_of_an_expression_and_a_percentile(segments, n):
    seg = segments(n)
    _check(seg, "SELECT sub(g20,'100000'), SUM(ri * rd), COUNT(*) FROM t WHERE s < 800 GROUP BY sub(g20,'100000')", reference="gpu")
    b, _ = _check(seg, "SELECT rg / 1000, g3, PERCENTILE(di, 95), COUNT(*), MAX(s) FROM t GROUP BY rg / 1000, g3", reference="gpu")
    assert b.stats.percentile_passes == 1
    _check(seg, "SELECT g7 * g3, SUM(add(di,dl)), PERCENTILE(rd, 50), AVG(g7 * g3) FROM t WHERE s >= 50 GROUP BY g7 * g3", reference="gpu")


# ---- key semantics --------------------------------------------------------------------------------------------------------------------------------
def test_signed_zeros_are_two_groups(segments):
    seg = segments(2049)
    b, _ = _check(seg, "SELECT mult(ri,'0'), COUNT(*) FROM t GROUP BY mult(ri,'0')")
    rows = dict(_key_rows(b))
    ri = seg[1]["ri"]
    assert rows == {(("bits", 0),): [int((ri > 0).sum())], (("bits", 1 << 63),): [int((ri < 0).sum())]}


def test_division_by_zero_gives_ordinary_keys(segments):
    """+Inf, -Inf and ONE NaN group (0 / 0): a division by zero is not refused in a key, unlike in a SUM"""
    seg = segments(2049)
    b, _ = _check(seg, "SELECT div(za,zz), COUNT(*) FROM t GROUP BY div(za,zz)")
    za, zz = seg[1]["za"], seg[1]["zz"]
    want = {_bits(np.inf): int(((za > 0) & (zz == 0)).sum()), _bits(-np.inf): int(((za < 0) & (zz == 0)).sum()),
            0x7FF8000000000000: int(((za == 0) & (zz == 0)).sum()), _bits(-2.0): int(((za == -2) & (zz == 1)).sum()),
            _bits(3.0): int(((za == 3) & (zz == 1)).sum()), _bits(0.0): int(((za == 0) & (zz == 1)).sum())}
    assert all(c > 0 for c in want.values())
    assert {k[0][1]: r[0] for k, r in _key_rows(b)} == want
    _check(seg, "SELECT div(za,zz), g3, COUNT(*), SUM(s) FROM t WHERE s < 500 GROUP BY div(za,zz), g3 ORDER BY div(za,zz) DESC, g3 LIMIT 2", min_segment_group_trim_size=1)


@pytest.mark.parametrize("n", [257, 2049])
def test_order_by_the_key_and_segment_trim(segments, n):
    seg = segments(n)
    # (every ORDER BY names all the keys: which of two groups that tie survives a trim is not pinned)
    for tail in ("ORDER BY rg / 1000, g3 LIMIT 2", "ORDER BY rg / 1000 DESC, g3 DESC LIMIT 1", "ORDER BY g3 DESC, DIVIDE( rg, 1000 ) LIMIT 1"):
        for mst in (1, 7):
            qc = parse_sql("SELECT rg / 1000, g3, COUNT(*), SUM(s) FROM t WHERE s < 900 GROUP BY rg / 1000, g3 " + tail)
            assert qc.resolved_order_by() is not None
            b, w = _check(seg, qc, min_segment_group_trim_size=mst)
            assert len(b.group_keys) == len(w.group_keys) == min(max(5 * qc.limit, mst), len(w.group_keys))


def test_num_groups_limit(segments):
    seg = segments(2049)
    for sql in ("SELECT add(rid,'0.5'), COUNT(*) FROM t GROUP BY add(rid,'0.5')", "SELECT rg / 1000, g20, COUNT(*), SUM(s) FROM t WHERE s < 900 GROUP BY rg / 1000, g20"):
        b, _ = _check(seg, sql, num_groups_limit=13)
        assert len(b.group_keys) == 13 and b.stats.num_groups_limit_reached == 1


@pytest.mark.parametrize("n", SIZES)
def test_one_key_per_doc(segments, n):
    """as many distinct values as docs: beyond the dense tables"""
    b, _ = _check(segments(n), "SELECT add(rid,'0.5'), COUNT(*), SUM(s) FROM t GROUP BY add(rid,'0.5')")
    assert len(b.group_keys) == n


def test_upsert_snapshot(gpu_api, oracle_api):
    host, data, schema, twins = _data(2049, seed=9)
    g, o = NativeSegment(gpu_api, host), NativeSegment(oracle_api, host)
    keep = snapshot_doc_ids(host.total_docs)
    g.set_queryable_doc_ids(keep)
    o.set_queryable_doc_ids(keep)
    try:
        seg = (host, data, schema, twins, g, o)
        b, _ = _check(seg, "SELECT sub(g20,'100000'), COUNT(*), SUM(s) FROM t GROUP BY sub(g20,'100000')")
        assert b.stats.num_docs_scanned == len(keep)
        _check(seg, "SELECT rg / 1000, g7, COUNT(*) FROM t WHERE s < 600 GROUP BY rg / 1000, g7")
    finally:
        g.destroy()
        o.destroy()


# ---- DISTINCT -------------------------------------------------------------------------------------------------------------------------------------
def _distinct_rows(b):
    vcols = b.group_value_columns
    return [tuple(("bits", _bits(vcols[j][i])) if j in vcols and vcols[j].dtype == np.float64 else c for j, c in enumerate(k))
            for i, k in enumerate(b.distinct_rows)]


@pytest.mark.parametrize("n", SIZES)
def test_distinct(segments, n):
    """SELECT DISTINCT <expr>, col and its GROUP-BY-without-aggregations spelling against the DISTINCT twin, ordered and in docId order"""
    host, data, schema, twins, gpu, oracle = segments(n)
    for where, tail in ((" WHERE s < 800", " ORDER BY g3 DESC, rg / 1000 LIMIT 10"), ("", " ORDER BY rg / 1000 DESC, g3 LIMIT 4"), (" WHERE s < 800", " LIMIT 7"), ("", " LIMIT 100000")):
        qd = parse_sql("SELECT DISTINCT rg / 1000, g3 FROM t" + where + tail)
        qg = parse_sql("SELECT rg / 1000, g3 FROM t" + where + " GROUP BY rg / 1000, g3" + tail)
        assert qg.has_group_by and qg.group_by == qd.distinct and not qg.aggregations
        qg.distinct, qg.group_by = qg.group_by, []       # the broker's rewrite of a GROUP BY without aggregations
        want = gpu.execute(_twin_query(qd, twins))
        for q in (qd, qg):
            b = gpu.execute(q)
            assert _distinct_rows(b) == _distinct_rows(want), tail
            assert b.stats.num_docs_scanned == want.stats.num_docs_scanned and b.stats.num_entries_scanned_in_filter == want.stats.num_entries_scanned_in_filter
            assert b.stats.num_entries_scanned_post_filter == b.stats.num_docs_scanned * len({"rg", "g3"})
    # an unbounded DISTINCT is the oracle's key set over the twin
    b = gpu.execute("SELECT DISTINCT mult(ri,'0'), div(za,zz) FROM t LIMIT 100000")
    w = oracle.execute(_twin_query(parse_sql("SELECT mult(ri,'0'), div(za,zz), COUNT(*) FROM t GROUP BY mult(ri,'0'), div(za,zz)"), twins))
    assert sorted(_distinct_rows(b)) == sorted(k for k, _ in _key_rows(w))
    assert b.stats.num_entries_scanned_post_filter == b.stats.num_docs_scanned * 3


# ---- results --------------------------------------------------------------------------------------------------------------------------------------
def test_data_table_names_and_types(segments):
    host, data, schema, twins, gpu, oracle = segments(2047)
    r = gpu.execute_native("SELECT SUB(g20, 100000), g3, rg / 1000, COUNT(*) FROM t WHERE s < 500 GROUP BY SUB(g20, 100000), g3, rg / 1000", keep_device_table=False)
    t = dt.parse_data_table_v4(r.data_table_v4())
    rows = r.block().rows()
    r.free()
    assert t["names"] == ["sub(g20,'100000')", "g3", "divide(rg,'1000')", "count(*)"]
    assert t["types"] == ["DOUBLE", "INT", "DOUBLE", "LONG"] and len(t["rows"]) == len(rows) > 3
    for a, g3, c, count in t["rows"]:
        assert isinstance(a, float) and isinstance(c, float) and rows[(a, g3, c)] == [count]
    r = gpu.execute_native("SELECT DISTINCT rg / 1000, g3 FROM t ORDER BY rg / 1000 LIMIT 3", keep_device_table=False)
    t = dt.parse_data_table_v4(r.data_table_v4())
    r.free()
    assert t["names"] == ["divide(rg,'1000')", "g3"] and t["types"] == ["DOUBLE", "INT"] and len(t["rows"]) == 3


def test_merge_of_two_results(segments):
    """pg_result_merge treats a result keyed by an expression as one keyed by a raw DOUBLE column of the same values: merged alike, or refused alike"""
    host, data, schema, twins, gpu, oracle = segments(2047)
    for sql in ("SELECT sub(g20,'100000'), COUNT(*), SUM(s) FROM t WHERE s < 800 GROUP BY sub(g20,'100000')",
                "SELECT rg / 1000, g3, COUNT(*), MAX(ri) FROM t GROUP BY rg / 1000, g3"):
        qc = parse_sql(sql)
        outcomes = []
        for q in (qc, _twin_query(qc, twins)):
            a, b = gpu.execute_native(q), gpu.execute_native(q)
            try:
                a.merge(b)
                outcomes.append(("merged", _key_rows(a.block())))
            except capi.NativeError as e:
                outcomes.append(("refused", e.status))
            finally:
                a.free()
                b.free()
        assert outcomes[0][0] == outcomes[1][0], (sql, outcomes)
        if outcomes[0][0] == "merged":
            once = dict(_key_rows(gpu.execute(qc)))
            assert dict(outcomes[0][1]).keys() == dict(outcomes[1][1]).keys() == once.keys()
            for k, r in outcomes[0][1]:
                assert _same_value(r, dict(outcomes[1][1])[k]) and r[0] == 2 * once[k][0], (sql, k)
        else:
            assert outcomes[0][1] == outcomes[1][1], (sql, outcomes)


def test_seventeen_texts_on_one_segment(gpu_api, segments):
    """one more text than the segment keeps derived columns: the one used longest ago goes, and comes back right"""
    host, data, schema, twins, _, oracle = segments(2047)
    gpu = NativeSegment(gpu_api, host)
    try:
        before = gpu.device_bytes()
        texts = ["add(ri,'%d')" % k for k in range(17)]
        for text in texts + texts[:1]:
            b = gpu.execute(f"SELECT {text}, COUNT(*), SUM(s) FROM t GROUP BY {text}")
            v = _evaluate(text, data, schema)
            want = {}
            for i, x in enumerate(v):
                e = want.setdefault(_bits(x), [0, 0.0])
                e[0] += 1
                e[1] += float(data["s"][i])
            assert {k[0][1]: r for k, r in _key_rows(b)} == want, text
        sixteen = gpu.device_bytes() - before
        gpu.execute("SELECT add(ri,'99'), COUNT(*) FROM t GROUP BY add(ri,'99')")
        assert gpu.device_bytes() - before == sixteen > 0      # the bit-packed ids of at most 16 derived columns are kept
    finally:
        gpu.destroy()


def test_star_tree_route_is_not_taken(gpu_api):
    from tests.fixtures import synth_star_segment
    host = synth_star_segment(num_docs=20_000)
    seg = NativeSegment(gpu_api, host)
    try:
        plain = seg.execute("SELECT h1, COUNT(*), SUM(m) FROM gpuBench GROUP BY h1")
        assert plain.stats.star_tree_index >= 0
        b = seg.execute("SELECT h1 + 1, COUNT(*), SUM(m) FROM gpuBench GROUP BY h1 + 1")
        assert b.stats.star_tree_index == -1 and b.stats.num_docs_scanned == 20_000
        assert {(k[0] - 1.0,): r for k, r in b.rows().items()} == {(float(k[0]),): r for k, r in plain.rows().items()}
    finally:
        seg.destroy()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------
def _keys(*texts, **kw):
    return QueryContext(group_by=list(texts), aggregations=[AggregationSpec("COUNT")], has_group_by=True, **kw)


def test_refusals(gpu_api):
    from pinot_amd.segment import build_column, build_mv_column
    host, data, schema, twins = _data(2047, seed=3)
    rng = np.random.default_rng(1)
    host.columns["by"] = build_column("by", [b"ab%d" % (i % 5) for i in range(host.total_docs)], "BYTES", dictionary=False)
    host.columns["mv"] = build_mv_column("mv", [list(rng.integers(0, 20, rng.integers(1, 4))) for _ in range(host.total_docs)], "INT")
    host.columns["di"].null_vector = np.frombuffer(formats.serialize_roaring(np.array([3, 77, 2000], dtype=np.int64)), dtype=np.uint8)
    seg = NativeSegment(gpu_api, host)
    refused = lambda qc, status, text: tge._refused(gpu_api, seg, qc, status, text)   # noqa: E731: through pg_query_supported and pg_query_exec
    try:
        U, I, N = capi.PG_ERR_UNSUPPORTED, capi.PG_ERR_INVALID_ARGUMENT, capi.PG_ERR_NOT_FOUND
        refused(_keys("add(ri,mv)"), U, "expression over the multi-value column mv")
        refused(_keys("add(ri,txt)"), U, "expression over the STRING column txt")
        refused(_keys("add(ri,rs)"), U, "expression over the STRING column rs")
        refused(_keys("add(ri,by)"), U, "expression over the BYTES column by")
        refused(_keys("mod(ri,'3')"), U, "the function mod")
        refused(_keys("add(ri,abs(rd))"), U, "the function abs")
        refused(_keys("add(" + ",".join(["ri"] * 16) + ")"), U, "more than 15 operations")
        refused(_keys("add(" + ",".join(["ri", "rd", "di", "dl", "df", "dd", "rl", "rf", "s"]) + ")"), U, "more than 8 distinct columns")
        refused(_keys(*["add(ri,'%d')" % k for k in range(5)]), U, "more than 4 expressions among the group-by / DISTINCT keys")
        refused(_keys("add(ri,rd)", "mv"), U, "multi-value group-by column mv next to the expression key add(ri,rd)")
        refused(parse_sql("SELECT DISTINCT ri + rd, mv FROM t"), U, "multi-value group-by column mv next to the expression key")
        for q in (_keys("add(di,rd)"), parse_sql("SELECT DISTINCT di * 2 FROM t")):
            q.flags |= capi.QUERY_FLAG_NULL_HANDLING
            refused(q, U, "expression over di, which holds nulls")
        q = _keys("add(ri,rd)", "g7")                           # columns without nulls run under the flag
        q.flags |= capi.QUERY_FLAG_NULL_HANDLING
        assert len(seg.execute(q).rows()) > 7
        assert len(seg.execute(_keys("add(di,rd)")).rows()) > 7   # ... and the column with nulls without it
        # a selection naming an expression stays with the Java plan
        q = parse_sql("SELECT ri + rd, g7 FROM t LIMIT 5")
        assert q.flags & capi.QUERY_FLAG_SELECTION
        refused(q, U, "selection of the expression plus(ri,rd)")
        refused(parse_sql("SELECT g7 FROM t ORDER BY ri + rd LIMIT 5"), U, "selection of the expression plus(ri,rd)")
        # malformed texts and unknown operands, with the parser's texts
        refused(_keys("add(ri,rd"), I, "unbalanced parentheses")
        refused(_keys("add(ri,)"), I, "an empty argument")
        refused(_keys("sub(ri,rd,dd)"), I, "sub takes exactly 2 arguments")
        refused(_keys("add('1','2')"), I, "expression without a column")
        refused(_keys("add(ri,nosuch)"), N, "column not found: nosuch")
        d = QueryContext(distinct=["add(ri,nosuch)"], flags=capi.QUERY_FLAG_DISTINCT)
        refused(d, N, "column not found: nosuch")
    finally:
        seg.destroy()


def test_key_kernel_uses_no_scratch():
    """the build leaves hipcc's kernel-resource-usage remarks of pg_kernels_exprkey.hip behind: pg_expr_keys may not spill, and uses no LDS"""
    log = os.path.join(ROOT, "pinot_amd", "csrc", "pg_kernels_exprkey.resources.log")
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
    assert usage.get(("pg_expr_keys", "Scr")) == 0 and usage.get(("pg_expr_keys", "LDS")) == 0, usage
