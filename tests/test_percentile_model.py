"""tests/percentile_model.py pinned to the reference: the 16 expected (v1, v2) pairs of InterSegmentAggregationSingleValueQueriesTest#testPercentile
(:379-473, recorded in tests/golden/percentile_expected.json) and their execution statistics over four copies of tests/golden/test_data_sv.npz,
the index formula, Double.compare ordering and the LONG -> double cast.  The SQL front end's four spellings are checked on the way."""
import json
import os

import numpy as np
import pytest

from pinot_amd.executor import NativeSegment, percentile_expand, percentile_final
from pinot_amd.query import SqlError, parse_sql
from tests import percentile_model as pm
from tests.fixtures import SV_FILTER, sv_segment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPECTED = json.load(open(os.path.join(ROOT, "tests", "golden", "percentile_expected.json")))
COPIES = 4   # the inter-segment tests query the same segment four times


@pytest.fixture(scope="module")
def filtered_docs(oracle_api, sv_data):
    seg = NativeSegment(oracle_api, sv_segment(sv_data))
    docs = seg.filter("SELECT COUNT(*) FROM testTable" + SV_FILTER).doc_ids()
    seg.destroy()
    return docs


def _spellings(p):
    return [f"SELECT PERCENTILE{p}(column1) AS v1, PERCENTILE{p}(column3) AS v2 FROM testTable",
            f"SELECT PERCENTILE(column1, {p}) AS v1, PERCENTILE(column3, {p}) AS v2 FROM testTable",
            f"SELECT PERCENTILE(column1, '{p}') AS v1, PERCENTILE(column3, '{p}') AS v2 FROM testTable"]


@pytest.mark.parametrize("p", [50, 90, 95, 99])
@pytest.mark.parametrize("shape", ["none", "filter", "group_by", "filter_group_by"])
def test_reference_goldens(sv_data, filtered_docs, p, shape):
    n = len(sv_data["column1"])
    docs = filtered_docs if "filter" in shape else np.arange(n)
    for sql in _spellings(p):   # the three spellings are one query
        qc = parse_sql(sql + (SV_FILTER if "filter" in shape else "")
                       + (" GROUP BY column9 ORDER BY v1 DESC, v2 DESC LIMIT 1" if "group_by" in shape else ""))
        assert [(a.function, a.column, a.percentile) for a in qc.aggregations] == [("PERCENTILE", "column1", float(p)), ("PERCENTILE", "column3", float(p))]
    cols = [pm.as_doubles(sv_data[c], "INT") for c in ("column1", "column3")]
    if "group_by" in shape:
        groups = pm.group_docs([sv_data["column9"]], docs)
        rows = [tuple(pm.final(np.tile(c[g], COPIES), float(p)) for c in cols) for g in groups.values()]
        got = max(rows)   # ORDER BY v1 DESC, v2 DESC LIMIT 1
        read = ["column9", "column1", "column3"]
    else:
        got = tuple(pm.final(np.tile(c[docs], COPIES), float(p)) for c in cols)
        read = ["column1", "column3"]
    assert list(got) == EXPECTED["values"][str(p)][shape]
    scanned, post = pm.statistics(len(docs) * COPIES, read)
    want = EXPECTED["stats"][shape]
    assert (scanned, post, n * COPIES) == (want[0], want[2], want[3])


@pytest.mark.parametrize("n", [1, 2, 3, 7])
@pytest.mark.parametrize("p", [0, 33.3, 50, 99.9, 100])
def test_index_formula(n, p):
    """sorted[(int)((long) n * p / 100)], the last value for p = 100: worked out by hand per case in exact rational arithmetic — none of these
    products lies within a rounding error of an integer, so the truncated double equals the truncated rational"""
    from fractions import Fraction
    want = n - 1 if p == 100 else int(Fraction(n) * Fraction(str(p)) / 100)
    assert pm.index_of(n, float(p)) == want
    assert 0 <= want < n
    values = np.arange(10, 10 + n, dtype=np.float64)[::-1]
    assert pm.final(values, float(p)) == 10.0 + want
    assert percentile_final(pm.runs(values), float(p)) == 10.0 + want


def test_double_compare_order():
    nan2 = np.array([0x7FF8000000000123], dtype=np.uint64).view(np.float64)[0]
    v = np.array([0.0, np.nan, -0.0, 1.0, -np.inf, nan2, np.inf, -1.0, 0.0], dtype=np.float64)
    s = pm.sort_doubles(v)
    assert np.array_equal(s[:7], np.array([-np.inf, -1.0, -0.0, 0.0, 0.0, 1.0, np.inf]))
    assert np.signbit(s[2]) and not np.signbit(s[3]) and np.isnan(s[7]) and np.isnan(s[8])
    values, counts = pm.runs(v)
    assert counts.tolist() == [1, 1, 1, 2, 1, 1, 2] and np.isnan(values[-1])   # -0.0 and 0.0 are two runs, the NaNs one
    assert np.isnan(pm.final(v, 100.0)) and pm.final(v, 0.0) == -np.inf
    assert pm.same_double(pm.final(v, 25.0), -0.0) and not pm.same_double(-0.0, 0.0)
    assert pm.final(np.zeros(0), 50.0) == float("-inf")   # Double.NEGATIVE_INFINITY over no value
    assert np.array_equal(pm.order_keys(percentile_expand((values, counts))), pm.order_keys(s))


def test_long_above_2_53_is_cast_not_kept():
    big = 2**53 + 1   # not a double: (double) rounds to nearest even, 2^53
    d = pm.as_doubles([big, 2**53 + 3, -5], "LONG")
    assert d.tolist() == [float(2**53), float(2**53 + 4), -5.0]
    assert pm.final(d, 50.0) == float(2**53)
    # the cast is monotone: selecting by value order and casting at the end gives the same answer
    longs = np.array([big, 2**53 + 3, -5, 2**53, 2**62 + 12345], dtype=np.int64)
    for p in (0.0, 20.0, 50.0, 99.9, 100.0):
        assert pm.final(pm.as_doubles(longs, "LONG"), p) == float(np.sort(longs)[pm.index_of(longs.size, p)])
    assert pm.as_doubles(np.array([0.1], dtype=np.float32), "FLOAT")[0] == float(np.float32(0.1))   # widened exactly


def test_parser_spellings_and_rejections():
    q = parse_sql("SELECT g, COUNT(*), PERCENTILE(a, 95), PERCENTILE(a, 99.9), PERCENTILE(b, '50'), PERCENTILE90(a) FROM t GROUP BY g "
                  "ORDER BY PERCENTILE(a, 99.9) DESC, percentile90(a), g LIMIT 3")
    assert [(a.function, a.column, a.percentile) for a in q.aggregations] == [
        ("COUNT", None, None), ("PERCENTILE", "a", 95.0), ("PERCENTILE", "a", 99.9), ("PERCENTILE", "b", 50.0), ("PERCENTILE", "a", 90.0)]
    from pinot_amd import capi
    assert q.resolved_order_by() == [(capi.ORDER_BY_AGGREGATION, 2, False), (capi.ORDER_BY_AGGREGATION, 4, True), (capi.ORDER_BY_GROUP_KEY, 0, True)]
    assert parse_sql("SELECT PERCENTILE(a, 0), PERCENTILE100(a) FROM t").aggregations[1].percentile == 100.0
    for bad in ("SELECT PERCENTILE(a, 100.5) FROM t", "SELECT PERCENTILE(a, -1) FROM t", "SELECT PERCENTILE101(a) FROM t",
                "SELECT PERCENTILE(a) FROM t", "SELECT PERCENTILE(a, 'x') FROM t", "SELECT PERCENTILE(*, 5) FROM t",
                "SELECT PERCENTILEMV(a, 5) FROM t", "SELECT PERCENTILETDIGEST(a, 5) FROM t"):
        with pytest.raises(SqlError):
            parse_sql(bad)


def test_cquery_carries_the_percentiles():
    from pinot_amd import capi
    from pinot_amd.query import CQuery
    cq = CQuery(parse_sql("SELECT COUNT(*), PERCENTILE(a, 99.9), PERCENTILE50(b) FROM t"))
    assert cq.query.n_aggregations == 3 and [cq.query.agg_params[i] for i in range(3)] == [0.0, 99.9, 50.0]
    assert cq.query.aggregations[1].function == capi.AGG_FUNCTIONS["PERCENTILE"] == 16
    assert not CQuery(parse_sql("SELECT COUNT(*), SUM(a) FROM t")).query.agg_params   # NULL without a PERCENTILE
