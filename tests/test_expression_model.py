"""tests/expression_model.py pinned to the reference — TransformQueriesTest#testTransformWithAvgInnerSegment's seven AvgPairs over its 10-row
segment and ForwardIndexDisabledSingleValueQueriesTest's MAX(ADD(column1, column9)) over tests/golden/test_data_sv.npz, both recorded in
tests/golden/expression_expected.json — and the SQL front end's expression forms: infix precedence and parentheses, the aliases, multi-argument
ADD / MULT, the canonical text, and what must stay as it was (COUNT(*), SELECT *, the rejects)."""
import json
import os

import numpy as np
import pytest

from pinot_amd import capi
from pinot_amd.query import CQuery, SqlError, parse_sql
from tests import expression_model as em

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPECTED = json.load(open(os.path.join(ROOT, "tests", "golden", "expression_expected.json")))


@pytest.mark.parametrize("case", EXPECTED["transform_avg"], ids=[c[0].split("AVG")[1].split(" FROM")[0] for c in EXPECTED["transform_avg"]])
def test_transform_queries_goldens(case):
    sql, want_sum, want_count = case
    data, schema = em.transform_queries_segment()
    qc = parse_sql(sql)
    assert len(qc.aggregations) == 1 and qc.aggregations[0].function == "AVG"
    got = em.aggregate("AVG", em.evaluate(qc.aggregations[0].column, data, schema))
    assert got == (want_sum, want_count)


def test_max_add_golden(sv_data):
    want = EXPECTED["max_add_column1_column9"]
    qc = parse_sql(want["query"])
    assert qc.aggregations[0].column == "add(column1,column9)"
    schema = {"column1": "INT", "column9": "INT"}
    assert em.aggregate("MAX", em.evaluate(qc.aggregations[0].column, sv_data, schema)) == want["value"]
    assert float(np.max(sv_data["column1"].astype(np.float64) + sv_data["column9"].astype(np.float64))) == want["value"]
    n = len(sv_data["column1"])
    assert n * len(em.columns_of(qc.aggregations[0].column)) == want["num_entries_scanned_post_filter_per_segment"]
    assert want["num_entries_scanned_post_filter_per_segment"] * want["segments"] == want["num_entries_scanned_post_filter"]


def _col(sql):
    return parse_sql(sql).aggregations[0].column


def test_infix_precedence_and_parentheses():
    assert _col("SELECT SUM(price * quantity) FROM t") == "times(price,quantity)"
    assert _col("SELECT SUM(a + b * c) FROM t") == "plus(a,times(b,c))"
    assert _col("SELECT SUM((a + b) * c) FROM t") == "times(plus(a,b),c)"
    assert _col("SELECT SUM(a - b - c) FROM t") == "minus(minus(a,b),c)"          # left-associative
    assert _col("SELECT SUM(a / b / c) FROM t") == "divide(divide(a,b),c)"
    assert _col("SELECT SUM(a - (b - c)) FROM t") == "minus(a,minus(b,c))"
    assert _col("SELECT SUM(a * b + c / d - e) FROM t") == "minus(plus(times(a,b),divide(c,d)),e)"
    assert _col("SELECT SUM(((a))) FROM t") == "a"                                # a lone column stays a plain column
    assert _col("SELECT AVG(a - b) FROM t") == "minus(a,b)"


def test_literals_print_quoted_and_a_leading_minus_after_an_operand_subtracts():
    assert _col("SELECT SUM(price * 1.5) FROM t") == "times(price,'1.5')"
    assert _col("SELECT SUM(mult(price,'1.5')) FROM t") == "mult(price,'1.5')"
    assert _col("SELECT SUM(2 * a) FROM t") == "times('2',a)"
    assert _col("SELECT SUM(a -5) FROM t") == "minus(a,'5')"
    assert _col("SELECT SUM(a-5*b) FROM t") == "minus(a,times('5',b))"
    assert _col("SELECT SUM(a - -5) FROM t") == "minus(a,'-5')"
    assert _col("SELECT SUM(-5 + a) FROM t") == "plus('-5',a)"
    assert _col("SELECT SUM(a * 1e3) FROM t") == "times(a,'1e3')"
    f = parse_sql("SELECT SUM(a - 1) FROM t WHERE b > -5 AND c BETWEEN -3 AND -1").filter    # filters keep their negative literals
    assert [c.predicate.lower for c in f.children] == ["-5", "-3"] and f.children[1].predicate.upper == "-1"


def test_function_forms_and_aliases():
    assert _col("SELECT MAX(ADD(column1, column9)) FROM t") == "add(column1,column9)"
    assert _col("SELECT MAX(add(column1,column9)) FROM t") == "add(column1,column9)"
    assert _col("SELECT SUM(PLUS(a, b)) FROM t") == "plus(a,b)"
    assert _col("SELECT SUM(Minus(a, Times(b, DIVIDE(c, d)))) FROM t") == "minus(a,times(b,divide(c,d)))"
    assert _col("SELECT SUM(ADD(a, 5, b)) FROM t") == "add(a,'5',b)"
    assert _col("SELECT SUM(ADD(a, b) * SUB(c, 2)) FROM t") == "times(add(a,b),sub(c,'2'))"
    data = {"a": np.array([1, -2], dtype=np.int32), "b": np.array([0.5, 4.0])}
    schema = {"a": "INT", "b": "DOUBLE"}
    for alias, fn in (("plus", "add"), ("minus", "sub"), ("times", "mult"), ("divide", "div")):
        assert np.array_equal(em.evaluate(f"{alias}(a,b)", data, schema), em.evaluate(f"{fn}(a,b)", data, schema))


def test_multi_argument_order():
    """ADD(a, 5, b) is ((0.0 + 5) + a) + b: the literals first, then the other arguments in their order"""
    data = {"a": np.array([2.0**53, -0.0, 1e308]), "b": np.array([1.0, -0.0, 1e308])}
    schema = {"a": "DOUBLE", "b": "DOUBLE"}
    a, b = data["a"], data["b"]
    with np.errstate(all="ignore"):
        assert np.array_equal(em.evaluate("add(a,'5',b)", data, schema), ((0.0 + 5.0) + a) + b)
        assert np.array_equal(em.evaluate("add(a,b,'5')", data, schema), ((0.0 + 5.0) + a) + b)          # not (a + b) + 5
        big = {"a": np.array([1e16]), "b": np.array([-1e16])}
        assert em.evaluate("add(a,b,'1')", big, schema)[0] == 0.0 and (big["a"][0] + big["b"][0]) + 1.0 == 1.0   # (1 + 1e16) rounds to 1e16
        v = em.evaluate("add(a,b)", data, schema)
        assert v[1] == 0.0 and not np.signbit(v[1])                                                      # 0.0 + -0.0 + -0.0 = +0.0
        m = em.evaluate("mult(a,'2','0.25',b)", data, schema)
        assert np.array_equal(m, ((1.0 * 2.0 * 0.25) * a) * b) and np.signbit(em.evaluate("mult(a,'-1')", data, schema)[1]) is np.False_
        assert np.array_equal(em.evaluate("sub('1',a)", data, schema), 1.0 - a) and np.array_equal(em.evaluate("div(a,'3')", data, schema), a / 3.0)
    assert em.evaluate("add(sub('3','1'),a)", data, schema)[1] == 2.0        # a literal-only call folds to a literal
    assert em.columns_of("add(div(a,b),div(c,a))") == ["a", "b", "c"]


def test_long_and_float_leaves():
    data = {"l": np.array([2**53 + 1, 2**53 + 3], dtype=np.int64), "f": np.array([0.1, 0.1], dtype=np.float32)}
    schema = {"l": "LONG", "f": "FLOAT"}
    assert em.evaluate("add(l,'0')", data, schema).tolist() == [float(2**53), float(2**53 + 4)]     # (double) rounds to nearest even
    assert em.evaluate("mult(f,'1')", data, schema)[0] == float(np.float32(0.1))                   # widened exactly
    assert em.aggregate("SUM", em.evaluate("add(l,f)", data, schema)) == float(2**54 + 4)


def test_aggregations_and_their_defaults():
    v = np.array([3.0, -1.5, 2.0**60, -(2.0**60), 1e-3])
    assert em.aggregate("SUM", v) == 1.501 and sum(v.tolist()) != 1.501           # exact, rounded once
    assert em.aggregate("MIN", v) == -(2.0**60) and em.aggregate("MAX", v) == 2.0**60
    assert em.aggregate("AVG", v) == (1.501, 5) and em.aggregate("MINMAXRANGE", v) == (-(2.0**60), 2.0**60)
    none = np.zeros(0)
    assert em.aggregate("SUM", none) == 0.0 and em.aggregate("MIN", none) == float("inf") and em.aggregate("MAX", none) == float("-inf")
    assert em.aggregate("AVG", none) == (0.0, 0)


def test_what_stays_as_it_was():
    q = parse_sql("SELECT COUNT(*), SUM(a), COUNT(b) FROM t")
    assert [(a.function, a.column) for a in q.aggregations] == [("COUNT", None), ("SUM", "a"), ("COUNT", "b")]
    q = parse_sql("SELECT * FROM t WHERE a > 3 LIMIT 5")
    assert q.selection == ["*"] and not q.aggregations and q.flags & capi.QUERY_FLAG_SELECTION
    with pytest.raises(SqlError):
        parse_sql("SELECT *, column1 FROM t")
    q = parse_sql("SELECT DISTINCTCOUNTHLL(a, 12), PERCENTILE(b, 99.9) FROM t")
    assert (q.aggregations[0].log2m, q.aggregations[1].percentile) == (12, 99.9)


def test_rejects():
    for bad in ("SELECT SUM(a +) FROM t", "SELECT SUM(a * 'x') FROM t", "SELECT SUM(5) FROM t", "SELECT SUM('5') FROM t", "SELECT SUM(-a) FROM t",
                "SELECT SUM((a + b) FROM t", "SELECT SUM(a + b)) FROM t", "SELECT SUM(ADD(a, )) FROM t", "SELECT SUM(ADD(, a)) FROM t",
                "SELECT SUM(a b) FROM t", "SELECT SUM(* a) FROM t", "SELECT SUM(a + *) FROM t", "SELECT PERCENTILE(*, 5) FROM t", "SELECT SUM() FROM t"):
        with pytest.raises(SqlError):
            parse_sql(bad)


def test_order_by_names_an_expression_aggregation_by_its_canonical_text():
    q = parse_sql("SELECT g, COUNT(*), SUM(a * b), MAX(ADD(a, 5, b)) FROM t GROUP BY g ORDER BY SUM(a*b) DESC, max(add(a,'5',b)), SUM(times(a, b)), g LIMIT 3")
    A, K = capi.ORDER_BY_AGGREGATION, capi.ORDER_BY_GROUP_KEY
    assert q.resolved_order_by() == [(A, 1, False), (A, 2, True), (A, 1, True), (K, 0, True)]
    assert parse_sql("SELECT g, SUM(a * b) FROM t GROUP BY g ORDER BY SUM(a + b)").resolved_order_by() is None   # another expression


def test_cquery_carries_the_text():
    cq = CQuery(parse_sql("SELECT SUM(price * quantity), COUNT(*) FROM t"))
    assert cq.query.aggregations[0].column == b"times(price,quantity)" and cq.query.aggregations[0].function == capi.AGG_FUNCTIONS["SUM"]
    assert not cq.query.aggregations[1].column and not cq.query.agg_params
