"""Arithmetic expressions as GROUP BY / DISTINCT keys in the SQL front end and the query record (no GPU): parse_sql's canonical texts, ORDER BY
matched against a key by canonical text whatever its spelling, and CQuery carrying the text in group_by_columns."""
import pytest

from pinot_amd import capi
from pinot_amd.query import CQuery, QueryContext, AggregationSpec, SqlError, canonical_expression, parse_sql

UDF = "SELECT sub(column1, 100000), COUNT(*) FROM testTable GROUP BY sub(column1, 100000) ORDER BY {} LIMIT 3"


def test_group_by_expressions_are_canonical():
    q = parse_sql("SELECT sub(column1, 100000), COUNT(*) FROM testTable GROUP BY sub(column1, 100000)")
    assert q.group_by == ["sub(column1,'100000')"] and q.select_columns == ["sub(column1,'100000')"] and q.has_group_by
    assert [a.function for a in q.aggregations] == ["COUNT"] and not q.distinct and not q.selection
    q = parse_sql("SELECT a + b * 2, (a - 1) / b, c, SUM(d) FROM t GROUP BY a + b * 2, (a - 1) / b, c")
    assert q.group_by == ["plus(a,times(b,'2'))", "divide(minus(a,'1'),b)", "c"]
    assert q.select_columns == q.group_by
    q = parse_sql("SELECT ADD(intColumn, floatColumn), stringColumn FROM t GROUP BY ADD( intColumn ,floatColumn), stringColumn")
    assert q.group_by == ["add(intColumn,floatColumn)", "stringColumn"]
    q = parse_sql("SELECT a, COUNT(*) FROM t GROUP BY MULT(a, '1.5', b), a -1, div(1, a)")
    assert q.group_by == ["mult(a,'1.5',b)", "minus(a,'1')", "div('1',a)"]
    # plain columns stay what they were
    q = parse_sql("SELECT a, b, COUNT(*), SUM(a * b) FROM t WHERE a * b > 3 GROUP BY a, b ORDER BY SUM(a * b) DESC, a LIMIT 4")
    assert q.group_by == ["a", "b"] and q.select_columns == ["a", "b"]
    assert q.resolved_order_by() == [(capi.ORDER_BY_AGGREGATION, 1, False), (capi.ORDER_BY_GROUP_KEY, 0, True)]
    with pytest.raises(SqlError):
        parse_sql("SELECT COUNT(*) FROM t GROUP BY 5")
    with pytest.raises(SqlError):
        parse_sql("SELECT COUNT(*) FROM t GROUP BY a +")


def test_distinct_expressions_are_canonical():
    q = parse_sql("SELECT DISTINCT ADD(intColumn, floatColumn), stringColumn FROM testTable WHERE longColumn < 60 "
                  "ORDER BY stringColumn DESC, ADD(intColumn, floatColumn) ASC LIMIT 10")
    assert q.distinct == ["add(intColumn,floatColumn)", "stringColumn"] and q.flags & capi.QUERY_FLAG_DISTINCT
    assert q.order_by == [("stringColumn", False), ("add(intColumn,floatColumn)", True)] and q.limit == 10
    q = parse_sql("SELECT DISTINCT a + 1, b FROM t ORDER BY a+1 DESC")
    assert q.distinct == ["plus(a,'1')", "b"] and q.order_by == [("plus(a,'1')", False)]
    with pytest.raises(SqlError):
        parse_sql("SELECT DISTINCT a + 1 FROM t ORDER BY a + 2")        # an ORDER BY expression must be one of the DISTINCT expressions
    # without aggregations, GROUP BY or DISTINCT an expression makes a selection (which the library leaves to the Java plan)
    q = parse_sql("SELECT a + 1, b FROM t LIMIT 5")
    assert q.selection == ["plus(a,'1')", "b"] and q.flags & capi.QUERY_FLAG_SELECTION


@pytest.mark.parametrize("spelling", ["sub(column1, 100000)", "SUB(   column1, 100000\t)", "Sub(column1,'100000')", "sub( column1 , 100000 ) DESC"])
def test_order_by_matches_a_key_by_canonical_text(spelling):
    q = parse_sql(UDF.format(spelling))
    desc = spelling.endswith("DESC")
    assert q.order_by == [("sub(column1,'100000')", not desc)]
    assert q.resolved_order_by() == [(capi.ORDER_BY_GROUP_KEY, 0, not desc)]


def test_order_by_of_a_hand_built_query_matches_by_canonical_text():
    q = QueryContext(group_by=["g", "sub(column1,'100000')"], aggregations=[AggregationSpec("COUNT")], has_group_by=True,
                     order_by=[("SUB(   column1, 100000\t)", False), ("column1 - 100000", True), ("COUNT(*)", True)])
    assert canonical_expression("SUB(   column1, 100000\t)") == "sub(column1,'100000')"
    assert canonical_expression("column1 - 100000") == "minus(column1,'100000')"       # infix is another function: another key
    assert canonical_expression("g") == "g" and canonical_expression("COUNT(*)") is None and canonical_expression("5") is None
    assert q.resolved_order_by() is None
    q.order_by = q.order_by[:1] + q.order_by[2:]
    assert q.resolved_order_by() == [(capi.ORDER_BY_GROUP_KEY, 1, False), (capi.ORDER_BY_AGGREGATION, 0, True)]
    q.group_by.append("minus(column1,'100000')")
    q.order_by = [("column1 - 100000", True)]
    assert q.resolved_order_by() == [(capi.ORDER_BY_GROUP_KEY, 2, True)]


def test_cquery_carries_the_text():
    q = parse_sql(UDF.format("SUB(   column1, 100000\t)"))
    q.min_segment_group_trim_size = 1
    cq = CQuery(q)
    assert cq.query.n_group_by == 1 and cq.query.group_by_columns[0] == b"sub(column1,'100000')"
    assert cq.query.n_aggregations == 1 and cq.query.aggregations[0].function == capi.AGG_FUNCTIONS["COUNT"]
    assert cq.query.n_order_by == 1
    ob = cq.query.order_by[0]
    assert (ob.kind, ob.index, ob.ascending) == (capi.ORDER_BY_GROUP_KEY, 0, 1) and cq.query.limit == 3
    d = CQuery(parse_sql("SELECT DISTINCT ADD(i, f), s FROM t ORDER BY s DESC, add(i,f) LIMIT 10"))
    assert [d.query.group_by_columns[j] for j in range(d.query.n_group_by)] == [b"add(i,f)", b"s"]
    assert d.query.flags & capi.QUERY_FLAG_DISTINCT and d.query.n_aggregations == 0
    assert [(d.query.order_by[i].index, d.query.order_by[i].ascending) for i in range(d.query.n_order_by)] == [(1, 0), (0, 1)]
    assert d.output_columns == ["add(i,f)", "s"]
