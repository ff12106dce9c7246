"""The SQL subset parser over time-bucket transforms: the canonical texts ExpressionContext#toString prints, in select lists, GROUP
BY, SELECT DISTINCT and ORDER BY, whatever the spelling; ORDER BY resolution by canonical text; and the SqlErrors that must remain."""
import pytest

from pinot_amd import capi
from pinot_amd.query import SqlError, canonical_expression, parse_sql
from tests import time_transform_cases as cases
from tests import time_transform_model as tm

CANONICAL = [
    ("dateTrunc('day', ts)", "datetrunc('day',ts)"),
    ("DATE_TRUNC( 'day' , ts )", "datetrunc('day',ts)"),
    ("datetrunc('WEEK', ts, 'SECONDS', 'UTC', 'milliseconds')", "datetrunc('WEEK',ts,'SECONDS','UTC','milliseconds')"),   # a literal keeps its case
    ("dateTrunc('hour', ts, 'MILLISECONDS', '+07:09')", "datetrunc('hour',ts,'MILLISECONDS','+07:09')"),
    ("toEpochHours(ts)", "toepochhours(ts)"),
    ("TO_EPOCH_MINUTES_ROUNDED(ts, 5)", "toepochminutesrounded(ts,'5')"),
    ("toEpochMinutesRounded(ts, '5')", "toepochminutesrounded(ts,'5')"),
    ("toEpochDaysBucket(ts, -7)", "toepochdaysbucket(ts,'-7')"),
    ("timeConvert(ts,'MILLISECONDS','DAYS')", "timeconvert(ts,'MILLISECONDS','DAYS')"),
    ("TIMECONVERT( ts , 'milliseconds' , 'days' )", "timeconvert(ts,'milliseconds','days')"),
    ("dateTimeConvert(ts,'1:MILLISECONDS:EPOCH','1:HOURS:EPOCH','1:HOURS')", "datetimeconvert(ts,'1:MILLISECONDS:EPOCH','1:HOURS:EPOCH','1:HOURS')"),
    ("DATE_TIME_CONVERT(ts, 'EPOCH|MILLISECONDS', 'EPOCH|HOURS|2', 'HOURS|2')", "datetimeconvert(ts,'EPOCH|MILLISECONDS','EPOCH|HOURS|2','HOURS|2')"),
    ("dateTrunc('day', a + b)", "datetrunc('day',plus(a,b))"),                  # parsed; the library refuses the value argument
    ("toEpochHours(ts) + 1", "plus(toepochhours(ts),'1')"),                      # parsed; the library refuses the nesting
]


@pytest.mark.parametrize("given,canonical", CANONICAL)
def test_canonical_texts(given, canonical):
    assert canonical_expression(given) == canonical
    q = parse_sql(f"SELECT {given}, g, COUNT(*) FROM t WHERE s < 5 GROUP BY {given}, g ORDER BY {given} DESC, g LIMIT 3")
    assert q.group_by == [canonical, "g"] and q.select_columns == [canonical, "g"] and q.has_group_by
    assert q.order_by == [(canonical, False), ("g", True)]
    assert q.resolved_order_by() == [(capi.ORDER_BY_GROUP_KEY, 0, False), (capi.ORDER_BY_GROUP_KEY, 1, True)]
    d = parse_sql(f"SELECT DISTINCT g, {given} FROM t ORDER BY {given} LIMIT 3")
    assert d.distinct == ["g", canonical] and d.flags & capi.QUERY_FLAG_DISTINCT and d.order_by == [(canonical, True)]


def test_the_parser_prints_what_the_model_and_the_library_read():
    for text, column in cases.ACCEPTED:
        assert canonical_expression(text) == text and tm.columns_of(text) == [column], text
    for given, canonical in cases.SPELLINGS:
        if "+" not in given:   # (a literal with a leading '+' is the library's to read, not SQL's)
            assert canonical_expression(given) == canonical


def test_order_by_names_the_key_in_any_spelling():
    q = parse_sql("SELECT dateTrunc('day', ts), COUNT(*) FROM t GROUP BY dateTrunc('day', ts) ORDER BY DATE_TRUNC( 'day', ts ) DESC, COUNT(*) LIMIT 5")
    assert q.group_by == ["datetrunc('day',ts)"]
    assert q.resolved_order_by() == [(capi.ORDER_BY_GROUP_KEY, 0, False), (capi.ORDER_BY_AGGREGATION, 0, True)]
    # another literal is another key: ORDER BY names no key of the query
    q = parse_sql("SELECT dateTrunc('day', ts), COUNT(*) FROM t GROUP BY dateTrunc('day', ts) ORDER BY dateTrunc('DAY', ts)")
    assert q.resolved_order_by() is None
    with pytest.raises(SqlError):
        parse_sql("SELECT DISTINCT dateTrunc('day', ts) FROM t ORDER BY dateTrunc('week', ts)")


def test_time_functions_elsewhere_parse_and_reach_the_library():
    """in WHERE, inside an aggregation and in a selection the text is spelled and handed over: the library refuses it there"""
    q = parse_sql("SELECT COUNT(*) FROM t WHERE toEpochHours(ts) > 5")
    assert q.filter.predicate.column == "toepochhours(ts)"
    assert parse_sql("SELECT SUM(dateTrunc('day', ts)) FROM t").aggregations[0].column == "datetrunc('day',ts)"
    q = parse_sql("SELECT dateTrunc('day', ts), g FROM t LIMIT 5")
    assert q.flags & capi.QUERY_FLAG_SELECTION and q.selection == ["datetrunc('day',ts)", "g"]


@pytest.mark.parametrize("sql", [
    "SELECT SUM(a * 'x') FROM t",
    "SELECT COUNT(*) FROM t WHERE a + 'x' > 1",
    "SELECT a + 'day', COUNT(*) FROM t GROUP BY a + 'day'",
    "SELECT add(a,'day'), COUNT(*) FROM t GROUP BY add(a,'day')",
    "SELECT dateTrunc('day', ts) + 'x', COUNT(*) FROM t GROUP BY dateTrunc('day', ts) + 'x'",
    "SELECT dateTrunc('day', ts * 'x'), COUNT(*) FROM t GROUP BY dateTrunc('day', ts * 'x')",
    "SELECT dateTrunc('day' ts), COUNT(*) FROM t GROUP BY dateTrunc('day' ts)",
    "SELECT dateTrunc('day', ts, COUNT(*) FROM t",
    "SELECT 'day', COUNT(*) FROM t GROUP BY 'day'",
])
def test_sql_errors_that_remain(sql):
    with pytest.raises(SqlError):
        parse_sql(sql)
