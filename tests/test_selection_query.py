"""Selection queries in the Python layer (no GPU): parsing of SELECT * / select lists into a selection, the output columns of
SelectionOperatorUtils#extractExpressions (:83-125), the C query record and the header's flag."""
import os
import re

import pytest

from pinot_amd import capi
from pinot_amd.query import CQuery, SqlError, parse_sql

COLS = ["column9", "column1", "$docId", "column11", "column5", "daysSinceEpoch", "column3"]


def test_flag_value_matches_header():
    assert capi.QUERY_FLAG_SELECTION == 0x100
    header = open(os.path.join(capi.REPO_ROOT, "include", "pinot_gpu.h")).read()
    m = re.search(r"#define PG_QUERY_FLAG_SELECTION (0x[0-9a-fA-F]+)", header)
    assert m and int(m.group(1), 16) == capi.QUERY_FLAG_SELECTION
    flags = [int(v, 16) for v in re.findall(r"#define PG_QUERY_FLAG_\w+ (0x[0-9a-fA-F]+)", header)]
    assert flags.count(capi.QUERY_FLAG_SELECTION) == 1   # no other flag shares the bit


def test_select_star_is_a_selection():
    q = parse_sql("SELECT * FROM testTable LIMIT 10")
    assert q.selection == ["*"] and q.flags & capi.QUERY_FLAG_SELECTION
    assert q.aggregations == [] and q.group_by == [] and q.distinct == []
    # every column not starting with '$', sorted by name
    assert q.extract_expressions(COLS) == ["column1", "column11", "column3", "column5", "column9", "daysSinceEpoch"]


def test_select_list_is_a_selection():
    q = parse_sql("SELECT column1, column5, column11 FROM testTable WHERE column1 > 5 LIMIT 7")
    assert q.selection == ["column1", "column5", "column11"] and q.limit == 7
    assert q.flags & capi.QUERY_FLAG_SELECTION
    assert q.extract_expressions(COLS) == ["column1", "column5", "column11"]


def test_default_limit_is_ten():
    assert parse_sql("SELECT column1 FROM t").limit == 10


@pytest.mark.parametrize("sql,want", [
    # ORDER BY expressions first, then the select list without them
    ("SELECT column1, column5, column11 FROM t ORDER BY column6, column1 LIMIT 10", ["column6", "column1", "column5", "column11"]),
    ("SELECT column1, column1, column5 FROM t LIMIT 10", ["column1", "column5"]),                       # deduped
    ("SELECT column5 FROM t ORDER BY column5 DESC, column5 LIMIT 3", ["column5"]),                       # a repeated ORDER BY column once
    ("SELECT * FROM t ORDER BY daysSinceEpoch DESC LIMIT 3",
     ["daysSinceEpoch", "column1", "column11", "column3", "column5", "column9"]),
    # LIMIT 0: the ORDER BY expressions are ignored (EmptySelectionOperator)
    ("SELECT column1, column5 FROM t ORDER BY column6 LIMIT 0", ["column1", "column5"]),
])
def test_extract_expressions_order(sql, want):
    assert parse_sql(sql).extract_expressions(COLS) == want


def test_c_record():
    q = parse_sql("SELECT column1, column5 FROM t ORDER BY column6 DESC, column1 LIMIT 25")
    cq = CQuery(q, COLS)
    r = cq.query
    assert r.flags & capi.QUERY_FLAG_SELECTION and not r.flags & capi.QUERY_FLAG_DISTINCT
    assert r.n_aggregations == 0 and r.limit == 25
    assert [r.group_by_columns[i].decode() for i in range(r.n_group_by)] == ["column6", "column1", "column5"]
    assert r.n_order_by == 2
    assert (r.order_by[0].kind, r.order_by[0].index, r.order_by[0].ascending) == (capi.ORDER_BY_GROUP_KEY, 0, 0)
    assert (r.order_by[1].kind, r.order_by[1].index, r.order_by[1].ascending) == (capi.ORDER_BY_GROUP_KEY, 1, 1)
    q0 = parse_sql("SELECT column1 FROM t ORDER BY column6 LIMIT 0")
    assert CQuery(q0, COLS).query.n_order_by == 0


def test_select_star_needs_the_segment():
    with pytest.raises(SqlError):
        CQuery(parse_sql("SELECT * FROM t LIMIT 1"))
    with pytest.raises(SqlError):
        parse_sql("SELECT *, column1 FROM t LIMIT 1")


def test_other_shapes_are_not_selections():
    for sql in ("SELECT COUNT(*) FROM t", "SELECT column1, COUNT(*) FROM t GROUP BY column1", "SELECT DISTINCT column1 FROM t LIMIT 5",
                "SELECT column1 FROM t GROUP BY column1"):
        q = parse_sql(sql)
        assert q.selection == [] and not q.flags & capi.QUERY_FLAG_SELECTION, sql
        assert not CQuery(q).query.flags & capi.QUERY_FLAG_SELECTION, sql
