"""CASE WHEN in the SQL front end (pinot_amd/query.py): every spelling gives the canonical text ExpressionContext#toString
prints — case(when1,then1,...,else) over equals / notequals / greaterthan / greaterthanorequal / lessthan / lessthanorequal and and / or / not,
literals quoted, an omitted ELSE as 'null' —, what a WHEN does not take raises a SqlError naming it, ORDER BY resolves an aggregation over a
CASE by its canonical text, and the shim carries the text as the column string of a plain aggregation record."""
import os
import subprocess

import pytest

from pinot_amd import capi
from pinot_amd.query import CQuery, SqlError, canonical_expression, parse_sql

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _columns(sql):
    return [a.column for a in parse_sql(sql).aggregations]


SPELLINGS = [
    ("SUM(CASE WHEN status = 'ok' THEN 1 ELSE 0 END)", "case(equals(status,'ok'),'1','0')"),
    ("sum(case when a > 100 then price * qty else 0 end)", "case(greaterthan(a,'100'),times(price,qty),'0')"),
    ("MIN(CASE WHEN a > 5000 THEN a ELSE 9999999 END)", "case(greaterthan(a,'5000'),a,'9999999')"),
    ("SUM(Case  When a>=1 Then 1 When a<=-1 Then -1 When a<>0 Then 2 When a!=3 Then 3 When a<4 Then 4 Else 0 End)",
     "case(greaterthanorequal(a,'1'),'1',lessthanorequal(a,'-1'),'-1',notequals(a,'0'),'2',notequals(a,'3'),'3',lessthan(a,'4'),'4','0')"),
    ("SUM(CASE WHEN a > 5 THEN a END)", "case(greaterthan(a,'5'),a,'null')"),                              # no ELSE ...
    ("SUM(CASE WHEN a > 5 THEN a ELSE NULL END)", "case(greaterthan(a,'5'),a,'null')"),                    # ... and ELSE NULL
    ("SUM(case(greater_than(a, 5), a, 0))", "case(greaterthan(a,'5'),a,'0')"),                             # the function forms
    ("SUM(CASE(GREATERTHAN(a,'5'),a,'0'))", "case(greaterthan(a,'5'),a,'0')"),
    ("SUM(case(and(equals(s,'x y'),not(less_than_or_equal(a,b))),a,'null'))", "case(and(equals(s,'x y'),not(lessthanorequal(a,b))),a,'null')"),
    ("SUM(CASE WHEN 5 < a THEN 1 ELSE 0 END)", "case(lessthan('5',a),'1','0')"),                           # no rewrite: the literal stays on the left
    ("SUM(CASE WHEN a > b THEN 1 ELSE 0 END)", "case(greaterthan(a,b),'1','0')"),                          # ... and a > b is no minus(a,b) > 0
    ("SUM(CASE WHEN 'ok' <> status THEN 1 ELSE 0 END)", "case(notequals('ok',status),'1','0')"),
    ("SUM(CASE WHEN a + b > 2 * c THEN a - 1 ELSE -1 END)", "case(greaterthan(plus(a,b),times('2',c)),minus(a,'1'),'-1')"),
    ("SUM(CASE WHEN (a + b) * 2 > 5 THEN 1 ELSE 0 END)", "case(greaterthan(times(plus(a,b),'2'),'5'),'1','0')"),   # a parenthesised operand ...
    ("SUM(CASE WHEN (a > 5) THEN 1 ELSE 0 END)", "case(greaterthan(a,'5'),'1','0')"),                      # ... and a parenthesised condition
    ("SUM(CASE WHEN a > 1 AND b > 2 AND c > 3 THEN 1 ELSE 0 END)", "case(and(greaterthan(a,'1'),greaterthan(b,'2'),greaterthan(c,'3')),'1','0')"),
    ("SUM(CASE WHEN a > 1 AND (b > 2 AND (c > 3 AND d > 4)) THEN 1 ELSE 0 END)",
     "case(and(greaterthan(a,'1'),greaterthan(b,'2'),greaterthan(c,'3'),greaterthan(d,'4')),'1','0')"),    # nested ANDs are one n-ary and
    ("SUM(CASE WHEN a > 1 OR (b > 2 OR c > 3) OR d > 4 THEN 1 ELSE 0 END)",
     "case(or(greaterthan(a,'1'),greaterthan(b,'2'),greaterthan(c,'3'),greaterthan(d,'4')),'1','0')"),
    ("SUM(CASE WHEN a > 1 OR b > 2 AND c > 3 THEN 1 ELSE 0 END)", "case(or(greaterthan(a,'1'),and(greaterthan(b,'2'),greaterthan(c,'3'))),'1','0')"),   # AND binds tighter
    ("SUM(CASE WHEN (a > 1 OR b > 2) AND NOT c > 3 THEN 1 ELSE 0 END)", "case(and(or(greaterthan(a,'1'),greaterthan(b,'2')),not(greaterthan(c,'3'))),'1','0')"),
    ("SUM(CASE WHEN NOT (a > 1 AND NOT b > 2) THEN 1 ELSE 0 END)", "case(not(and(greaterthan(a,'1'),not(greaterthan(b,'2')))),'1','0')"),
    ("SUM(CASE WHEN a > 1 THEN CASE WHEN b > 2 THEN b END ELSE CASE WHEN c > 3 THEN c ELSE 0 END END)",
     "case(greaterthan(a,'1'),case(greaterthan(b,'2'),b,'null'),case(greaterthan(c,'3'),c,'0'))"),        # nested
    ("SUM(2 * CASE WHEN a > 1 THEN a ELSE 0 END + 1)", "plus(times('2',case(greaterthan(a,'1'),a,'0')),'1')"),   # inside arithmetic
    ("AVG(mult(case when a > 1 then 1 else 0 end, m))", "mult(case(greaterthan(a,'1'),'1','0'),m)"),
    ("SUM(CASE WHEN s = '7' THEN 1 ELSE 0 END)", "case(equals(s,'7'),'1','0')"),
    ("SUM(CASE WHEN a = 1e3 THEN 1.5 ELSE 0.25 END)", "case(equals(a,'1e3'),'1.5','0.25')"),
]


@pytest.mark.parametrize("sql,text", SPELLINGS, ids=[s[0][:48] for s in SPELLINGS])
def test_spellings(sql, text):
    assert _columns(f"SELECT {sql} FROM t") == [text]
    inner = sql[sql.index("(") + 1:-1]
    assert canonical_expression(inner) == text
    assert canonical_expression(text) == text            # the canonical text is a spelling of itself


def test_the_query_keeps_its_other_parts():
    qc = parse_sql("SELECT g, SUM(CASE WHEN a > 5 THEN a ELSE 0 END) AS big, COUNT(*) FROM t WHERE s < 5 GROUP BY g LIMIT 7")
    assert qc.group_by == ["g"] and [a.function for a in qc.aggregations] == ["SUM", "COUNT"] and qc.limit == 7 and qc.filter is not None
    cq = CQuery(qc)                                      # ... and marshals like any aggregation over an expression
    assert cq.ptr() is not None
    # a CASE where a key or a filter's left-hand side stands is parsed to its text too: the library refuses it there, in its own words
    qc = parse_sql("SELECT CASE WHEN a > 5 THEN 1 ELSE 0 END, COUNT(*) FROM t WHERE CASE WHEN a > 5 THEN a ELSE 0 END > 3 GROUP BY CASE WHEN a > 5 THEN 1 ELSE 0 END")
    assert qc.group_by == ["case(greaterthan(a,'5'),'1','0')"] == qc.select_columns
    assert qc.filter.predicate.column == "case(greaterthan(a,'5'),a,'0')"


ERRORS = [
    ("CASE WHEN a IN (1, 2) THEN 1 ELSE 0 END", "IN inside a WHEN"),
    ("CASE WHEN a NOT IN (1, 2) THEN 1 ELSE 0 END", "IN inside a WHEN"),
    ("CASE WHEN a BETWEEN 1 AND 2 THEN 1 ELSE 0 END", "BETWEEN inside a WHEN"),
    ("CASE WHEN (a BETWEEN 1 AND 2) OR a > 7 THEN 1 ELSE 0 END", "BETWEEN inside a WHEN"),
    ("CASE WHEN s LIKE 'k%' THEN 1 ELSE 0 END", "LIKE inside a WHEN"),
    ("CASE WHEN a IS NULL THEN 1 ELSE 0 END", "IS [NOT] NULL inside a WHEN"),
    ("CASE WHEN NOT a IS NOT NULL THEN 1 ELSE 0 END", "IS [NOT] NULL inside a WHEN"),
    ("CASE WHEN s > 'k' THEN 1 ELSE 0 END", "= and <> compare strings"),
    ("CASE WHEN 1 = 1 THEN 1 ELSE 0 END", "a comparison of two literals"),
    ("CASE WHEN 'a' = 'b' THEN 1 ELSE 0 END", "a comparison of two literals"),
    ("CASE WHEN a THEN 1 ELSE 0 END", "expected a comparison inside a WHEN"),
    ("CASE WHEN a > 1 THEN 'big' ELSE 'small' END", "is not a number"),
    ("CASE WHEN a > 1 THEN 1 ELSE 0", "expected END"),
    ("CASE WHEN a > 1 ELSE 0 END", "expected THEN"),
    ("CASE WHEN s = 'it''s' THEN 1 ELSE 0 END", "holds a quote"),
]


@pytest.mark.parametrize("inner,message", ERRORS, ids=[e[1] + str(i) for i, e in enumerate(ERRORS)])
def test_sql_errors(inner, message):
    with pytest.raises(SqlError) as e:
        parse_sql(f"SELECT SUM({inner}) FROM t")
    assert message in str(e.value)
    assert canonical_expression(inner) is None


def test_order_by_resolves_a_case_aggregation():
    qc = parse_sql("SELECT g, SUM(CASE WHEN status = 'ok' THEN 1 ELSE 0 END), MIN(CASE WHEN a > 5000 THEN a ELSE 9999999 END), COUNT(*) FROM t GROUP BY g "
                   "ORDER BY min(case(greater_than(a, 5000), a, 9999999)), SUM(case when status='ok' then 1 else 0 end) DESC, g, COUNT(*) LIMIT 5")
    assert qc.resolved_order_by() == [(capi.ORDER_BY_AGGREGATION, 1, True), (capi.ORDER_BY_AGGREGATION, 0, False), (capi.ORDER_BY_GROUP_KEY, 0, True),
                                      (capi.ORDER_BY_AGGREGATION, 2, True)]
    qc = parse_sql("SELECT g, SUM(CASE WHEN a > 5 THEN a ELSE 0 END) FROM t GROUP BY g ORDER BY SUM(CASE WHEN a > 6 THEN a ELSE 0 END)")
    assert qc.resolved_order_by() is None                # another text names no aggregation of the select list
    assert parse_sql("SELECT g, SUM(a * b) FROM t GROUP BY g ORDER BY SUM(a * b) DESC").resolved_order_by() == [(capi.ORDER_BY_AGGREGATION, 0, False)]


def test_shim_carries_the_text(tmp_path):
    """tests/shim_case_records.c: the record of an aggregation over a CASE is the plain aggregation's, with the text as its column string"""
    if not os.path.exists(capi.GPU_LIB_PATH):
        pytest.skip("libpinot_gpu.so not built here")
    csrc = os.path.join(ROOT, "pinot_amd", "csrc")
    exe = str(tmp_path / "shim_case_records")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "integration", "jni"), os.path.join(ROOT, "tests", "shim_case_records.c"),
                           os.path.join(ROOT, "integration", "jni", "pinot_gpu_shim.c"), "-L" + csrc, "-lpinot_gpu", "-Wl,-rpath," + csrc, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    for line in ("the texts round-trip under the plain function ids, without parameters or flags", "a truncated record fails cleanly",
                 "a percentile next to them keeps its parameter", "wire format ok"):
        assert line in out.stdout
