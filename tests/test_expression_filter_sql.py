"""Arithmetic expressions on the left-hand side of a predicate through the upper layers: parse_sql (the canonical text, the rewrites of
PredicateComparisonRewriter), CQuery (the text passes through to pg_filter_node.column) and the JNI wire format through the shim's C half
(tests/shim_expression_filter_records.c against integration/jni/pinot_gpu_shim.c)."""
import os
import subprocess

import pytest

from pinot_amd import capi
from pinot_amd.query import UNBOUNDED, CQuery, SqlError, parse_sql

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _show(f):
    if f.type == "PREDICATE":
        p = f.predicate
        if p.type == "RANGE":
            return "%s %s%s,%s%s" % (p.column, "[" if p.lower_inclusive else "(", p.lower, p.upper, "]" if p.upper_inclusive else ")")
        return "%s %s %s" % (p.column, p.type, ",".join(p.values))
    return "%s(%s)" % (f.type, "; ".join(_show(c) for c in f.children))


def _where(text):
    return _show(parse_sql("SELECT COUNT(*) FROM t WHERE " + text).filter)


@pytest.mark.parametrize("where, want", [
    # infix and function forms: the canonical text of ExpressionContext#toString
    ("price * quantity > 1000", "times(price,quantity) (1000,*)"),
    ("DIV(a, b) BETWEEN 10 AND 20", "div(a,b) [10,20]"),
    ("add(a, 2.5, b) <= -3", "add(a,'2.5',b) (*,-3]"),
    ("a + b * 2 - c / 4 = 7", "minus(plus(a,times(b,'2')),divide(c,'4')) EQ 7"),
    ("a - 5 != 3", "minus(a,'5') NOT_EQ 3"),
    ("a -5 >= 3", "minus(a,'5') [3,*)"),
    ("MULT(a, SUB(b, 1)) < 0", "mult(a,sub(b,'1')) (*,0)"),
    # a leading '(' opens an expression, or a predicate group
    ("(a + b) > 3", "plus(a,b) (3,*)"),
    ("(a + b) * 2 > 3", "times(plus(a,b),'2') (3,*)"),
    ("((a + b)) / (c - 1) <= 3", "divide(plus(a,b),minus(c,'1')) (*,3]"),
    ("(a) > 3", "a (3,*)"),
    ("(a > 3)", "a (3,*)"),
    ("(a > 3 OR b + 1 < 2) AND c = 'x'", "AND(OR(a (3,*); plus(b,'1') (*,2)); c EQ x)"),
    ("((a > 1 AND b < 2))", "AND(a (1,*); b (*,2))"),
    ("NOT (a - b > 0)", "NOT(minus(a,b) (0,*))"),
    ("(a + b) BETWEEN 1 AND 2 OR (c > 1)", "OR(plus(a,b) [1,2]; c (1,*))"),
    # PredicateComparisonRewriter: a literal on the left changes sides ...
    ("10 < a", "a (10,*)"),
    ("10 >= a", "a (*,10]"),
    ("10 = a + b", "plus(a,b) EQ 10"),
    ("'10' <> a", "a NOT_EQ 10"),
    # ... and a right-hand side that is no literal becomes minus(lhs,rhs) <op> 0
    ("a > b", "minus(a,b) (0,*)"),
    ("a <= b", "minus(a,b) (*,0]"),
    ("a = b", "minus(a,b) EQ 0"),
    ("a != b + 1", "minus(a,plus(b,'1')) NOT_EQ 0"),
    ("a * 2 >= b / c", "minus(times(a,'2'),divide(b,c)) [0,*)"),
    # every predicate form after an expression
    ("a + b BETWEEN 1 AND 2", "plus(a,b) [1,2]"),
    ("a + b NOT BETWEEN 1 AND 2", "NOT(plus(a,b) [1,2])"),
    ("a + b IN (1, 2, 3.5)", "plus(a,b) IN 1,2,3.5"),
    ("div(a,b) NOT IN (1, '2')", "div(a,b) NOT_IN 1,2"),
    ("a + b IS NOT NULL", "plus(a,b) IS_NOT_NULL "),
    # plain columns are what they were
    ("city = 'Paris' AND x IN ('a', 'b') AND y BETWEEN 1 AND 9", "AND(city EQ Paris; x IN a,b; y [1,9])"),
    ("x NOT IN (1) OR y IS NULL", "OR(x NOT_IN 1; y IS_NULL )"),
])
def test_parse_sql(where, want):
    assert _where(where) == want


def test_parse_errors():
    for where in ("1 < 2", "a + 'x' > 1", "10 BETWEEN a AND b", "a + > 1", "(a + b > 1"):
        with pytest.raises(SqlError):
            parse_sql("SELECT COUNT(*) FROM t WHERE " + where)


def test_cquery_passes_the_text_through():
    qc = parse_sql("SELECT COUNT(*) FROM t WHERE a > b AND DIV(a, b) NOT IN (1, 2)")
    root = CQuery(qc).query.filter.contents
    assert root.type == capi.FILTER_AND and root.n_children == 2
    first, second = root.children[0], root.children[1]
    assert first.column == b"minus(a,b)" and first.predicate_type == capi.PRED_RANGE
    assert (first.lower, first.upper, first.lower_inclusive, first.upper_inclusive) == (b"0", UNBOUNDED.encode(), 0, 0)
    assert second.column == b"div(a,b)" and second.predicate_type == capi.PRED_NOT_IN and [second.values[i] for i in range(2)] == [b"1", b"2"]


def test_filter_records_through_the_shim(tmp_path):
    if not os.path.exists(capi.GPU_LIB_PATH):
        pytest.skip("libpinot_gpu.so not built here")
    csrc = os.path.join(ROOT, "pinot_amd", "csrc")
    exe = str(tmp_path / "shim_expression_filter_records")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "integration", "jni"), os.path.join(ROOT, "tests", "shim_expression_filter_records.c"),
                           os.path.join(ROOT, "integration", "jni", "pinot_gpu_shim.c"), "-L" + csrc, "-lpinot_gpu", "-Wl,-rpath," + csrc, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    for line in ("an infix comparison round-trips as a RANGE over its canonical text", "an IN list over a function call round-trips under NOT",
                 "round-trips whole", "a truncated record fails cleanly", "wire format ok"):
        assert line in out.stdout
