"""tests/case_model.py against the reference's own CaseTransformFunctionTest, over fixed values around its thresholds instead of its random
ones (tests/golden/case_expected.json: the values, the thresholds and what the test's Java expressions give for them):
  #testCasePriorityObserved                              eight threshold triples over INT / LONG / FLOAT / DOUBLE columns
  #testCaseTransformFunctionWithIntResults               the six operators against one of the column's own values (the FLOAT column's
                                                         literal is CAST there, which is out of scope: the test below covers FLOAT)
  #testCaseTransformFunctionWithoutCastForFloatValues    equals(floatCol, <its %f text>) compares the widened float with the double
The golden expectations compare exactly, which is the function's Double.compare on the widened values (the Java test's own `float > int`
promotes the threshold to float, which differs only at thresholds no float holds).  And the model's own rules: typing and upcast, Double.compare, the 0.0 placeholder, float narrowing, the exact SUM."""
import json
import math
import os

import numpy as np
import pytest

from pinot_amd.query import canonical_expression
from tests import case_model as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "case_expected.json")))
_NP = {"INT": np.int32, "LONG": np.int64, "FLOAT": np.float32, "DOUBLE": np.float64}


def _column(name):
    c = GOLDEN["columns"][name]
    return {name: np.asarray(c["values"], dtype=_NP[c["type"]])}, {name: c["type"]}


@pytest.mark.parametrize("case", GOLDEN["priority"], ids=lambda c: "%s-%s" % (c["column"], c["thresholds"][0]))
def test_case_priority_observed(case):
    col, (t1, t2, t3) = case["column"], case["thresholds"]
    text = canonical_expression(f"CASE WHEN {col} > {t1} THEN 3 WHEN {col} > {t2} THEN 2 WHEN {col} > {t3} THEN 1 ELSE -1 END")
    assert text == f"case(greaterthan({col},'{t1}'),'3',greaterthan({col},'{t2}'),'2',greaterthan({col},'{t3}'),'1','-1')"
    data, schema = _column(col)
    assert cm.result_type(text, schema) == "INT"
    assert cm.evaluate(text, data, schema).tolist() == [float(v) for v in case["expected"]]


@pytest.mark.parametrize("case", GOLDEN["operators"], ids=lambda c: "%s-%s" % (c["function"], c["column"]))
def test_case_with_int_results(case):
    col = case["column"]
    text = f"case({case['function']}({col},{case['literal']}),'100','10')"
    if col == "stringSV":
        n = len(GOLDEN["strings"])
        data, schema = {col: list(GOLDEN["strings"])}, {col: "STRING"}
        assert len(case["expected"]) == n
    else:
        data, schema = _column(col)
    assert cm.evaluate(text, data, schema).tolist() == [float(v) for v in case["expected"]]


def test_case_without_cast_for_float_values():
    g = GOLDEN["float_without_cast"]
    data = {"floatSV": np.asarray(g["values"], dtype=np.float32), "intSV": np.arange(100, 100 + len(g["values"]), dtype=np.int32)}   # (none is the ELSE's 10)
    schema = {"floatSV": "FLOAT", "intSV": "INT"}
    assert any(c["equal"] for c in g["cases"]) and not all(c["equal"] for c in g["cases"])
    for i, c in enumerate(g["cases"]):
        text = f"case(equals(floatSV,'{c['literal']}'),intSV,'10')"
        assert cm.result_type(text, schema) == "INT"
        got = cm.evaluate(text, data, schema)
        assert (got[i] == data["intSV"][i]) == c["equal"], c      # 0.1f is not 0.100000: the ELSE answers for its own doc


def test_without_else_takes_the_placeholder():
    g = GOLDEN["without_else"]
    data, schema = _column("intSV")
    assert cm.evaluate(g["text"], data, schema).tolist() == g["expected"]
    assert canonical_expression("CASE WHEN intSV > 0 THEN intSV END") == g["text"] == canonical_expression("case when intSV > 0 then intSV else null end")


def test_typing_and_upcast():
    schema = {"i": "INT", "l": "LONG", "f": "FLOAT", "d": "DOUBLE"}
    assert [cm.literal_type(t) for t in ("1", "-2147483648", "2147483648", "-9223372036854775808", "9223372036854775808", "1.0", "1e3", "abc")] == \
        ["INT", "INT", "LONG", "LONG", "DOUBLE", "DOUBLE", "DOUBLE", "STRING"]
    for text, want in (("case(equals(i,'1'),'1','0')", "INT"), ("case(equals(i,'1'),i,'3000000000')", "LONG"), ("case(equals(i,'1'),l,f)", "FLOAT"),
                       ("case(equals(i,'1'),f,'1')", "FLOAT"), ("case(equals(i,'1'),f,'1.0')", "DOUBLE"), ("case(equals(i,'1'),i,'null')", "INT"),
                       ("case(equals(i,'1'),times(i,i),'0')", "DOUBLE"), ("case(equals(i,'1'),case(equals(i,'2'),f,'0'),l)", "FLOAT"),
                       ("case(equals(i,'1'),case(equals(i,'2'),f,'0'),d)", "DOUBLE")):
        assert cm.result_type(text, schema) == want, text


def test_double_compare():
    nan, inf = float("nan"), float("inf")
    x = np.array([0.0, -0.0, nan, inf, -inf, 1.0, nan])
    y = np.array([-0.0, 0.0, nan, nan, -inf, 2.0, 1e308])
    assert cm.double_compare(x, y).tolist() == [1, -1, 0, -1, 0, -1, 1]
    data, schema = {"d": x}, {"d": "DOUBLE"}
    assert cm.evaluate("case(equals(d,'0'),'1','0')", data, schema).tolist() == [1, 0, 0, 0, 0, 0, 0]      # -0.0 is not 0
    assert cm.evaluate("case(lessthan(d,'0'),'1','0')", data, schema).tolist() == [0, 1, 0, 0, 1, 0, 0]    # ... it is below it
    assert cm.evaluate("case(greaterthan(d,'1e308'),'1','0')", data, schema).tolist() == [0, 0, 1, 1, 0, 0, 1]   # NaN above everything


def test_first_true_wins_and_logical_operators():
    data, schema = {"a": np.arange(10, dtype=np.int32), "s": ["x", "y"] * 5}, {"a": "INT", "s": "STRING"}
    text = "case(greaterthan(a,'6'),'3',greaterthan(a,'3'),'2',greaterthan(a,'0'),'1','-1')"
    assert cm.evaluate(text, data, schema).tolist() == [-1, 1, 1, 1, 2, 2, 2, 3, 3, 3]
    text = "case(and(greaterthan(a,'2'),or(equals(s,'x'),not(lessthan(a,'8')))),a,'null')"
    assert cm.evaluate(text, data, schema).tolist() == [0, 0, 0, 0, 4, 0, 6, 0, 8, 9]
    assert cm.columns_of(text) == ["a", "s"]
    assert cm.conditions("notequals(s,'x')", data, schema).tolist() == [False, True] * 5


def test_float_narrowing_of_literals():
    data, schema = {"f": np.array([0.5, 1.5], dtype=np.float32), "i": np.array([1, 2], dtype=np.int32)}, {"f": "FLOAT", "i": "INT"}
    got = cm.evaluate("case(greaterthan(f,'1'),f,'16777217')", data, schema)      # FLOAT: (float)16777217 = 16777216
    assert got.tolist() == [16777216.0, 1.5]
    got = cm.evaluate("case(greaterthan(f,'1'),f,'16777217.0')", data, schema)    # DOUBLE: the literal stays
    assert got.tolist() == [16777217.0, 1.5]
    got = cm.evaluate("case(greaterthan(i,'1'),i,'16777217')", data, schema)      # INT: widened
    assert got.tolist() == [16777217.0, 2.0]


def test_only_the_selected_branch_counts_and_sum_is_exact():
    data = {"a": np.array([1, 2, 3, 4], dtype=np.int32), "b": np.array([0, 2, 0, 3], dtype=np.int32),
            "d": np.array([1e16, 1.0, -1e16, 1.0])}
    schema = {"a": "INT", "b": "INT", "d": "DOUBLE"}
    v = cm.evaluate("case(notequals(b,'0'),divide(a,b),'0')", data, schema)
    assert v.tolist() == [0.0, 1.0, 0.0, 4 / 3]
    v = cm.evaluate("case(greaterthan(a,'0'),d,'0')", data, schema)
    assert cm.aggregate("SUM", v) == math.fsum(v) == 2.0                       # rounded once: a running double gives 1.0
    assert cm.aggregate("AVG", v) == (2.0, 4) and cm.aggregate("MINMAXRANGE", v) == (-1e16, 1e16)
    v = cm.evaluate("times('2',case(greaterthan(a,'2'),a,'null'))", data, schema)
    assert v.tolist() == [0.0, 0.0, 6.0, 8.0]
