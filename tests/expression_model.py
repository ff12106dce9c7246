"""A numpy restatement of the reference's arithmetic transform functions inside aggregations (AdditionTransformFunction,
SubtractionTransformFunction, MultiplicationTransformFunction, DivisionTransformFunction under pinot-core/.../operator/transform/function/):
IEEE double, one separately rounded operation at a time, in the reference's argument order —
  add(args):  sum = 0.0; sum += every literal argument in argument order; then sum += every other argument in argument order
  mult(args): the same with 1.0 and *=
  sub(a, b) = a - b;  div(a, b) = a / b
over operands as getDoubleValuesSV gives them (a LONG cast (double) round-to-nearest, a FLOAT widened exactly).  The aggregations: SUM is
math.fsum of the per-doc values (exact, rounded once), MIN / MAX compare with < / >, AVG is (sum, count), MINMAXRANGE (min, max); over no doc
0.0, +inf, -inf, (0.0, 0), (+inf, -inf).  The text is what ExpressionContext#toString prints; the aliases plus / minus / times / divide
(TransformFunctionType.java:47-50) are the same functions."""
import math

import numpy as np

from tests.percentile_model import as_doubles

_FUNCTIONS = {"add": "add", "plus": "add", "sub": "sub", "minus": "sub", "mult": "mult", "times": "mult", "div": "div", "divide": "div"}


def parse(text: str):
    """('col', name) | ('lit', float) | (fn, [args]) of a canonical expression text"""
    pos = 0

    def skip():
        nonlocal pos
        while pos < len(text) and text[pos] == " ":
            pos += 1

    def arg():
        nonlocal pos
        skip()
        if text[pos] == "'":
            end = text.index("'", pos + 1)
            v = float(text[pos + 1:end])
            pos = end + 1
            return ("lit", v)
        start = pos
        while pos < len(text) and text[pos] not in "(),' ":
            pos += 1
        token = text[start:pos]
        skip()
        if pos < len(text) and text[pos] == "(":
            pos += 1
            args = [arg()]
            skip()
            while text[pos] == ",":
                pos += 1
                args.append(arg())
                skip()
            assert text[pos] == ")", text
            pos += 1
            return (_FUNCTIONS[token.lower()], args)
        if token[0].isdigit() or token[0] in "+-.":
            return ("lit", float(token))
        return ("col", token)

    tree = arg()
    skip()
    assert pos == len(text), text
    return tree


def columns_of(text: str):
    """the distinct columns an expression names, in order of first appearance"""
    out = []

    def walk(node):
        if node[0] == "col":
            if node[1] not in out:
                out.append(node[1])
        elif node[0] != "lit":
            for a in node[1]:
                walk(a)
    walk(parse(text))
    return out


def evaluate(text: str, data, schema, docs=None) -> np.ndarray:
    """the per-doc float64 values of the expression over `docs` (all docs by default)"""
    def walk(node):
        if node[0] == "lit":
            return node[1]
        if node[0] == "col":
            v = np.asarray(data[node[1]])
            return as_doubles(v if docs is None else v[np.asarray(docs, dtype=np.int64)], schema[node[1]])
        fn, args = node[0], [walk(a) for a in node[1]]
        literals = [a for a in args if isinstance(a, float)]
        others = [a for a in args if not isinstance(a, float)]
        with np.errstate(all="ignore"):
            if fn in ("add", "mult"):
                assert len(args) >= 2, text
                acc = np.float64(0.0 if fn == "add" else 1.0)
                for v in literals:
                    acc = acc + np.float64(v) if fn == "add" else acc * np.float64(v)
                if not others:
                    return float(acc)
                for v in others:
                    acc = acc + v if fn == "add" else acc * v
                return acc
            assert len(args) == 2, text
            a, b = (np.float64(x) if isinstance(x, float) else x for x in args)
            r = a - b if fn == "sub" else a / b
            return float(r) if not others else r
    v = walk(parse(text))
    assert not isinstance(v, float), f"{text}: no column"
    return np.asarray(v, dtype=np.float64)


def agg_sum(values) -> float:
    return math.fsum(float(v) for v in values)


def agg_min(values) -> float:
    m = float("inf")
    for v in values:
        if v < m:
            m = float(v)
    return m


def agg_max(values) -> float:
    m = float("-inf")
    for v in values:
        if v > m:
            m = float(v)
    return m


def aggregate(function: str, values):
    """the intermediate result of `function` over the per-doc values, as ResultsBlock.rows() shows it"""
    if function == "SUM":
        return agg_sum(values)
    if function == "MIN":
        return agg_min(values)
    if function == "MAX":
        return agg_max(values)
    if function == "AVG":
        return (agg_sum(values), len(values))
    if function == "MINMAXRANGE":
        return (agg_min(values), agg_max(values))
    raise ValueError(function)


def transform_queries_segment(n_rows: int = 10):
    """TransformQueriesTest#buildSegment: ten equal rows (INT_COL1 1000, INT_COL2 2000, LONG_COL1 500000, LONG_COL2 1000000)"""
    data = {"INT_COL1": np.full(n_rows, 1000, dtype=np.int32), "INT_COL2": np.full(n_rows, 2000, dtype=np.int32),
            "LONG_COL1": np.full(n_rows, 500000, dtype=np.int64), "LONG_COL2": np.full(n_rows, 1000000, dtype=np.int64)}
    schema = {"INT_COL1": "INT", "INT_COL2": "INT", "LONG_COL1": "LONG", "LONG_COL2": "LONG"}
    return data, schema
