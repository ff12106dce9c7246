"""A numpy restatement of the reference's CASE inside aggregations (CaseTransformFunction, BinaryOperatorTransformFunction and the
LogicalOperatorTransformFunctions under pinot-core/.../operator/transform/function/), over the canonical text ExpressionContext#toString
prints: case(when1,then1,...,whenN,thenN,else) with conditions equals / notequals / greaterthan / greaterthanorequal / lessthan /
lessthanorequal and and / or / not, beside the arithmetic of tests/expression_model.py.

  typing     a literal is INT when its text looks like an integer and fits int, LONG when it fits long, DOUBLE otherwise
             (RequestUtils.getLiteral); a column has its type; an arithmetic call is DOUBLE; a CASE is the numeric upcast
             INT -> LONG -> FLOAT -> DOUBLE over its THENs and its ELSE ('null', the omitted ELSE, takes no part)
  values     SUM / MIN / MAX / AVG / MINMAXRANGE read a CASE through transformToDoubleValuesSV: a DOUBLE-typed CASE reads every branch
             as a double, an INT- or LONG-typed one reads ints / longs and widens them (the same doubles), a FLOAT-typed one reads every
             branch as a FLOAT — an INT / LONG branch is narrowed with (float) — and widens the result
  conditions a comparison is Double.compare over the operands as doubles (exact for INT, FLOAT, DOUBLE and for LONGs up to 2^53): -0.0 below
             0.0, NaN equal to NaN and above +Infinity; a STRING column against a string literal is String#equals; and: every argument
             != 0, or: any, not: == 0
  selection  the first WHEN that holds selects its THEN, none the ELSE; without ELSE (null handling off) the doc takes 0.0
The aggregations are those of tests/expression_model.py: SUM is exact and rounded once."""
import numpy as np

from tests import expression_model as em
from tests.percentile_model import as_doubles, order_keys

INT, LONG, FLOAT, DOUBLE, STRING = "INT", "LONG", "FLOAT", "DOUBLE", "STRING"
_RANK = {INT: 0, LONG: 1, FLOAT: 2, DOUBLE: 3}
_ARITHMETIC = {"add": "add", "plus": "add", "sub": "sub", "minus": "sub", "mult": "mult", "times": "mult", "div": "div", "divide": "div"}
_COMPARISONS = ("equals", "notequals", "greaterthan", "greaterthanorequal", "lessthan", "lessthanorequal")
_LOGICAL = ("and", "or", "not")


def parse(text: str):
    """('col', name) | ('lit', text) | (canonical function name, [args]) of a canonical expression text"""
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
            lit = text[pos + 1:end]
            pos = end + 1
            return ("lit", lit)
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
            return (token.lower().replace("_", ""), args)
        if token[0].isdigit() or token[0] in "+-.":
            return ("lit", token)
        return ("col", token)

    tree = arg()
    skip()
    assert pos == len(text), text
    return tree


def columns_of(text: str):
    """the distinct columns an expression names, condition columns included, in order of first appearance"""
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


def literal_type(lit: str) -> str:
    """RequestUtils.getLiteral: INT, LONG or DOUBLE from the text; STRING when it is no number"""
    body = lit[1:] if lit[:1] in "+-" else lit
    if body.isdigit():
        v = int(lit)
        return INT if -2**31 <= v < 2**31 else LONG if -2**63 <= v < 2**63 else DOUBLE
    try:
        float(lit)
    except ValueError:
        return STRING
    return DOUBLE


def upcast(types):
    return max(types, key=lambda t: _RANK[t])


def _branches(node):
    """the THENs and the ELSE of a case node ('null' left out), and whether it has an ELSE"""
    args = node[1]
    assert node[0] == "case" and len(args) % 2 == 1 and len(args) >= 3, node
    otherwise = args[-1]
    has_else = otherwise != ("lit", "null")
    return args[1:-1:2] + ([otherwise] if has_else else []), has_else


def type_of(node, schema) -> str:
    if node[0] == "col":
        return schema[node[1]]
    if node[0] == "lit":
        return literal_type(node[1])
    if node[0] == "case":
        return upcast([type_of(b, schema) for b in _branches(node)[0]])
    assert node[0] in _ARITHMETIC, node
    return DOUBLE


def result_type(text: str, schema) -> str:
    return type_of(parse(text), schema)


def double_compare(x, y) -> np.ndarray:
    """Double.compare(x, y) per doc: -1, 0 or 1"""
    x, y = np.broadcast_arrays(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64))
    kx, ky = order_keys(x), order_keys(y)
    return (kx > ky).astype(np.int8) - (kx < ky).astype(np.int8)


_HOLDS = {"equals": lambda c: c == 0, "notequals": lambda c: c != 0, "greaterthan": lambda c: c > 0, "greaterthanorequal": lambda c: c >= 0,
          "lessthan": lambda c: c < 0, "lessthanorequal": lambda c: c <= 0}


class _Evaluator:
    def __init__(self, data, schema, docs):
        self.data, self.schema = data, schema
        self.docs = None if docs is None else np.asarray(docs, dtype=np.int64)
        self.n = len(next(iter(data.values()))) if self.docs is None else len(self.docs)

    def column(self, name):
        v = self.data[name]
        if self.schema[name] == STRING:
            v = np.asarray(v, dtype=object)
        else:
            v = np.asarray(v)
        return v if self.docs is None else v[self.docs]

    def full(self, v):
        return np.full(self.n, v, dtype=np.float64)

    def doubles(self, node) -> np.ndarray:
        """transformToDoubleValuesSV"""
        if node[0] == "lit":
            assert literal_type(node[1]) != STRING, node
            return self.full(float(int(node[1])) if literal_type(node[1]) in (INT, LONG) else float(node[1]))
        if node[0] == "col":
            assert self.schema[node[1]] != STRING, node
            return as_doubles(self.column(node[1]), self.schema[node[1]])
        if node[0] == "case":
            if type_of(node, self.schema) == FLOAT:
                return self.floats(node).astype(np.float64)
            return self.select(node, self.doubles)
        return self.arithmetic(node)

    def floats(self, node) -> np.ndarray:
        """transformToFloatValuesSV: what a FLOAT-typed CASE reads its branches through"""
        if node[0] == "lit":
            t = literal_type(node[1])
            assert t in (INT, LONG), node   # (a DOUBLE literal would make the CASE a DOUBLE)
            return np.full(self.n, np.float32(int(node[1])), dtype=np.float32)
        if node[0] == "col":
            t = self.schema[node[1]]
            v = self.column(node[1])
            return np.asarray(v, dtype=np.float32) if t == FLOAT else np.asarray(v, dtype=np.int64).astype(np.float32)
        assert node[0] == "case", node
        if type_of(node, self.schema) == FLOAT:
            return self.select(node, self.floats)
        return self.select(node, self.doubles).astype(np.int64).astype(np.float32)   # an INT / LONG-typed CASE, narrowed per doc

    def select(self, node, read):
        args = node[1]
        _, has_else = _branches(node)
        out = read(args[-1]) if has_else else read(("lit", "0"))   # NullValuePlaceHolder: 0 / 0.0
        out = np.array(out, copy=True)
        for k in range(len(args) - 3, -1, -2):   # from the last WHEN backwards: the first one that holds is written last
            out = np.where(self.condition(args[k]), read(args[k + 1]), out)
        return out

    def condition(self, node) -> np.ndarray:
        fn, args = node
        if fn in _COMPARISONS:
            assert len(args) == 2, node
            a, b = args
            strings = [x for x in (a, b) if x[0] == "col" and self.schema[x[1]] == STRING]
            if strings:
                assert fn in ("equals", "notequals") and len(strings) == 1, node
                col, lit = (a, b) if a[0] == "col" else (b, a)
                assert lit[0] == "lit", node
                same = self.column(col[1]) == lit[1]
                return np.asarray(same if fn == "equals" else ~same, dtype=bool)
            return _HOLDS[fn](double_compare(self.doubles(a), self.doubles(b)))
        assert fn in _LOGICAL, node
        parts = [self.condition(a) for a in args]
        if fn == "not":
            assert len(parts) == 1, node
            return ~parts[0]
        assert len(parts) >= 2, node
        out = parts[0]
        for p in parts[1:]:
            out = (out & p) if fn == "and" else (out | p)
        return out

    def arithmetic(self, node) -> np.ndarray:
        fn = _ARITHMETIC[node[0]]
        args = node[1]
        literals = [float(a[1]) for a in args if a[0] == "lit"]
        others = [self.doubles(a) for a in args if a[0] != "lit"]
        assert others, ("a call over literals only is folded before a segment sees it", node)
        with np.errstate(all="ignore"):
            if fn in ("add", "mult"):
                assert len(args) >= 2, node
                acc = np.float64(0.0 if fn == "add" else 1.0)
                for v in literals:
                    acc = acc + np.float64(v) if fn == "add" else acc * np.float64(v)
                for v in others:
                    acc = acc + v if fn == "add" else acc * v
                return np.asarray(acc, dtype=np.float64)
            assert len(args) == 2, node
            a, b = (np.float64(float(x[1])) if x[0] == "lit" else self.doubles(x) for x in args)
            return np.asarray(a - b if fn == "sub" else a / b, dtype=np.float64)


def evaluate(text: str, data, schema, docs=None) -> np.ndarray:
    """the per-doc float64 values an aggregation reads from the expression over `docs` (all docs by default)"""
    node = parse(text)
    assert node[0] not in _COMPARISONS + _LOGICAL, text
    return np.asarray(_Evaluator(data, schema, docs).doubles(node), dtype=np.float64)


def conditions(text: str, data, schema) -> np.ndarray:
    """the per-doc truth of a condition's canonical text"""
    return _Evaluator(data, schema, None).condition(parse(text))


aggregate = em.aggregate
agg_sum = em.agg_sum
