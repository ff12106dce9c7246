"""QueryContext for the hot path + a small SQL front end so tests read like the reference's (`getOperator(sql)`).

Mirrors the part of the reference a segment operator sees:
  QueryContext        pinot-core/.../query/request/context/QueryContext.java
  FilterContext       pinot-common/.../request/context/FilterContext.java
  Predicate & co      pinot-common/.../request/context/predicate/{Eq,NotEq,In,NotIn,Range}Predicate.java
SQL → QueryContext follows CalciteSqlParser.compileToPinotQuery + RequestContextUtils.getFilter for the shapes the
inner-segment tests use: nested AND/OR are flattened (CalciteSqlParser.compileAndExpression), comparisons become RANGE
predicates with "*" for an unbounded side (RequestContextUtils.java, RangePredicate.UNBOUNDED), BETWEEN is an inclusive
RANGE.  The broker-side QueryOptimizer (range merging etc.) is *not* applied, exactly as in BaseQueriesTest.getOperator
(pinot-core/src/test/.../queries/BaseQueriesTest.java:100-105).
"""
from __future__ import annotations

import ctypes as C
import functools
import re
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

from . import capi

UNBOUNDED = "*"


@dataclass
class Predicate:
    type: str                      # EQ / NOT_EQ / IN / NOT_IN / RANGE
    column: str
    values: List[str] = field(default_factory=list)
    lower: str = UNBOUNDED
    upper: str = UNBOUNDED
    lower_inclusive: bool = False
    upper_inclusive: bool = False


@dataclass
class FilterContext:
    type: str                      # AND / OR / NOT / PREDICATE / CONSTANT_TRUE / CONSTANT_FALSE
    children: List["FilterContext"] = field(default_factory=list)
    predicate: Optional[Predicate] = None

    @staticmethod
    def and_(children):
        return FilterContext("AND", list(children))

    @staticmethod
    def or_(children):
        return FilterContext("OR", list(children))

    @staticmethod
    def not_(child):
        return FilterContext("NOT", [child])

    @staticmethod
    def pred(p: Predicate):
        return FilterContext("PREDICATE", [], p)


def eq(col, v):
    return FilterContext.pred(Predicate("EQ", col, [str(v)]))


def neq(col, v):
    return FilterContext.pred(Predicate("NOT_EQ", col, [str(v)]))


def in_(col, vs):
    return FilterContext.pred(Predicate("IN", col, [str(v) for v in vs]))


def not_in(col, vs):
    return FilterContext.pred(Predicate("NOT_IN", col, [str(v) for v in vs]))


def range_(col, lower=UNBOUNDED, upper=UNBOUNDED, lower_inclusive=True, upper_inclusive=True):
    return FilterContext.pred(Predicate("RANGE", col, [], str(lower), str(upper),
                                        bool(lower_inclusive) and str(lower) != UNBOUNDED,
                                        bool(upper_inclusive) and str(upper) != UNBOUNDED))


@dataclass
class AggregationSpec:
    function: str                  # COUNT / SUM / MIN / MAX / AVG / DISTINCTCOUNT / DISTINCTCOUNTHLL / MINMAXRANGE
    column: Optional[str] = None   # None for COUNT(*); an arithmetic expression as its canonical text, e.g. "plus(a,times(b,'2'))"
    log2m: int = 0
    percentile: Optional[float] = None   # PERCENTILE: p in [0, 100]


@dataclass
class QueryContext:
    table: str = "testTable"
    filter: Optional[FilterContext] = None
    group_by: List[str] = field(default_factory=list)   # columns, or arithmetic expressions as their canonical text, e.g. "sub(column1,'100000')"
    aggregations: List[AggregationSpec] = field(default_factory=list)
    select_columns: List[str] = field(default_factory=list)   # identifiers and arithmetic expressions (canonical text) in the select list
    order_by: List[Tuple[str, bool]] = field(default_factory=list)  # (expression text, ascending)
    order_by_nulls_last: List[Optional[bool]] = field(default_factory=list)   # parallel: NULLS LAST / NULLS FIRST, None = the default (OrderByExpressionContext#isNullsLast: as ascending)
    limit: int = 10
    num_groups_limit: int = 0
    max_initial_result_holder_capacity: int = 0
    flags: int = 0
    has_group_by: bool = False
    min_segment_group_trim_size: int = -1   # InstancePlanMakerImplV2.DEFAULT_MIN_SEGMENT_GROUP_TRIM_SIZE: the segment's groups are not trimmed
    distinct: List[str] = field(default_factory=list)   # SELECT DISTINCT a, b + c: the DISTINCT columns and expressions (empty: not a DISTINCT query)
    selection: List[str] = field(default_factory=list)  # a selection query (no aggregation, GROUP BY or DISTINCT): its select list, "*" kept

    def extract_expressions(self, column_names) -> List[str]:
        """The output columns of a selection on a segment with these columns: SelectionOperatorUtils#extractExpressions (:83-125) — the
        ORDER BY expressions first (none under LIMIT 0), then the select list without them; SELECT * is every column not starting with '$',
        sorted by name."""
        out = []
        if self.limit > 0:
            for text, _ in self.order_by:
                if text not in out:
                    out.append(text)
        if self.selection == ["*"]:
            rest = sorted(c for c in column_names if not c.startswith("$"))
        else:
            rest = self.selection
        for c in rest:
            if c not in out:
                out.append(c)
        return out

    def resolved_order_by(self) -> "Optional[List[Tuple[int, int, bool]]]":
        """(kind, index, ascending) per ORDER BY expression as TableResizer resolves them (TableResizer.java:129-161): a group-by expression
        or an aggregation of the select list; None when some expression is neither (post-aggregations, literals: not carried by the ABI)."""
        out = []
        def norm(t):
            t = re.sub(r"\s+", "", t).upper()
            head, paren, rest = t.partition("(")   # VAR_POP(x) names the aggregation VARPOP(x): AggregationFunctionType strips underscores
            if paren and with_time_function_name(head):   # ... and LAST_WITH_TIME(x, t, 'int') names LASTWITHTIME(X,T,INT): the type literal with or without its quotes
                return with_time_function_name(head) + paren + rest.replace("'", "")
            if paren and covariance_function_name(head):   # ... and covar_pop(x, y) names COVARPOP(X,Y)
                return covariance_function_name(head) + paren + rest
            return variance_function_name(head) + paren + rest if paren and variance_function_name(head) else t
        aggs = [norm(f"{a.function}({a.column or '*'}{',' + str(a.log2m) if a.log2m else ''})") for a in self.aggregations]
        pctl = [(a.column, a.percentile) if a.function == "PERCENTILE" else None for a in self.aggregations]
        hists = [a.column if a.function in capi.HISTOGRAM_FUNCTIONS else None for a in self.aggregations]
        modes = [a.column if a.function in capi.MODE_FUNCTIONS else None for a in self.aggregations]
        expr_aggs = {}   # (function, canonical text) of the aggregations over expressions -> the first one's index
        for i, a in enumerate(self.aggregations):
            if "(" in (a.column or ""):
                expr_aggs.setdefault((a.function, a.column), i)
        # group-by expressions by canonical text: 'SUB(   column1, 100000\t)' names the key "sub(column1,'100000')"
        keys = [canonical_expression(g) if "(" in g else g for g in self.group_by]
        for text, asc in self.order_by:
            if text in self.group_by:
                out.append((capi.ORDER_BY_GROUP_KEY, self.group_by.index(text), asc))
            elif canonical_expression(text) is not None and canonical_expression(text) in keys:
                out.append((capi.ORDER_BY_GROUP_KEY, keys.index(canonical_expression(text)), asc))
            elif norm(text) in aggs:
                out.append((capi.ORDER_BY_AGGREGATION, aggs.index(norm(text)), asc))
            elif _percentile_of_text(text) is not None and _percentile_of_text(text) in pctl:   # any of PERCENTILE's spellings names the same aggregation
                out.append((capi.ORDER_BY_AGGREGATION, pctl.index(_percentile_of_text(text)), asc))
            elif _histogram_of_text(text) is not None and _histogram_of_text(text) in hists:   # a HISTOGRAM by its canonical argument list
                out.append((capi.ORDER_BY_AGGREGATION, hists.index(_histogram_of_text(text)), asc))
            elif _mode_of_text(text) is not None and _mode_of_text(text) in modes:   # a MODE by its canonical argument list: MODE(x) names MODE(x) alone, not MODE(x, 'MIN')
                out.append((capi.ORDER_BY_AGGREGATION, modes.index(_mode_of_text(text)), asc))
            elif expr_aggs and _expression_aggregation_of_text(text) in expr_aggs:
                # an aggregation over an expression, whatever its spelling (infix or function form): by its canonical text
                out.append((capi.ORDER_BY_AGGREGATION, expr_aggs[_expression_aggregation_of_text(text)], asc))
            else:
                return None
        return out


def variance_function_name(fn: str):
    """VARPOP / VARSAMP / STDDEVPOP / STDDEVSAMP for any spelling of them (VAR_POP, stddev_samp, STD_DEV_POP: AggregationFunctionType
    strips underscores and ignores case), else None."""
    name = fn.replace("_", "").upper()
    return name if name in capi.VARIANCE_FUNCTIONS else None


def covariance_function_name(fn: str):
    """COVARPOP / COVARSAMP for any spelling of them (COVAR_POP, covarSamp), else None."""
    name = fn.replace("_", "").upper()
    return name if name in capi.COVARIANCE_FUNCTIONS else None


def _is_number(text: str) -> bool:
    try:
        float(text)
        return True
    except ValueError:
        return False


def with_time_function_name(fn: str):
    """FIRSTWITHTIME / LASTWITHTIME for any spelling of them (FIRST_WITH_TIME, lastWithTime), else None."""
    name = fn.replace("_", "").upper()
    return name if name in capi.WITH_TIME_FUNCTIONS else None


def with_time_arguments(column: str):
    """(x, t, TYPE) of a FIRSTWITHTIME / LASTWITHTIME argument list "x,t,'type'" (the type upper-cased, as DataType.valueOf(toUpperCase()))."""
    x, t, ty = (p.strip() for p in column.split(","))
    return x, t, ty.strip("'").upper()


_PERCENTILE_LEGACY = re.compile(r"^PERCENTILE(\d+)$")
_PERCENTILE_TEXT = re.compile(r"^PERCENTILE(\d*)\(([A-Za-z_][A-Za-z_0-9.$]*)(?:,'?([^')]+)'?)?\)$", re.I)


def percentile_value(text) -> float:
    """The p of PERCENTILE(col, p) / PERCENTILEp(col) (AggregationFunctionFactory: a numeric or quoted literal, 0 <= p <= 100)."""
    try:
        p = float(text)
    except (TypeError, ValueError):
        raise SqlError(f"bad percentile {text!r}")
    if not (0.0 <= p <= 100.0):
        raise SqlError(f"percentile {text} out of [0, 100]")
    return p


def _percentile_of_text(text: str):
    """(column, p) of an ORDER BY expression text that spells a PERCENTILE, else None."""
    m = _PERCENTILE_TEXT.match(re.sub(r"\s+", "", text))
    if not m or bool(m.group(1)) == bool(m.group(3)):
        return None
    try:
        return (m.group(2), percentile_value(m.group(1) or m.group(3)))
    except SqlError:
        return None


@functools.lru_cache(maxsize=256)
def _histogram_of_text(text: str):
    """The canonical argument list of an ORDER BY expression text that spells a HISTOGRAM, else None."""
    try:
        p = _Parser(text)
        if not (p.kw("HISTOGRAM") and p.peek(1) == ("op", "(")):
            return None
        p.i += 2
        args = p.histogram_arguments()
    except (SqlError, IndexError):
        return None
    return args if p.peek()[0] == "eof" else None


@functools.lru_cache(maxsize=256)
def _mode_of_text(text: str):
    """The canonical argument list of an ORDER BY expression text that spells a MODE, else None."""
    try:
        p = _Parser(text)
        if not (p.kw("MODE") and p.peek(1) == ("op", "(")):
            return None
        p.i += 2
        args = p.mode_arguments(bare=True)   # (an ORDER BY text spells the reducer literal without its quotes)
    except (SqlError, IndexError):
        return None
    return args if p.peek()[0] == "eof" else None


@functools.lru_cache(maxsize=256)
def _expression_aggregation_of_text(text: str):
    """(function, canonical expression text) of an ORDER BY expression that spells an aggregation over an arithmetic expression, else None
    (parsed once per text)."""
    try:
        p = _Parser(text)
        q = QueryContext()
        p.select_item(q)
    except SqlError:
        return None
    if p.peek()[0] != "eof" or len(q.aggregations) != 1 or "(" not in (q.aggregations[0].column or ""):
        return None
    return (q.aggregations[0].function, q.aggregations[0].column)


@functools.lru_cache(maxsize=256)
def canonical_expression(text: str):
    """The canonical text of an arithmetic expression in any spelling (infix or function form, any case and whitespace, literals quoted or
    bare); a lone column gives its name; None when the text is no such expression."""
    try:
        p = _Parser(text)
        e = p.expression()
    except (SqlError, IndexError):
        return None
    if p.peek()[0] != "eof" or e.startswith("'"):
        return None
    return e


# ----------------------------------------------------------------------------------------------------------------------
# SQL subset parser
# ----------------------------------------------------------------------------------------------------------------------
_TOKEN = re.compile(r"\s*(?:(?P<num>-?\d+(?:\.\d+)?(?:[eE][-+]?\d+)?)|(?P<str>'(?:[^']|'')*')|(?P<id>[A-Za-z_][A-Za-z_0-9.$]*)"
                    r"|(?P<qid>\"[^\"]*\")|(?P<op><=|>=|<>|!=|=|<|>|\(|\)|\[|\]|,|\*|\+|-|/))")


class SqlError(ValueError):
    pass


class _WhenError(SqlError):
    """a construct the condition of a CASE does not take (IN, BETWEEN, LIKE, IS NULL ...): raised through the parser's own backtracking"""


def _tokenize(sql: str) -> List[Tuple[str, str]]:
    pos = 0
    out = []
    sql = sql.strip().rstrip(";")
    while pos < len(sql):
        m = _TOKEN.match(sql, pos)
        if not m or m.end() == pos:
            raise SqlError(f"cannot tokenize at: {sql[pos:pos + 20]!r}")
        pos = m.end()
        if m.group("num") is not None:
            out.append(("num", m.group("num")))
        elif m.group("str") is not None:
            out.append(("str", m.group("str")[1:-1].replace("''", "'")))
        elif m.group("id") is not None:
            out.append(("id", m.group("id")))
        elif m.group("qid") is not None:   # a double-quoted identifier: "Infinity" / "-Infinity" among a HISTOGRAM's edges
            out.append(("id", m.group("qid")[1:-1]))
        else:
            out.append(("op", m.group("op")))
    return out


class _Parser:
    def __init__(self, sql: str):
        self.toks = _tokenize(sql)
        self.i = 0

    def peek(self, k=0):
        return self.toks[self.i + k] if self.i + k < len(self.toks) else ("eof", "")

    def kw(self, word: str, k=0) -> bool:
        t = self.peek(k)
        return t[0] == "id" and t[1].upper() == word

    def take(self):
        t = self.peek()
        self.i += 1
        return t

    def expect_kw(self, word: str):
        if not self.kw(word):
            raise SqlError(f"expected {word}, got {self.peek()}")
        self.i += 1

    def expect_op(self, op: str):
        t = self.take()
        if t != ("op", op):
            raise SqlError(f"expected {op!r}, got {t}")

    def literal(self) -> str:
        t = self.take()
        if t[0] not in ("num", "str"):
            raise SqlError(f"expected literal, got {t}")
        return t[1]

    # --- filter -------------------------------------------------------------------------------------------------
    def or_expr(self) -> FilterContext:
        parts = [self.and_expr()]
        while self.kw("OR"):
            self.i += 1
            parts.append(self.and_expr())
        if len(parts) == 1:
            return parts[0]
        flat = []
        for p in parts:
            flat.extend(p.children if p.type == "OR" else [p])
        return FilterContext.or_(flat)

    def and_expr(self) -> FilterContext:
        parts = [self.not_expr()]
        while self.kw("AND"):
            self.i += 1
            parts.append(self.not_expr())
        if len(parts) == 1:
            return parts[0]
        flat = []
        for p in parts:
            flat.extend(p.children if p.type == "AND" else [p])
        return FilterContext.and_(flat)

    def not_expr(self) -> FilterContext:
        if self.kw("NOT"):
            self.i += 1
            return FilterContext.not_(self.not_expr())
        return self.primary()

    _OPPOSITE = {"=": "=", "!=": "!=", "<>": "<>", "<": ">", "<=": ">=", ">": "<", ">=": "<="}

    def primary(self) -> FilterContext:
        if self.peek() == ("op", "("):
            # a leading '(' opens either a predicate group or an arithmetic expression: try the group, fall back to the expression
            mark, toks = self.i, list(self.toks)
            try:
                self.i += 1
                e = self.or_expr()
                self.expect_op(")")
                t = self.peek()
                if (t[0] == "op" and t[1] != ")") or (t[0] == "num" and t[1].startswith("-")) or any(self.kw(w) for w in ("BETWEEN", "IN", "IS")) \
                        or (self.kw("NOT") and (self.kw("IN", 1) or self.kw("BETWEEN", 1))):
                    raise SqlError("a parenthesised expression, not a predicate group")
                return e
            except SqlError:
                self.i, self.toks = mark, toks
        # the left-hand side: a column, or an arithmetic expression in its canonical text (the function forms and infix + - * /)
        col = self.expression()
        if col.startswith("'"):
            # PredicateComparisonRewriter.java:108-115: '10 < a' becomes 'a > 10'
            op = self.take()
            if op[0] != "op" or op[1] not in self._OPPOSITE:
                raise SqlError(f"expected comparison after the literal {col}, got {op}")
            lit, col = col[1:-1], self.expression()
            if col.startswith("'"):
                raise SqlError("a comparison of two literals")
            return self._comparison(col, self._OPPOSITE[op[1]], lit)
        if self.kw("BETWEEN"):
            self.i += 1
            lo = self.literal()
            self.expect_kw("AND")
            hi = self.literal()
            return FilterContext.pred(Predicate("RANGE", col, [], lo, hi, True, True))
        if self.kw("IS"):   # IS [NOT] NULL → Predicate.Type.IS_NULL / IS_NOT_NULL (IsNullPredicate, IsNotNullPredicate)
            self.i += 1
            not_null = self.kw("NOT")
            if not_null:
                self.i += 1
            self.expect_kw("NULL")
            return FilterContext.pred(Predicate("IS_NOT_NULL" if not_null else "IS_NULL", col, []))
        negate = False
        if self.kw("NOT"):
            self.i += 1
            negate = True
            if self.kw("BETWEEN"):   # Calcite: NOT BETWEEN → NOT(RANGE)
                self.i += 1
                lo = self.literal()
                self.expect_kw("AND")
                hi = self.literal()
                return FilterContext.not_(FilterContext.pred(Predicate("RANGE", col, [], lo, hi, True, True)))
        if self.kw("IN"):
            self.i += 1
            self.expect_op("(")
            vals = [self.literal()]
            while self.peek() == ("op", ","):
                self.i += 1
                vals.append(self.literal())
            self.expect_op(")")
            return FilterContext.pred(Predicate("NOT_IN" if negate else "IN", col, vals))
        if negate:
            raise SqlError("NOT must be followed by IN here")
        op = self.take()
        if op[0] != "op":
            raise SqlError(f"expected comparison, got {op}")
        if self.peek()[0] in ("num", "str"):
            return self._comparison(col, op[1], self.literal())
        # PredicateComparisonRewriter.java:117-124: a right-hand side that is no literal — 'a > b' becomes 'minus(a,b) > 0'
        rhs = self.expression()
        return self._comparison(f"minus({col},{rhs})", op[1], "0")

    @staticmethod
    def _comparison(col: str, o: str, v: str) -> FilterContext:
        if o == "=":
            return FilterContext.pred(Predicate("EQ", col, [v]))
        if o in ("!=", "<>"):
            return FilterContext.pred(Predicate("NOT_EQ", col, [v]))
        if o == ">":
            return FilterContext.pred(Predicate("RANGE", col, [], v, UNBOUNDED, False, False))
        if o == ">=":
            return FilterContext.pred(Predicate("RANGE", col, [], v, UNBOUNDED, True, False))
        if o == "<":
            return FilterContext.pred(Predicate("RANGE", col, [], UNBOUNDED, v, False, False))
        if o == "<=":
            return FilterContext.pred(Predicate("RANGE", col, [], UNBOUNDED, v, False, True))
        raise SqlError(f"unsupported operator {o}")

    # --- arithmetic expressions inside aggregations -----------------------------------------------------------------
    # The canonical text is what ExpressionContext#toString prints: fn(arg,arg,...) with the function name in lower case, literals quoted.
    # Infix + - * / become plus / minus / times / divide, as the reference's compiler names them (CalciteSqlParser: SqlKind -> function name);
    # the function forms ADD / SUB / MULT / DIV keep their names.  A lone column stays a plain column name.
    _INFIX = {"+": "plus", "-": "minus", "*": "times", "/": "divide"}

    def expression(self) -> str:
        """the canonical text of an additive expression (a lone column: its name)"""
        left = self.term()
        while True:
            t = self.peek()
            if t in (("op", "+"), ("op", "-")):
                self.i += 1
                name = self._INFIX[t[1]]
            elif t[0] == "num" and t[1].startswith("-"):   # after an operand, a number with a leading '-' is a subtraction
                self.toks[self.i] = ("num", t[1][1:])
                name = "minus"
            else:
                return left
            right = self.term()
            left = f"{name}({left},{right})"

    def term(self) -> str:
        left = self.factor()
        while self.peek() in (("op", "*"), ("op", "/")):
            name = self._INFIX[self.take()[1]]
            right = self.factor()
            left = f"{name}({left},{right})"
        return left

    def factor(self) -> str:
        t = self.take()
        if t == ("op", "("):
            e = self.expression()
            self.expect_op(")")
            return e
        if t[0] == "num":
            return f"'{t[1]}'"
        if t[0] == "str":
            try:
                float(t[1])
            except ValueError:
                raise SqlError(f"the literal {t[1]!r} in an arithmetic expression is not a number")
            return f"'{t[1]}'"
        if t[0] != "id":
            raise SqlError(f"bad aggregation argument {t}")
        if t[1].upper() == "CASE" and self.kw("WHEN"):
            return self.case_expression()
        if self.peek() == ("op", "("):   # a function call: its name in lower case, without underscores (FunctionContext's canonical name)
            self.i += 1
            name = t[1].lower().replace("_", "")
            argument = self.time_argument if name in self._TIME or name in ("equals", "notequals") else self.else_argument if name == "case" else self.expression
            args = [argument()]
            while self.peek() == ("op", ","):
                self.i += 1
                args.append(argument())
            self.expect_op(")")
            return f"{name}({','.join(args)})"
        return t[1]

    # CASE WHEN c THEN x [WHEN ...] [ELSE y] END: case(c1,x1,...,cN,xN,else) as CalciteSqlParser compiles it (711-734):
    # WHEN and THEN in pairs, the ELSE last, an omitted ELSE or ELSE NULL as the literal 'null'.  A condition is not a
    # FilterContext here but a function call like any other: a > b stays greater_than(a,b) (PredicateComparisonRewriter touches WHERE and
    # HAVING only), AND / OR are n-ary and flattened, NOT and parentheses nest.
    _COMPARISON = {"=": "equals", "!=": "notequals", "<>": "notequals", ">": "greaterthan", ">=": "greaterthanorequal",
                   "<": "lessthan", "<=": "lessthanorequal"}   # FunctionContext's canonical names: lower case, no underscores

    def else_argument(self) -> str:
        """an argument of the function form case(...): the last one may be the literal 'null', the omitted ELSE"""
        if self.peek() == ("str", "null") and self.peek(1) == ("op", ")"):
            self.i += 1
            return "'null'"
        return self.expression()

    def case_expression(self) -> str:
        args = []
        while self.kw("WHEN"):
            self.i += 1
            args.append(self._condition_text(self.condition()))
            self.expect_kw("THEN")
            args.append(self.expression())
        if self.kw("ELSE"):
            self.i += 1
            if self.kw("NULL"):
                self.i += 1
                args.append("'null'")
            else:
                args.append(self.expression())
        else:
            args.append("'null'")
        self.expect_kw("END")
        return f"case({','.join(args)})"

    @staticmethod
    def _condition_text(c) -> str:
        op, items = c
        return items[0] if op is None else f"{op}({','.join(items)})"

    def _condition_list(self, word: str, op: str, operand):
        parts = [operand()]
        while self.kw(word):
            self.i += 1
            parts.append(operand())
        if len(parts) == 1:
            return parts[0]
        flat = []
        for p in parts:   # a AND (b AND c) is and(a,b,c)
            flat.extend(p[1] if p[0] == op else [self._condition_text(p)])
        return (op, flat)

    def condition(self):
        """(None, [text]) | ('and' | 'or', [texts]) of the condition that starts here"""
        return self._condition_list("OR", "or", lambda: self._condition_list("AND", "and", self.condition_not))

    def condition_not(self):
        if self.kw("NOT"):
            self.i += 1
            return (None, [f"not({self._condition_text(self.condition_not())})"])
        if self.peek() == ("op", "("):   # a group of conditions, or a parenthesised operand: try the group, fall back to the operand
            mark, toks = self.i, list(self.toks)
            try:
                self.i += 1
                c = self.condition()
                self.expect_op(")")
                t = self.peek()
                if (t[0] == "op" and t[1] not in (")", ",")) or (t[0] == "num" and t[1].startswith("-")):
                    raise SqlError("a parenthesised operand, not a group of conditions")
                return c
            except _WhenError:
                raise
            except SqlError:
                self.i, self.toks = mark, toks
        return self.comparison()

    def condition_operand(self):
        """(canonical text, is a non-numeric string literal)"""
        t = self.peek()
        if t[0] == "str" and not _is_number(t[1]):
            self.i += 1
            if "'" in t[1]:
                raise SqlError(f"the literal {t[1]!r} holds a quote: the canonical text cannot carry it")
            return f"'{t[1]}'", True
        return self.expression(), False

    def comparison(self):
        left, left_text = self.condition_operand()
        for word in ("IN", "BETWEEN", "LIKE", "IS"):
            if self.kw(word) or (self.kw("NOT") and self.kw(word, 1)):
                raise _WhenError(f"{'IS [NOT] NULL' if word == 'IS' else word} inside a WHEN: comparisons, AND, OR and NOT are its conditions")
        op = self.take()
        if op[0] != "op" or op[1] not in self._COMPARISON:
            raise SqlError(f"expected a comparison inside a WHEN, got {op}")
        right, right_text = self.condition_operand()
        if left.startswith("'") and right.startswith("'"):
            raise SqlError("a comparison of two literals")
        if (left_text or right_text) and op[1] not in ("=", "!=", "<>"):
            raise SqlError(f"the string literal {left if left_text else right} under {op[1]}: = and <> compare strings inside a WHEN")
        return (None, [f"{self._COMPARISON[op[1]]}({left},{right})"])

    # The time-bucket transforms: GROUP BY / DISTINCT keys such as dateTrunc('day', ts).  Their arguments other than the value are
    # literals of any text (units, formats, time zones), printed single-quoted with their case kept; nowhere else is a non-numeric string literal
    # an operand.
    _TIME = frozenset(["timeconvert", "datetimeconvert", "datetrunc"]
                      + ["toepoch" + u + v for u in ("seconds", "minutes", "hours", "days") for v in ("", "rounded", "bucket")])

    def time_argument(self) -> str:
        t = self.peek()
        if t[0] == "str" and self.peek(1) in (("op", ","), ("op", ")")):
            self.i += 1
            return f"'{t[1]}'"
        return self.expression()

    _ARITHMETIC = frozenset(("add", "sub", "mult", "div", "plus", "minus", "times", "divide", "case"))

    def starts_expression(self) -> bool:
        """Does an expression start here, where a select item, a GROUP BY key or an ORDER BY expression is expected: one of the eight
        arithmetic function forms, a time-bucket transform, a parenthesis, or an operand followed by an infix operator?"""
        t, u = self.peek(), self.peek(1)
        if t == ("op", "("):
            return True
        if self.kw("CASE") and self.kw("WHEN", 1):
            return True
        if t[0] == "id" and u == ("op", "("):
            return t[1].lower().replace("_", "") in self._ARITHMETIC or t[1].lower().replace("_", "") in self._TIME
        if t[0] in ("id", "num"):
            return (u[0] == "op" and u[1] in self._INFIX) or (u[0] == "num" and u[1].startswith("-"))
        return False

    def key_expression(self) -> str:
        """a GROUP BY / DISTINCT key: a column, or an arithmetic expression as its canonical text"""
        e = self.expression()
        if e.startswith("'"):
            raise SqlError(f"a literal ({e}) where a column or an expression is expected")
        return e

    def aggregation_argument(self) -> str:
        e = self.expression()
        if e.startswith("'"):
            raise SqlError(f"bad aggregation argument {e}: a literal")
        return e

    def histogram_arguments(self) -> str:
        """The canonical argument list of a HISTOGRAM, the opening parenthesis taken: "x,'lower','upper','numBins'" or
        "x,arrayvalueconstructor('e0','e1',...)" with Infinity / -Infinity bare (identifiers, as the reference's parser hands them over).  The
        malformed forms raise with HistogramAggregationFunction's own texts."""
        args = [self.aggregation_argument()]
        while self.peek() == ("op", ","):
            self.i += 1
            if self.kw("ARRAY") and self.peek(1) == ("op", "["):
                self.i += 2
                edges = []
                while self.peek() != ("op", "]"):
                    t = self.take()
                    if t == ("op", "-") and self.peek() == ("id", "Infinity"):   # (an ORDER BY text spells the quoted identifier bare)
                        t = ("id", "-" + self.take()[1])
                    if t[0] == "id" and t[1] in ("Infinity", "-Infinity"):
                        edges.append((t[1], float(t[1].replace("Infinity", "inf"))))
                    elif t[0] in ("num", "str"):
                        try:
                            edges.append((f"'{t[1]}'", float(t[1])))
                        except ValueError:
                            raise SqlError(f'For input string: "{t[1]}"')
                    else:
                        raise SqlError(f"HISTOGRAM: bad bin edge {t}")
                    if self.peek() == ("op", ","):
                        self.i += 1
                self.i += 1
                args.append(edges)
            else:
                t = self.take()
                if t[0] not in ("num", "str"):
                    raise SqlError(f"HISTOGRAM: expected a literal, got {t}")
                args.append(t[1])
        self.expect_op(")")
        if len(args) not in (2, 4):
            raise SqlError(f"Histogram expects 2 or 4 arguments, got: {len(args)}; usage example: `Histogram(columnName, ARRAY[0,1,10,100])` to "
                           "specify bins [0,1), [1,10), [10,1000] or `Histogram(columnName, 0, 1000, 10)` to specify 10 equal-length bins "
                           "[0,100), [100,200), ..., [900,1000]")
        if len(args) == 2:
            edges = args[1]
            if not isinstance(edges, list):
                raise SqlError("Please use the format of `Histogram(columnName, ARRAY[1,10,100])` to specify the bin edges")
            if len(edges) < 2:
                raise SqlError("The number of bin edges must be greater than 1")
            if any(not (b[1] > a[1]) for a, b in zip(edges, edges[1:])):
                raise SqlError("The bin edges must be strictly increasing")
            return f"{args[0]},arrayvalueconstructor({','.join(e[0] for e in edges)})"
        if any(isinstance(a, list) for a in args[1:]):
            raise SqlError("HISTOGRAM: the equal-width form takes three literals, not an array")
        try:
            lower, upper = float(args[1]), float(args[2])
        except ValueError:
            bad = args[1] if not _is_number(args[1]) else args[2]
            raise SqlError(f'For input string: "{bad}"')
        if not _is_number(args[3]) or float(args[3]) != int(float(args[3])):
            raise SqlError(f'For input string: "{args[3]}"')
        bins = int(float(args[3]))
        if not upper > lower:
            raise SqlError(f"The right most edge must be greater than left most edge, given {lower!r} and {upper!r}")
        if bins <= 0:
            raise SqlError(f"The number of bins must be greater than zero, given {bins}")
        return f"{args[0]},'{args[1]}','{args[2]}','{args[3]}'"

    def mode_arguments(self, bare: bool = False) -> str:
        """The canonical argument list of a MODE, the opening parenthesis taken: "x" or "x,'MAX'".  The malformed forms raise with
        ModeAggregationFunction's own texts: more than two arguments, a reducer MultiModeReducerType.valueOf does not know (it is exact:
        upper case)."""
        args = [self.aggregation_argument()]
        while self.peek() == ("op", ","):
            self.i += 1
            t = self.take()
            if t[0] not in ("str", "num", "id"):
                raise SqlError(f"MODE: expected an argument, got {t}")
            args.append(t)
        self.expect_op(")")
        if len(args) > 2:
            raise SqlError(f"Mode expects at most 2 arguments, got: {len(args)}")
        if len(args) == 1:
            return args[0]
        if args[1][0] != "str" and not (bare and args[1][0] == "id"):
            raise SqlError(f"MODE: the second argument must be a quoted MultiModeReducerType ('MIN', 'MAX' or 'AVG'), got {args[1][1]}")
        if args[1][1] not in capi.MODE_REDUCERS:
            raise SqlError("No enum constant org.apache.pinot.core.query.aggregation.function.ModeAggregationFunction.MultiModeReducerType." + args[1][1])
        return f"{args[0]},'{args[1][1]}'"

    # --- select -------------------------------------------------------------------------------------------------
    def select_item(self, q: QueryContext):
        if self.peek() != ("op", "*") and self.starts_expression():   # an arithmetic expression: a DISTINCT / GROUP BY key of the select list
            q.select_columns.append(self.key_expression())
            if self.kw("AS"):
                self.i += 2
            return
        t = self.take()
        if t == ("op", "*"):   # SELECT *
            q.select_columns.append("*")
            return
        if t[0] != "id":
            raise SqlError(f"bad select item {t}")
        if self.peek() == ("op", "("):
            fn = variance_function_name(t[1]) or with_time_function_name(t[1]) or covariance_function_name(t[1]) or t[1].upper()
            self.i += 1
            if fn in capi.COVARIANCE_FUNCTIONS:   # COVAR_POP(x, y): the argument list "x,y", as getResultColumnName joins it
                args = [self.aggregation_argument()]
                self.expect_op(",")
                args.append(self.aggregation_argument())
                self.expect_op(")")
                q.aggregations.append(AggregationSpec(fn, f"{args[0]},{args[1]}"))
                if self.kw("AS"):
                    self.i += 2
                return
            if fn in capi.HISTOGRAM_FUNCTIONS:   # HISTOGRAM(x, lower, upper, numBins) / HISTOGRAM(x, ARRAY[e0, e1, ...])
                q.aggregations.append(AggregationSpec(fn, self.histogram_arguments()))
                if self.kw("AS"):
                    self.i += 2
                return
            if fn in capi.MODE_FUNCTIONS:   # MODE(x) / MODE(x, 'MIN' | 'MAX' | 'AVG')
                q.aggregations.append(AggregationSpec(fn, self.mode_arguments()))
                if self.kw("AS"):
                    self.i += 2
                return
            if fn in capi.WITH_TIME_FUNCTIONS:   # FIRSTWITHTIME(x, t, 'TYPE'): the argument list travels as getResultColumnName prints it
                args = [self.aggregation_argument()]
                self.expect_op(",")
                args.append(self.aggregation_argument())
                self.expect_op(",")
                t3 = self.take()
                if t3[0] != "str":
                    raise SqlError(f"{fn}: the third argument must be a quoted data type literal, got {t3}")
                self.expect_op(")")
                q.aggregations.append(AggregationSpec(fn, f"{args[0]},{args[1]},'{t3[1]}'"))
                if self.kw("AS"):
                    self.i += 2
                return
            if self.peek() == ("op", "*") and self.peek(1) == ("op", ")"):
                self.i += 1
                col = None
            else:
                col = self.aggregation_argument()   # a column, or the canonical text of an arithmetic expression
            log2m = 0
            legacy = _PERCENTILE_LEGACY.match(fn)
            if fn == "PERCENTILE" or legacy:   # PERCENTILE(col, 95) / (col, 99.9) / (col, '50') and the legacy PERCENTILE95(col)
                if col is None:
                    raise SqlError("PERCENTILE needs a column")
                if legacy:
                    p = percentile_value(legacy.group(1))
                else:
                    if self.peek() != ("op", ","):
                        raise SqlError("PERCENTILE(col, p) needs its percentile")
                    self.i += 1
                    p = percentile_value(self.literal())
                self.expect_op(")")
                q.aggregations.append(AggregationSpec("PERCENTILE", col, 0, p))
                if self.kw("AS"):
                    self.i += 2
                return
            if self.peek() == ("op", ","):
                self.i += 1
                log2m = int(self.literal())
            self.expect_op(")")
            if fn not in capi.AGG_FUNCTION_IDS:
                raise SqlError(f"unsupported aggregation function {fn}")
            q.aggregations.append(AggregationSpec(fn, col, log2m))
        else:
            q.select_columns.append(t[1])
        if self.kw("AS"):
            self.i += 2

    def parse(self) -> QueryContext:
        q = QueryContext()
        self.expect_kw("SELECT")
        is_distinct = self.kw("DISTINCT")
        if is_distinct:
            self.i += 1
        self.select_item(q)
        while self.peek() == ("op", ","):
            self.i += 1
            self.select_item(q)
        self.expect_kw("FROM")
        q.table = self.take()[1]
        if self.kw("WHERE"):
            self.i += 1
            q.filter = self.or_expr()
        if self.kw("GROUP"):
            self.i += 1
            self.expect_kw("BY")
            q.has_group_by = True
            q.group_by.append(self.key_expression())
            while self.peek() == ("op", ","):
                self.i += 1
                q.group_by.append(self.key_expression())
        if self.kw("ORDER"):
            self.i += 1
            self.expect_kw("BY")
            while True:
                if self.starts_expression():   # an arithmetic expression: its canonical text, as GROUP BY and the select list carry it
                    t, text = None, self.key_expression()
                else:
                    t = self.take()
                    text = t[1]
                if t is not None and self.peek() == ("op", "("):
                    depth = 0
                    in_case, last = False, ("op", "")
                    while True:
                        u = self.take()
                        if u[0] == "eof":
                            raise SqlError("unbalanced parentheses in ORDER BY")
                        in_case = in_case or (u[0] == "id" and u[1].upper() == "CASE")
                        if u[0] != "op" and last[0] != "op":   # CASE WHEN a ...: words stay apart
                            text += " "
                        text += "'%s'" % u[1].replace("'", "''") if u[0] == "str" and in_case else u[1]
                        last = u
                        if u == ("op", "("):
                            depth += 1
                        if u == ("op", ")"):
                            depth -= 1
                            if depth == 0:
                                break
                asc = True
                if self.kw("DESC"):
                    self.i += 1
                    asc = False
                elif self.kw("ASC"):
                    self.i += 1
                nulls_last = None
                if self.kw("NULLS"):
                    self.i += 1
                    if self.kw("LAST"):
                        nulls_last = True
                    elif self.kw("FIRST"):
                        nulls_last = False
                    else:
                        raise SqlError("NULLS FIRST or NULLS LAST expected")
                    self.i += 1
                q.order_by.append((text, asc))
                q.order_by_nulls_last.append(nulls_last)
                if self.peek() == ("op", ","):
                    self.i += 1
                    continue
                break
        if self.kw("LIMIT"):
            self.i += 1
            q.limit = int(self.literal())
        if self.peek()[0] != "eof":
            raise SqlError(f"trailing tokens: {self.toks[self.i:]}")
        if is_distinct:
            # DistinctPlanNode: the select list is the DISTINCT expressions; an ORDER BY expression must be one of them (the broker
            # rejects anything else) and DISTINCT does not mix with aggregations or GROUP BY
            if q.aggregations or q.has_group_by:
                raise SqlError("DISTINCT with aggregations or GROUP BY is not supported")
            if any(text not in q.select_columns for text, _ in q.order_by):
                raise SqlError("ORDER BY of a DISTINCT query must name DISTINCT columns")
            q.distinct = list(q.select_columns)
            q.flags |= capi.QUERY_FLAG_DISTINCT
        elif not q.aggregations and not q.has_group_by:
            # SelectionPlanNode: a query without aggregations, GROUP BY or DISTINCT selects rows; SELECT * stands alone
            if "*" in q.select_columns and len(q.select_columns) > 1:
                raise SqlError("SELECT * cannot be combined with other select expressions")
            q.selection = list(q.select_columns)
            q.flags |= capi.QUERY_FLAG_SELECTION
        return q


def parse_sql(sql: str) -> QueryContext:
    return _Parser(sql).parse()


# ----------------------------------------------------------------------------------------------------------------------
# QueryContext → C structs (keeps every backing object alive on the returned holder)
# ----------------------------------------------------------------------------------------------------------------------
_FILTER_TYPES = {"AND": capi.FILTER_AND, "OR": capi.FILTER_OR, "NOT": capi.FILTER_NOT,
                 "PREDICATE": capi.FILTER_PREDICATE, "CONSTANT_TRUE": capi.FILTER_CONSTANT_TRUE,
                 "CONSTANT_FALSE": capi.FILTER_CONSTANT_FALSE}
_PRED_TYPES = {"EQ": capi.PRED_EQ, "NOT_EQ": capi.PRED_NOT_EQ, "IN": capi.PRED_IN, "NOT_IN": capi.PRED_NOT_IN,
               "RANGE": capi.PRED_RANGE, "IS_NULL": capi.PRED_IS_NULL, "IS_NOT_NULL": capi.PRED_IS_NOT_NULL}


class CQuery:
    def __init__(self, q: QueryContext, column_names=None):
        """`column_names`: the segment's columns — a selection's output list (SELECT *) is built when the query is bound to a segment."""
        self._keep = []
        self.query = capi.PgQuery()
        if q.filter is not None:
            root = capi.PgFilterNode()
            self._fill(root, q.filter)
            self._keep.append(root)
            self.query.filter = C.pointer(root)
        else:
            self.query.filter = None
        if q.selection:
            if q.selection == ["*"] and column_names is None:
                raise SqlError("SELECT * needs the segment's column names")
            keys = q.extract_expressions(column_names if column_names is not None else [])
        else:
            keys = q.distinct or q.group_by
        self.output_columns = keys
        ng = len(keys)
        self.query.n_group_by = ng
        if ng:
            arr = (C.c_char_p * ng)(*[g.encode() for g in keys])
            self._keep.append(arr)
            self.query.group_by_columns = arr
        na = len(q.aggregations)
        self.query.n_aggregations = na
        if na:
            aggs = (capi.PgAggSpec * na)()
            for i, a in enumerate(q.aggregations):
                aggs[i].function = capi.AGG_FUNCTION_IDS[a.function]
                aggs[i].log2m = a.log2m
                aggs[i].column = a.column.encode() if a.column else None
            self._keep.append(aggs)
            self.query.aggregations = aggs
            if any(a.function == "PERCENTILE" for a in q.aggregations):
                params = (C.c_double * na)(*[float(a.percentile) if a.percentile is not None else 0.0 for a in q.aggregations])
                self._keep.append(params)
                self.query.agg_params = params
        self.query.num_groups_limit = q.num_groups_limit
        self.query.max_initial_result_holder_capacity = q.max_initial_result_holder_capacity
        self.query.flags = q.flags | (capi.QUERY_FLAG_DISTINCT if q.distinct else 0) | (capi.QUERY_FLAG_SELECTION if q.selection else 0)
        # segment-level group trim (GroupByOperator.java:120-133): ORDER BY + LIMIT + minSegmentGroupTrimSize travel with group-by queries
        if q.distinct:   # ORDER BY over DISTINCT columns: group-key entries
            ob = [(capi.ORDER_BY_GROUP_KEY, q.distinct.index(text), asc) for text, asc in q.order_by] or None
        elif q.selection:   # ORDER BY over output columns (ignored under LIMIT 0: EmptySelectionOperator)
            ob = [(capi.ORDER_BY_GROUP_KEY, keys.index(text), asc) for text, asc in q.order_by] if q.limit > 0 else None
            ob = ob or None
        else:
            ob = q.resolved_order_by() if (ng and q.order_by) else None
        self.query.limit = q.limit
        self.query.min_segment_group_trim_size = q.min_segment_group_trim_size
        if ob:
            arr = (capi.PgOrderBy * len(ob))()
            for i, (kind, index, asc) in enumerate(ob):
                nl = q.order_by_nulls_last[i] if i < len(q.order_by_nulls_last) else None
                arr[i].kind, arr[i].index, arr[i].ascending, arr[i].nulls_last = kind, index, int(asc), int(asc if nl is None else nl)   # NULLS LAST for ASC is the default
            self._keep.append(arr)
            self.query.order_by = arr
            self.query.n_order_by = len(ob)

    def _fill(self, node: capi.PgFilterNode, f: FilterContext):
        node.type = _FILTER_TYPES[f.type]
        n = len(f.children)
        node.n_children = n
        if n:
            arr = (capi.PgFilterNode * n)()
            self._keep.append(arr)
            for i, ch in enumerate(f.children):
                self._fill(arr[i], ch)
            node.children = arr
        if f.type == "PREDICATE":
            p = f.predicate
            node.predicate_type = _PRED_TYPES[p.type]
            node.column = p.column.encode()
            node.n_values = len(p.values)
            if p.values:
                vals = (C.c_char_p * len(p.values))(*[v.encode() for v in p.values])
                self._keep.append(vals)
                node.values = vals
            node.lower = p.lower.encode()
            node.upper = p.upper.encode()
            node.lower_inclusive = int(p.lower_inclusive)
            node.upper_inclusive = int(p.upper_inclusive)

    def ptr(self):
        return C.byref(self.query)

    def filter_ptr(self):
        return self.query.filter
