"""MODE as ModeAggregationFunction computes it, restated independently of pinot_amd: the argument rules, the maps typed by the column's
stored type, merge, the three extractFinalResult loops as the reference writes them, and the two rules the GPU path defines rather than
copies — keys ordered as Double.compare orders them (so a tie at the greatest count that involves NaN or both zeros has one answer, where
the reference's depends on its hash map's iteration order), and AVG's sum as the exact sum of the tied keys, rounded once (Fraction)."""
import math
import struct
from fractions import Fraction

import numpy as np

REDUCERS = ("MIN", "MAX", "AVG")
NEG_INF = float("-inf")
MAP_CLASS = {"INT": "Int2LongOpenHashMap", "LONG": "Long2LongOpenHashMap", "FLOAT": "Float2LongOpenHashMap", "DOUBLE": "Double2LongOpenHashMap"}
OBJECT_TYPE = {"INT": 23, "LONG": 24, "FLOAT": 25, "DOUBLE": 26}   # ObjectSerDeUtils: Int2LongMap .. Double2LongMap
ENUM = "org.apache.pinot.core.query.aggregation.function.ModeAggregationFunction.MultiModeReducerType"


def parse_arguments(text: str):
    """(column, reducer) of an argument list "x" / "x,'MAX'": commas at depth 0, blanks ignored; ValueError with the reference's text"""
    args, cur, depth, quoted, in_quote = [], "", 0, False, False
    for ch in text:
        if in_quote:
            if ch == "'":
                in_quote = False
            else:
                cur += ch
            continue
        if ch == "'":
            if depth == 0 and (cur or quoted):
                raise ValueError("text next to a quoted literal")
            in_quote, quoted = True, quoted or depth == 0
        elif ch in " \t\r\n":
            continue
        elif quoted and depth == 0 and ch != ",":
            raise ValueError("text next to a quoted literal")
        elif ch == "," and depth == 0:
            args.append((cur, quoted))
            cur, quoted = "", False
        else:
            depth += ch == "("
            depth -= ch == ")"
            cur += ch
    args.append((cur, quoted))
    if not any(a or q for a, q in args):
        raise ValueError("empty argument list")
    if in_quote or depth != 0 or any(a == "" and not q for a, q in args):
        raise ValueError("malformed argument list")
    if len(args) > 2:
        raise ValueError("Mode expects at most 2 arguments, got: %d" % len(args))
    if args[0][1]:
        raise ValueError("the first argument must be a column")
    if len(args) == 2:
        if not args[1][1]:
            raise ValueError("the reducer is a quoted literal")
        if args[1][0] not in REDUCERS:   # MultiModeReducerType.valueOf: exact, upper case
            raise ValueError("No enum constant %s.%s" % (ENUM, args[1][0]))
    return args[0][0], (args[1][0] if len(args) == 2 else "MIN")


def _bits(v: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def compare_key(k):
    """sorts keys as Integer / Long / Float / Double.compare does: -0.0 < 0.0, NaN greatest (one NaN)"""
    if isinstance(k, float):
        if k != k:
            return 1 << 65
        b = _bits(k)
        return (1 << 63) - (b & ((1 << 63) - 1)) - 1 if b >> 63 else (1 << 63) + b
    return (1 << 63) + int(k)


def typed_keys(values, data_type: str):
    """the keys as the typed map holds them: Python ints for INT / LONG, floats for FLOAT (widened exactly) / DOUBLE, every NaN one key"""
    if data_type in ("INT", "LONG"):
        return [int(v) for v in np.asarray(values, dtype=np.int64)]
    if data_type == "FLOAT":
        return [float(v) for v in np.asarray(values, dtype=np.float32).astype(np.float64)]
    return [float(v) for v in np.asarray(values, dtype=np.float64)]


def value_map(values, data_type: str):
    """(type, ((key, count), ...)) ascending by key; an empty map is the Int2LongOpenHashMap whatever the column's type"""
    counts = {}
    for k in typed_keys(values, data_type):
        ck = compare_key(k)
        counts[ck] = (k, counts[ck][1] + 1) if ck in counts else (k, 1)
    entries = tuple(counts[ck] for ck in sorted(counts))
    return (data_type, entries) if entries else ("INT", ())


def merge(a, b):
    if not a[1]:
        return b
    if not b[1]:
        return a
    if a[0] != b[0]:
        raise ValueError("Illegal data type for Intermediate Result of MODE aggregation function: %s, %s" % (MAP_CLASS[a[0]], MAP_CLASS[b[0]]))
    counts = {}
    for k, c in a[1] + b[1]:
        ck = compare_key(k)
        counts[ck] = (k, counts[ck][1] + c) if ck in counts else (k, c)
    return (a[0], tuple(counts[ck] for ck in sorted(counts)))


def reference_final(entries, reducer: str) -> float:
    """extractFinalResult's loops as written, over the entries in the given iteration order (keys compared with < / >, the AVG sum a
    running double)"""
    it = iter(entries)
    first_key, max_frequency = next(it)
    if reducer == "MIN":
        best = first_key
        for k, c in it:
            if c > max_frequency or (c == max_frequency and best > k):
                max_frequency, best = c, k
        return float(best)
    if reducer == "MAX":
        best = first_key
        for k, c in it:
            if c > max_frequency or (c == max_frequency and best < k):
                max_frequency, best = c, k
        return float(best)
    if reducer != "AVG":
        raise ValueError("Illegal reducer type for MODE aggregation function: " + reducer)
    total, count = float(first_key), 1
    for k, c in it:
        if c > max_frequency:
            max_frequency, total, count = c, float(k), 1
        elif c == max_frequency:
            total += float(k)
            count += 1
    return total / count


def final(m, reducer: str = "MIN") -> float:
    """the defined final value: ties in Double.compare order; AVG = the exact sum of the tied keys as doubles, rounded once, / their number"""
    if reducer not in REDUCERS:
        raise ValueError("No enum constant %s.%s" % (ENUM, reducer))
    if not m[1]:
        return NEG_INF
    top = max(c for _, c in m[1])
    tied = [float(k) for k, c in m[1] if c == top]
    if reducer == "MIN":
        return tied[0]
    if reducer == "MAX":
        return tied[-1]
    if any(t != t for t in tied) or (math.inf in tied and -math.inf in tied):
        return math.nan
    if math.inf in tied or -math.inf in tied:
        return math.inf if math.inf in tied else -math.inf
    exact = sum(Fraction(t) for t in tied)
    try:
        total = float(exact)   # one rounding, to nearest even
    except OverflowError:
        total = math.inf if exact > 0 else -math.inf
    return total / len(tied)


def order_free(m) -> bool:
    """does the reference's answer not depend on its iteration order?  Not when a tie at the greatest count involves NaN or both zeros."""
    if not m[1]:
        return True
    top = max(c for _, c in m[1])
    tied = [k for k, c in m[1] if c == top]
    has_nan = any(isinstance(k, float) and k != k for k in tied)
    zeros = [k for k in tied if isinstance(k, float) and k == 0.0]
    return not (len(tied) > 1 and (has_nan or len(zeros) > 1))


def serialize(m) -> tuple:
    """(ObjectSerDeUtils type, bytes): int size, then (key in its own width, long count) entries, big-endian, ascending by key"""
    t, entries = m
    out = struct.pack(">i", len(entries))
    for k, c in entries:
        out += {"INT": lambda: struct.pack(">i", k), "LONG": lambda: struct.pack(">q", k), "FLOAT": lambda: struct.pack(">f", k),
                "DOUBLE": lambda: struct.pack(">d", k)}[t]() + struct.pack(">q", c)
    return (OBJECT_TYPE[t] if entries else 23), out


def deserialize(kind: int, b: bytes):
    t = {v: k for k, v in OBJECT_TYPE.items()}[kind]
    n = struct.unpack_from(">i", b)[0]
    fmt, width = {"INT": (">i", 4), "LONG": (">q", 8), "FLOAT": (">f", 4), "DOUBLE": (">d", 8)}[t]
    entries, at = [], 4
    for _ in range(n):
        k = struct.unpack_from(fmt, b, at)[0]
        c = struct.unpack_from(">q", b, at + width)[0]
        entries.append((k, c))
        at += width + 8
    assert at == len(b)
    return (t if entries else "INT", tuple(entries))


def same_map(a, b) -> bool:
    """bit for bit: the type, the counts, and the keys with every NaN one value"""
    return a[0] == b[0] and len(a[1]) == len(b[1]) and all(
        type(x[0]) is type(y[0]) and compare_key(x[0]) == compare_key(y[0]) and x[1] == y[1] for x, y in zip(a[1], b[1]))


def same_double(a: float, b: float) -> bool:
    return (a != a and b != b) or _bits(float(a)) == _bits(float(b))


def combine(a, b):
    """the selection's partial (max_count, n_tied, lowest tied id, highest tied id); None: no counted id"""
    if a is None or b is None:
        return a if b is None else b
    if a[0] != b[0]:
        return a if a[0] > b[0] else b
    return (a[0], a[1] + b[1], min(a[2], b[2]), max(a[3], b[3]))


def partial_of_row(counts, first_id=0):
    """the whole range's partial, by definition rather than by combining"""
    top = max(counts, default=0)
    if top == 0:
        return None
    tied = [first_id + i for i, c in enumerate(counts) if c == top]
    return (top, len(tied), tied[0], tied[-1])
