"""An independent restatement of HistogramAggregationFunction in Python, for the tests: the argument rules, getBinId one IEEE double
operation at a time (Python floats are IEEE doubles: a subtraction, a division and a floor, each rounded once), the per-group arrays and
the merge.  The GPU path (pinot_amd/csrc/pg_histogram.h and the kernels of pg_kernels_hist.hip) is held to this model over the oracle's
match set; the model itself is pinned to every array of HistogramQueriesTest (tests/golden/histogram_expected.json)."""
import json
import math
import os
import re

import numpy as np

NONE, THROWS_NAN, THROWS_INDEX = -1, -2, -3
MAX_BINS, MAX_SPECS = 65536, 4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "histogram_expected.json")


class Spec:
    """kind "equal" (lower, upper, n_bins, bin_length) or "edges" (edges; lower = edges[0], upper = edges[-1])"""

    def __init__(self, kind, lower, upper, n_bins, edges=None):
        self.kind, self.lower, self.upper, self.n_bins, self.edges = kind, lower, upper, n_bins, edges
        self.bin_length = (upper - lower) / n_bins if kind == "equal" else None


def _split(text):
    """the argument list split at its commas of depth 0, blanks dropped, quotes removed: (text, quoted) pairs"""
    out, cur, depth, quoted = [], "", 0, False
    i = 0
    while i < len(text):
        ch = text[i]
        if ch == "'":
            j = text.index("'", i + 1)
            cur += text[i + 1:j]
            quoted = quoted or depth == 0
            i = j + 1
            continue
        if ch in " \t\r\n":
            i += 1
            continue
        if ch == "," and depth == 0:
            out.append((cur, quoted))
            cur, quoted = "", False
        else:
            depth += ch == "("
            depth -= ch == ")"
            cur += ch
        i += 1
    out.append((cur, quoted))
    return out


def _number(text):
    if text in ("Infinity", "+Infinity"):
        return math.inf
    if text == "-Infinity":
        return -math.inf
    if text == "NaN":
        return math.nan
    if not re.fullmatch(r"[-+]?(\d+\.?\d*|\.\d+)([eE][-+]?\d+)?", text):
        raise ValueError(f'For input string: "{text}"')
    return float(text)


def _java_double(v):
    return repr(float(v)).replace("inf", "Infinity")


def parse_arguments(text):
    """(x, Spec) of a canonical argument list; ValueError with the reference's message for the malformed forms"""
    args = _split(text)
    if len(args) not in (2, 4):
        raise ValueError(f"Histogram expects 2 or 4 arguments, got: {len(args)}; usage example: `Histogram(columnName, ARRAY[0,1,10,100])` to specify "
                         "bins [0,1), [1,10), [10,1000] or `Histogram(columnName, 0, 1000, 10)` to specify 10 equal-length bins [0,100), [100,200), ..., "
                         "[900,1000]")
    x = args[0][0]
    if len(args) == 2:
        m = re.fullmatch(r"arrayvalueconstructor\((.*)\)", args[1][0])
        if not m or args[1][1]:
            raise ValueError("Please use the format of `Histogram(columnName, ARRAY[1,10,100])` to specify the bin edges")
        parts = [p for p, _ in _split(m.group(1))] if m.group(1) else []
        if len(parts) < 2:
            raise ValueError("The number of bin edges must be greater than 1")
        edges = []
        for p in parts:
            v = _number(p)
            if edges and not v > edges[-1]:
                raise ValueError("The bin edges must be strictly increasing")
            edges.append(v)
        return x, Spec("edges", edges[0], edges[-1], len(edges) - 1, edges)
    lower, upper, bins = _number(args[1][0]), _number(args[2][0]), _number(args[3][0])
    if bins != math.floor(bins):
        raise ValueError(f'For input string: "{args[3][0]}"')
    if not upper > lower:
        raise ValueError(f"The right most edge must be greater than left most edge, given {_java_double(lower)} and {_java_double(upper)}")
    if not bins > 0:
        raise ValueError(f"The number of bins must be greater than zero, given {int(bins)}")
    return x, Spec("equal", lower, upper, int(bins))


def sql_arguments(x, args):
    """the canonical argument list of HISTOGRAM(x, <args as written in SQL>): what pinot_amd.query.parse_sql must produce"""
    m = re.fullmatch(r"\s*ARRAY\[(.*)\]\s*", args)
    if m:
        edges = [e.strip() for e in m.group(1).split(",")]
        return f"{x},arrayvalueconstructor({','.join(e.strip(chr(34)) if e.startswith(chr(34)) else chr(39) + e + chr(39) for e in edges)})"
    return x + "," + ",".join(f"'{a.strip()}'" for a in args.split(","))


def bin_of(spec, val):
    """getBinId: a bin, NONE, or one of the two inputs on which the reference throws"""
    val = float(val)
    if math.isnan(val):
        return THROWS_NAN
    if val > spec.upper or val < spec.lower:
        return NONE
    if val == spec.upper:
        return spec.n_bins - 1
    if spec.kind == "equal":
        with np.errstate(all="ignore"):
            f = np.floor(np.float64(np.float64(val) - np.float64(spec.lower)) / np.float64(spec.bin_length))
        if math.isnan(f):
            return 0
        return THROWS_INDEX if f >= spec.n_bins else int(f)
    i, j = 0, len(spec.edges) - 1
    while i < j:
        mid = (i + j + 1) // 2
        if spec.edges[mid] > val:
            j = mid - 1
        else:
            i = mid
    return i


def as_doubles(values, data_type):
    """the values as getDoubleValuesSV gives them: an INT exact, a LONG (double)-rounded, a FLOAT widened exactly"""
    if data_type == "FLOAT":
        return [float(np.float32(v)) for v in values]
    if data_type in ("INT", "LONG"):
        return [float(int(v)) for v in values]
    return [float(v) for v in values]


class Throws(Exception):
    pass


def histogram(spec, doubles):
    """the count array of one group as a tuple of floats; Throws where the reference throws"""
    out = [0.0] * spec.n_bins
    for v in doubles:
        b = bin_of(spec, v)
        if b < NONE:
            raise Throws(b)
        if b >= 0:
            out[b] += 1.0
    return tuple(out)


def merge(a, b):
    """DoubleVectorOpUtils#vectorAdd"""
    if len(a) != len(b):
        raise ValueError(f"The two operand arrays are not of the same size! provided {len(a)}, {len(b)}")
    return tuple(x + y for x, y in zip(a, b))


def golden():
    return json.load(open(GOLDEN))


def golden_columns(g=None):
    """the four columns of HistogramQueriesTest as numpy arrays, and their data types"""
    g = g or golden()
    i = np.arange(g["num_records"])
    data = {"intColumn": i.astype(np.int32), "longColumn": (i - g["num_records"] // 2).astype(np.int64),
            "floatColumn": (i * 0.5).astype(np.float32), "doubleColumn": i.astype(np.float64)}
    return data, {k: v["type"] for k, v in g["columns"].items()}


def header_constants():
    """the #defines of the path in pinot_amd/csrc/pg_device.h and pg_histogram.h"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "pinot_amd", "csrc", "pg_device.h")).read() + open(os.path.join(root, "pinot_amd", "csrc", "pg_histogram.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (PG_HIST_\w+) (\d+)", text)}
