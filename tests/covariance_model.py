"""An independent model of COVAR_POP / COVAR_SAMP over decoded columns (CovarianceAggregationFunction and its intermediate
CovarianceTuple(sumX, sumY, sumXY, count)).

  exact_tuple       what the GPU path returns: count exact; sumX, sumY and sumXY the exact sums of the per-doc doubles x, y and fl(x * y) —
                    the product ROUNDED to double first, as the reference multiplies — each rounded once (nearest-even, +0.0 for a zero
                    sum), from fractions.Fraction
  reference_tuple   a restatement of what the reference computes in docId order in IEEE double — three local sums per block of 10 000 docs
                    added to the holder's tuple without GROUP BY, CovarianceTuple#apply(x, y, x * y, 1) one value at a time with one —,
                    which gives its drift from the exact value
  final             CovarianceAggregationFunction#extractFinalResult in its operation order, the -infinity cases included

and the window of pinot_amd/csrc/pg_covar.h from the header's own constants, with the vectors the host harness
(tests/test_covar_host.py) uses."""
import math
import os
import re
import struct
from fractions import Fraction

import numpy as np

from tests.variance_model import (MAX_DOC_PER_CALL, as_doubles, fx_exp_of, int_power_sums, integer_values, round_fraction, same_bits,  # noqa: F401
                                   sum_int64)   # (shared with the callers)

NEG_INF = float("-inf")
FUNCTIONS = ("COVARPOP", "COVARSAMP")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def products(xs, ys) -> list:
    """fl(x * y) per doc: one IEEE double multiply (Python's float product is one)"""
    return [x * y for x, y in zip(xs, ys)]


def exact_sum(doubles) -> Fraction:
    """the exact sum of doubles: every double is an integer times a power of two — integer sums, one Fraction at the end"""
    if len(doubles) == 0:
        return Fraction(0)
    parts = [float(v).as_integer_ratio() for v in doubles]
    scale = max(d for _, d in parts)   # a power of two
    return Fraction(sum(m * (scale // d) for m, d in parts), scale)


def exact_tuple(xs, ys) -> tuple:
    assert len(xs) == len(ys)
    return (round_fraction(exact_sum(xs)), round_fraction(exact_sum(ys)), round_fraction(exact_sum(products(xs, ys))), len(xs))


def exact_sum_of_array(d: np.ndarray) -> Fraction:
    """exact_sum over a float64 array of finite values: the 53-bit mantissas summed as integers per binary exponent"""
    d = np.asarray(d, dtype=np.float64)
    if d.size == 0:
        return Fraction(0)
    m, e = np.frexp(d)
    mant, e = np.ldexp(m, 53).astype(np.int64), e.astype(np.int64) - 53   # d = mant x 2^e, |mant| < 2^53: exact
    lowest = int(e.min())
    total = 0
    for x in np.unique(e):
        total += sum_int64(mant[e == x]) << (int(x) - lowest)
    return Fraction(total) * Fraction(2) ** lowest


def exact_tuple_of_ints(x_values, tx: str, y_values, ty: str) -> tuple:
    """exact_tuple over two INT / LONG columns, through the integer path: the sums of x and y as integers (tests/variance_model.py), the
    products fl(x * y) by one IEEE multiply each in numpy and their exact sum per exponent"""
    assert len(x_values) == len(y_values)
    xi, yi = integer_values(x_values, tx), integer_values(y_values, ty)
    xd, yd = xi.astype(np.float64), yi.astype(np.float64)   # exact: they are (double) values already
    sx, sy = int_power_sums(xi, 1)[0], int_power_sums(yi, 1)[0]
    return (round_fraction(Fraction(sx)), round_fraction(Fraction(sy)), round_fraction(exact_sum_of_array(xd * yd)), len(xi))


def reference_tuple(xs, ys, grouped: bool = False) -> tuple:
    """The reference's doubles in docId order.  Without GROUP BY (aggregate): per block three local sums from 0.0, then
    CovarianceTuple#apply(sumX, sumY, sumXY, length) — the first block's sums become the tuple; with GROUP BY (aggregateGroupBySV): the
    group's tuple is created from its first doc and apply(x, y, x * y, 1) adds every further one."""
    if not xs:
        return 0.0, 0.0, 0.0, 0
    if grouped:
        sx, sy, sxy, n = xs[0], ys[0], xs[0] * ys[0], 1
        for x, y in zip(xs[1:], ys[1:]):
            sx += x
            sy += y
            sxy += x * y
            n += 1
        return sx, sy, sxy, n
    holder = None
    for b0 in range(0, len(xs), MAX_DOC_PER_CALL):
        sx = sy = sxy = 0.0
        bx, by = xs[b0:b0 + MAX_DOC_PER_CALL], ys[b0:b0 + MAX_DOC_PER_CALL]
        for x, y in zip(bx, by):
            sx += x
            sy += y
            sxy += x * y
        holder = [sx, sy, sxy, len(bx)] if holder is None else [holder[0] + sx, holder[1] + sy, holder[2] + sxy, holder[3] + len(bx)]
    return tuple(holder)


def final(function: str, t) -> float:
    """extractFinalResult: (sumXY / count) - (sumX * sumY) / (count * count), for COVAR_SAMP (sumXY / (count - 1)) - (sumX * sumY) /
    (count * (count - 1)) — count a long, so the products of counts are exact longs converted once —; Double.NEGATIVE_INFINITY for count 0
    and, for COVAR_SAMP, count 1"""
    sx, sy, sxy, n = t
    sample = function == "COVARSAMP"
    if n == 0 or (sample and n == 1):
        return NEG_INF
    with np.errstate(all="ignore"):
        sx, sy, sxy = np.float64(sx), np.float64(sy), np.float64(sxy)
        if sample:
            return float(sxy / np.float64(n - 1) - (sx * sy) / np.float64(n * (n - 1)))
        return float(sxy / np.float64(n) - (sx * sy) / np.float64(n * n))


def merge(a, b) -> tuple:
    """CovarianceTuple#apply(CovarianceTuple)"""
    return a[0] + b[0], a[1] + b[1], a[2] + b[2], a[3] + b[3]


def to_bytes(t) -> bytes:
    """CovarianceTuple#toBytes: double sumX, double sumY, double sumXY, long count, big-endian (the count LAST, unlike VarianceTuple)"""
    return struct.pack(">dddq", float(t[0]), float(t[1]), float(t[2]), int(t[3]))


def from_bytes(b: bytes) -> tuple:
    return struct.unpack(">dddq", b)


# ---- the window of pg_covar.h, from the header's own constants -----------------------------------------------------------------------------------
def header_constants() -> dict:
    text = open(os.path.join(ROOT, "pinot_amd", "csrc", "pg_covar.h")).read()
    k = {name: int(re.search(r"#define %s (\d+)" % name, text).group(1))
         for name in ("PG_COVAR_PROD_LIMBS", "PG_COVAR_INT_EXP", "PG_COVAR_MAX_COLS", "PG_COVAR_MAX_PAIRS", "PG_COVAR_INT_SLOTS")}
    var = open(os.path.join(ROOT, "pinot_amd", "csrc", "pg_moments.h")).read()
    for name in ("PG_VAR_SUM_LIMBS", "PG_VAR_LONG_EXP"):
        k[name] = int(re.search(r"#define %s (\d+)" % name, var).group(1))
    k["PG_COVAR_DBL_SLOTS"] = k["PG_VAR_SUM_LIMBS"]
    k["PG_COVAR_WINDOW"] = 32 * k["PG_COVAR_PROD_LIMBS"] - 53
    dev = open(os.path.join(ROOT, "pinot_amd", "csrc", "pg_device.h")).read()
    k["PG_COVAR_LDS_SLOTS"] = int(re.search(r"#define PG_COVAR_LDS_SLOTS (\d+)", dev).group(1))
    return k


def column_exp(data_type: str, doubles, k: dict = None) -> int:
    """the plan-time bound E of a column: every |value| < 2^E (the type's for INT / LONG, fx_exp for FLOAT / DOUBLE)"""
    k = k or header_constants()
    if data_type == "INT":
        return k["PG_COVAR_INT_EXP"]
    if data_type == "LONG":
        return k["PG_VAR_LONG_EXP"]
    return fx_exp_of(max((abs(v) for v in doubles), default=0.0))


def prod_scale(Ep: int, k: dict = None) -> int:
    k = k or header_constants()
    return Ep - 32 * k["PG_COVAR_PROD_LIMBS"] + 1


def slots_per_group(types_of_columns, n_pairs: int, k: dict = None) -> int:
    """slot 0 the count, then the columns' sums, then the pairs' product limbs"""
    k = k or header_constants()
    return 1 + sum(k["PG_COVAR_INT_SLOTS"] if t == "INT" else k["PG_COVAR_DBL_SLOTS"] for t in types_of_columns) + n_pairs * k["PG_COVAR_PROD_LIMBS"]


def in_exact_window(xs, ys, tx: str, ty: str, k: dict = None) -> bool:
    """does the window hold every digit — of x and y in their sums (as SUM: multiples of 2^q1) and of every product (multiples of 2^qp)?"""
    k = k or header_constants()
    for t, vs in ((tx, xs), (ty, ys)):
        if t != "INT":
            q1 = column_exp(t, vs, k) - (32 * k["PG_VAR_SUM_LIMBS"] - 1)
            if any((Fraction(v) / Fraction(2) ** q1).denominator != 1 for v in vs):
                return False
    qp = prod_scale(column_exp(tx, xs, k) + column_exp(ty, ys, k), k)
    return all((Fraction(p) / Fraction(2) ** qp).denominator == 1 for p in products(xs, ys))


# ---- vectors of the host harness: name -> (type of x, values of x, type of y, values of y) ----------------------------------------------------------
def _vectors():
    rng = np.random.default_rng(20242)
    v = {}
    # INT x INT products beyond 2^53: (double) x * (double) y rounds, the int64 product would be another value
    xi = [2**31 - 1, -(2**31), 2**31 - 1, 2**30 + 12345, -(2**30) - 777, 3, 2**31 - 3] + rng.integers(2**29, 2**31, 200).tolist()
    yi = [2**31 - 3, 2**31 - 1, -(2**31), 2**30 + 54321, 2**31 - 5, -7, -(2**31) + 1] + rng.integers(-2**31, -2**29, 200).tolist()
    v["int_products_beyond_2_53"] = ("INT", xi, "INT", yi)
    big = [2**62, -2**62, 2**62 + 1, -(2**62) - 1, 2**62 - 1, 2**53 + 1, -(2**53) - 3, 2**63 - 1, -2**63]
    v["long_2_62"] = ("LONG", big * 3, "LONG", (big[::-1]) * 3)
    v["long_times_int"] = ("LONG", big * 3, "INT", rng.integers(-2**31, 2**31, 27).tolist())
    v["float_times_double"] = ("FLOAT", rng.uniform(1.0, 1000.0, 333).astype(np.float32).tolist(), "DOUBLE", rng.uniform(-5.0, 5.0, 333).tolist())
    # products that are subnormal or underflow to 0.0 (2^-600 x 2^-500 .. 2^-480): ordinary addends
    xs = (rng.uniform(1.0, 2.0, 60) * 2.0**-600).tolist()
    ys = [float(m) * 2.0**e for m, e in zip(rng.uniform(1.0, 2.0, 60), list(range(-500, -470)) * 2)]
    v["underflowing_products"] = ("DOUBLE", xs, "DOUBLE", ys)
    alt = [(-1.0) ** i * (1000.0 + (i // 2) * 0.125) for i in range(1000)]
    v["alternating_to_zero"] = ("DOUBLE", alt, "DOUBLE", [3.0] * 1000)
    v["same_column"] = ("DOUBLE", rng.standard_normal(500).tolist(), "DOUBLE", None)   # COVAR(x, x)
    v["one_doc"] = ("INT", [7], "DOUBLE", [0.5])
    return v


VECTORS = _vectors()
for _name, (_tx, _x, _ty, _y) in list(VECTORS.items()):
    if _y is None:
        VECTORS[_name] = (_tx, _x, _ty, _x)
