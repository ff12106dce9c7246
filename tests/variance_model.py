"""An independent model of VAR_POP / VAR_SAMP / STDDEV_POP / STDDEV_SAMP over decoded columns (VarianceAggregationFunction and its
intermediate VarianceTuple(count, sum, m2)).

  exact_tuple       what the GPU path returns: count exact, sum = the exact sum rounded once, m2 = the exact sum x^2 - (sum x)^2 / n rounded
                    once (nearest-even), from fractions.Fraction
  reference_tuple   a restatement of what the reference computes in docId order in IEEE double — VarianceTuple#apply(double) per block of
                    10 000 docs without GROUP BY, VarianceTuple#apply(1, value, 0.0) per doc with one —, which gives its drift from the exact
                    value
  final             VarianceAggregationFunction#extractFinalResult for the four functions, the -infinity cases included

and the vectors the host harness (tests/test_moments_host.py) and the GPU tests (tests/test_gpu_variance.py) share."""
import math
import re
import os
from fractions import Fraction

import numpy as np

NEG_INF = float("-inf")
FUNCTIONS = ("VARPOP", "VARSAMP", "STDDEVPOP", "STDDEVSAMP")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_DOC_PER_CALL = 10000   # DocIdSetPlanNode.MAX_DOC_PER_CALL: the reference aggregates block by block


def as_doubles(values, data_type: str) -> list:
    """getDoubleValuesSV of a column's values as Python floats: an INT exact, a LONG (double) rounded to nearest-even first, a FLOAT widened
    exactly."""
    if data_type in ("INT", "LONG"):
        return [float(int(v)) for v in values]   # int -> float rounds to nearest-even, as (double) does
    if data_type == "FLOAT":
        return [float(v) for v in np.asarray(values, dtype=np.float32).astype(np.float64)]
    return [float(v) for v in np.asarray(values, dtype=np.float64)]


def round_fraction(x: Fraction) -> float:
    """`x` rounded ONCE to the nearest double, ties to even, subnormals included; beyond the largest double: infinity."""
    if x == 0:
        return 0.0
    sign = -1.0 if x < 0 else 1.0
    n, d = abs(x.numerator), x.denominator
    e = n.bit_length() - d.bit_length()
    if (n >> e if e >= 0 else n << -e) < d:
        e -= 1                                   # 2^e <= n / d < 2^(e + 1)
    lsb = max(e - 52, -1074)                     # the lowest bit a double of this size keeps
    num, den = (n, d << lsb) if lsb >= 0 else (n << -lsb, d)
    q, r = divmod(num, den)
    if 2 * r > den or (2 * r == den and (q & 1)):
        q += 1
    try:
        return sign * math.ldexp(float(q), lsb)   # q <= 2^53: exact
    except OverflowError:
        return sign * math.inf


def _moments_of_sums(n: int, sx: int, sq: int, scale: int):
    """(n, sum x, sum x^2 - (sum x)^2 / n) from the integer power sums of the values times `scale`"""
    if n == 0:
        return 0, Fraction(0), Fraction(0)
    return n, Fraction(sx, scale), Fraction(n * sq - sx * sx, n * scale * scale)


def exact_moments(doubles):
    """(n, sum x, sum x^2 - (sum x)^2 / n) as exact Fractions (m2 = 0 for n = 0)"""
    n = len(doubles)
    if n == 0:
        return 0, Fraction(0), Fraction(0)
    # every double is an integer times 2^-1074: integer sums, one Fraction at the end (the same values as summing Fractions, much faster)
    parts = [v.as_integer_ratio() for v in doubles]
    scale = max(d for _, d in parts)   # a power of two
    ints = [m * (scale // d) for m, d in parts]
    return _moments_of_sums(n, sum(ints), sum(i * i for i in ints), scale)


def exact_tuple(doubles) -> tuple:
    n, sx, m2 = exact_moments(doubles)
    return n, round_fraction(sx), round_fraction(m2)


# ---- the integer path: INT / LONG columns of millions of docs -----------------------------------------------------------------------------------
# The (double) of an INT or a LONG is an integer, so its power sums are integers: numpy computes them in int64 where a power stays below
# 2^62 (chunked sums of the 32-bit halves, totalled as Python ints) and in object arrays of Python ints beyond.  The sums feed the same
# construction as the Fraction path; tests/test_model_int_path.py pins the two to each other.
_CHUNK = 1 << 20


def integer_values(values, data_type: str) -> np.ndarray:
    """getDoubleValuesSV of an INT / LONG column as exact integers: an int64 array, or an object array of Python ints where a (double)-rounded
    LONG reaches 2^63"""
    assert data_type in ("INT", "LONG"), data_type
    a = np.asarray(values, dtype=np.int64)
    if data_type == "INT":
        return a
    d = a.astype(np.float64)   # rounds to nearest-even, as (double) does
    if d.size == 0 or np.abs(d).max() < 2.0**63:
        return d.astype(np.int64)
    return np.array([int(v) for v in d], dtype=object)


def sum_int64(a: np.ndarray) -> int:
    """the exact total of an int64 array as a Python int"""
    total = 0
    for c0 in range(0, a.size, _CHUNK):
        c = a[c0:c0 + _CHUNK]
        total += (int((c >> 32).sum()) << 32) + int((c & 0xFFFFFFFF).sum())   # |high halves| < 2^31 and low halves < 2^32, 2^20 of them
    return total


def int_power_sums(ints: np.ndarray, kmax: int) -> tuple:
    """(S1, .., S_kmax) of integer_values() as Python ints"""
    if len(ints) == 0:
        return (0,) * kmax
    bits = 64 if ints.dtype == object else int(np.abs(ints.astype(np.float64)).max()).bit_length()
    out, p = [], None   # p: the k-th powers, an int64 array while they stay below 2^62, then an object array of Python ints
    for k in range(1, kmax + 1):
        if k * bits <= 62:
            p = ints if k == 1 else p * ints
            out.append(sum_int64(p))
        else:
            base = ints if ints.dtype == object else ints.astype(object)
            p = base if k == 1 else (p if p.dtype == object else p.astype(object)) * base
            out.append(int(p.sum()))
    return tuple(out)


def exact_tuple_of_ints(values, data_type: str) -> tuple:
    """exact_tuple(as_doubles(values, data_type)) for an INT / LONG column, through the integer path"""
    ints = integer_values(values, data_type)
    n, sx, m2 = _moments_of_sums(len(ints), *int_power_sums(ints, 2), 1)
    return n, round_fraction(sx), round_fraction(m2)


def _merge(t, count, s, m2):
    """VarianceTuple#apply(long count, double sum, double m2) on t = [count, sum, m2]"""
    if count == 0:
        return
    avg = 0.0 if t[0] == 0 else t[1] / t[0]
    delta = (s / count) - avg
    t[2] += m2 + delta * delta * float(count) * float(t[0]) / float(count + t[0])
    t[0] += count
    t[1] += s


def reference_tuple(doubles, grouped: bool = False) -> tuple:
    """The reference's doubles in docId order.  Without GROUP BY: per block a fresh tuple updated by apply(double), merged into the holder;
    with GROUP BY: the group's tuple created from its first value and merged with (1, value, 0.0) per further doc."""
    if not doubles:
        return 0, 0.0, 0.0
    if grouped:
        t = [1, doubles[0], 0.0]
        for v in doubles[1:]:
            _merge(t, 1, v, 0.0)
        return t[0], t[1], t[2]
    holder = None
    for b0 in range(0, len(doubles), MAX_DOC_PER_CALL):
        count, s, m2 = 0, 0.0, 0.0
        for v in doubles[b0:b0 + MAX_DOC_PER_CALL]:
            count += 1
            s += v
            if count > 1:
                t = float(count) * v - s
                m2 += (t * t) / float(count * (count - 1))
        if holder is None:
            holder = [count, s, m2]
        else:
            _merge(holder, count, s, m2)
    return holder[0], holder[1], holder[2]


def final(function: str, t) -> float:
    """extractFinalResult: Double.NEGATIVE_INFINITY for count 0 and, for the sample forms, count 1"""
    n, _, m2 = t
    sample = function in ("VARSAMP", "STDDEVSAMP")
    if n == 0 or (sample and n == 1):
        return NEG_INF
    v = m2 / (n - 1) if sample else m2 / n
    return math.sqrt(v) if function.startswith("STDDEV") else v


def to_bytes(t) -> bytes:
    """VarianceTuple#toBytes: long count, double sum, double m2, big-endian"""
    import struct
    return struct.pack(">qdd", int(t[0]), float(t[1]), float(t[2]))


def same_bits(a: float, b: float) -> bool:
    return np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64)


# ---- the window of pg_moments.h, from the header's own constants -------------------------------------------------------------------------------
def header_constants() -> dict:
    text = open(os.path.join(ROOT, "pinot_amd", "csrc", "pg_moments.h")).read()
    return {k: int(re.search(r"#define %s (\d+)" % k, text).group(1)) for k in ("PG_VAR_SUM_LIMBS", "PG_VAR_SQ_LIMBS", "PG_VAR_INT_SLOTS", "PG_VAR_LONG_EXP")}


def fx_exp_of(max_abs: float) -> int:
    """the planner's bound E for a FLOAT / DOUBLE column (pg_segment.cpp): a multiple of 16 with every finite |value| < 2^E"""
    if not max_abs > 0:
        return 0
    return 16 * math.floor((math.frexp(max_abs)[1] + 15) / 16)


def scales(E: int, k: dict = None) -> tuple:
    k = k or header_constants()
    return E - (32 * k["PG_VAR_SUM_LIMBS"] - 1), 2 * E - 32 * k["PG_VAR_SQ_LIMBS"] + 1


def truncation_bound(n: int, E: int, k: dict = None) -> Fraction:
    """n (2^q2 + 2^(E + q1 + 1)): how far m2 may be from the exact value BEFORE its one rounding when values fall below the window"""
    q1, q2 = scales(E, k)
    return n * (Fraction(2) ** q2 + Fraction(2) ** (E + q1 + 1))


def ulp(x: float) -> Fraction:
    return Fraction(math.ulp(x))


# ---- shared vectors: name -> (data type, values) ------------------------------------------------------------------------------------------------
def _vectors():
    rng = np.random.default_rng(20241)
    v = {}
    v["all_equal"] = ("DOUBLE", [0.1] * 100)
    v["n1"] = ("DOUBLE", [3.5])
    v["n2"] = ("DOUBLE", [1.5, 2.5])
    v["mean1e9_double"] = ("DOUBLE", (1e9 + rng.standard_normal(2000)).tolist())
    v["mean1e9_int"] = ("INT", (10**9 + rng.integers(-3, 4, 2000)).tolist())
    v["int_extremes"] = ("INT", [-2**31, 2**31 - 1, -2**31, 2**31 - 1, 0, -1, 1])
    big = [2**62, -2**62, 2**62 + 1, -(2**62) - 1, 2**62 - 1, 2**53 + 1, -(2**53) - 3, 2**63 - 1, -2**63]
    v["long_2_62"] = ("LONG", big * 3)
    v["long_2_62_same_sign"] = ("LONG", [2**62 + int(k) for k in rng.integers(0, 2**40, 500)])
    v["floats"] = ("FLOAT", rng.uniform(1.0, 1000.0, 777).astype(np.float32).tolist())
    v["subnormals"] = ("DOUBLE", [float(k) * 5e-324 for k in rng.integers(1, 1000, 300)])
    v["at_2_500"] = ("DOUBLE", (rng.uniform(1.0, 8.0, 400) * 2.0**500).tolist())
    v["mean_2_500"] = ("DOUBLE", ((1e6 + rng.standard_normal(300)) * 2.0**500).tolist())
    v["tiny_m2"] = ("DOUBLE", (rng.uniform(1.0, 2.0, 100) * 2.0**-520).tolist())   # m2 is a subnormal: one rounding at 2^-1074
    v["at_2_m500"] = ("DOUBLE", (rng.uniform(1.0, 900.0, 400) * 2.0**-500).tolist())
    v["alternating"] = ("DOUBLE", [(-1.0) ** i * (1000.0 + i * 0.125) for i in range(1001)])
    v["zeros_and_values"] = ("DOUBLE", [0.0, -0.0, 7.25, 0.0, 7.5, -0.0])
    return v


VECTORS = _vectors()
# magnitudes 2^-300 .. 2^300: most values fall below the window; held to the documented bound, not to exactness
WIDE_RANGE = ("DOUBLE", [float(m) * 2.0**int(e) for m, e in zip(np.random.default_rng(7).uniform(1, 2, 601), range(-300, 301))])
# the columns on which the reference's docId-order arithmetic drifts visibly (mean >> sigma)
ILL_CONDITIONED = ("mean1e9_double", "mean1e9_int", "long_2_62_same_sign", "mean_2_500", "floats")


def in_exact_window(doubles) -> bool:
    """non-zero magnitudes span at most 2^10: with E up to 16 above the largest exponent every value is within 2^-26 of 2^E, and the squares'
    window (pg_moments.h: 2 s <= 32 L2 - 107) holds them exactly from L2 = 5 on"""
    mags = [abs(v) for v in doubles if v != 0]
    return not mags or max(mags) <= min(mags) * 1024
