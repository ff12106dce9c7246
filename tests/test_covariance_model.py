"""tests/covariance_model.py pinned: its final values against numpy.cov on the kinds of data the reference's own test uses
(StatisticalQueriesTest: random INT, LONG, FLOAT and DOUBLE columns of 2 000 rows in 10 groups, values in [-500, 500), checked there with
RELATIVE_EPSILON = 1e-4), the count-0 and count-1 defaults, CovarianceTuple#toBytes' field order, and the model against itself: the exact
tuple is the correctly rounded value, so it is never further from the truth than the docId-order restatement."""
import math
import struct
from fractions import Fraction

import numpy as np
import pytest

from pinot_amd.executor import covariance_final, covariance_merge
from tests import covariance_model as cm

RELATIVE_EPSILON = 1e-4
NUM_RECORDS, NUM_GROUPS, MAX_VALUE = 2000, 10, 500


def _columns():
    rng = np.random.default_rng(5)
    return {
        "INT": rng.integers(-MAX_VALUE, MAX_VALUE, NUM_RECORDS).tolist(),
        "INT2": rng.integers(-MAX_VALUE, MAX_VALUE, NUM_RECORDS).tolist(),
        "LONG": rng.integers(-MAX_VALUE, MAX_VALUE, NUM_RECORDS).tolist(),
        "FLOAT": (-MAX_VALUE + rng.random(NUM_RECORDS, dtype=np.float32) * 2 * MAX_VALUE).tolist(),
        "DOUBLE": rng.uniform(-MAX_VALUE, MAX_VALUE, NUM_RECORDS).tolist(),
        "DOUBLE2": rng.uniform(-MAX_VALUE, MAX_VALUE, NUM_RECORDS).tolist(),
    }


COLUMNS = _columns()
# the pairs of the reference's 8-covariance query
PAIRS = [("INT", "INT2"), ("DOUBLE", "DOUBLE2"), ("INT", "DOUBLE"), ("INT", "LONG"), ("INT", "FLOAT"), ("DOUBLE", "LONG"), ("DOUBLE", "FLOAT"), ("LONG", "FLOAT")]


def _doubles(name):
    return cm.as_doubles(COLUMNS[name], name.rstrip("2"))


@pytest.mark.parametrize("x,y", PAIRS)
@pytest.mark.parametrize("grouped", [False, True])
def test_final_values_agree_with_numpy_cov(x, y, grouped):
    xs, ys = _doubles(x), _doubles(y)
    size = NUM_RECORDS // NUM_GROUPS
    spans = [(g * size, (g + 1) * size) for g in range(NUM_GROUPS)] if grouped else [(0, NUM_RECORDS)]
    for lo, hi in spans:
        gx, gy = xs[lo:hi], ys[lo:hi]
        for t in (cm.exact_tuple(gx, gy), cm.reference_tuple(gx, gy, grouped)):
            assert t[3] == hi - lo
            for function, bias in (("COVARPOP", True), ("COVARSAMP", False)):
                want = float(np.cov(np.array(gx), np.array(gy), bias=bias)[0, 1])
                for got in (cm.final(function, t), covariance_final(function, t)):
                    assert abs(got - want) <= RELATIVE_EPSILON * abs(want), (function, x, y, got, want)


@pytest.mark.parametrize("function", cm.FUNCTIONS)
def test_defaults_over_no_doc_and_one_doc(function):
    for fin in (cm.final, covariance_final):
        assert fin(function, (0.0, 0.0, 0.0, 0)) == cm.NEG_INF
        one = fin(function, cm.exact_tuple([7.5], [2.0]))
        assert one == (cm.NEG_INF if function == "COVARSAMP" else 0.0)
    assert cm.exact_tuple([], []) == (0.0, 0.0, 0.0, 0) == cm.reference_tuple([], [])
    assert all(math.copysign(1.0, v) == 1.0 for v in cm.exact_tuple([], [])[:3])   # +0.0


def test_the_final_formulas_keep_the_reference_operation_order():
    # a tuple on which another grouping of the operations rounds differently: (sumXY / n) - (sumX * sumY) / (n * n), never (sumXY - sumX sumY / n) / n
    t = (1e8 + 1.0, 3.0, 3e8 + 0.1, 7)
    pop = (t[2] / 7.0) - (t[0] * t[1]) / 49.0
    samp = (t[2] / 6.0) - (t[0] * t[1]) / 42.0
    for fin in (cm.final, covariance_final):
        assert fin("COVARPOP", t) == pop and fin("COVARSAMP", t) == samp
    assert pop != (t[2] - t[0] * t[1] / 7.0) / 7.0


def test_to_bytes_field_order():
    t = (1.5, -2.25, 1e300, 12345678901)
    b = cm.to_bytes(t)
    assert len(b) == 32
    assert b == struct.pack(">d", 1.5) + struct.pack(">d", -2.25) + struct.pack(">d", 1e300) + struct.pack(">q", 12345678901)   # the count LAST
    assert cm.from_bytes(b) == t


def test_merge_adds_member_by_member():
    a, b = (1.0, 2.0, 3.0, 4), (0.5, 0.25, 0.125, 1)
    assert cm.merge(a, b) == covariance_merge(a, b) == (1.5, 2.25, 3.125, 5)


def test_the_product_is_rounded_before_it_is_summed():
    x, y = [float(2**31 - 1)] * 3, [float(2**31 - 3)] * 3
    assert cm.exact_tuple(x, y)[2] == cm.round_fraction(3 * Fraction(x[0] * y[0]))
    assert Fraction(x[0] * y[0]) != (2**31 - 1) * (2**31 - 3)


@pytest.mark.parametrize("name", sorted(cm.VECTORS))
def test_exact_tuple_is_never_further_from_the_truth(name):
    tx, x, ty, y = cm.VECTORS[name]
    xs, ys = cm.as_doubles(x, tx), cm.as_doubles(y, ty)
    truth = (cm.exact_sum(xs), cm.exact_sum(ys), cm.exact_sum(cm.products(xs, ys)))
    got = cm.exact_tuple(xs, ys)
    for grouped in (False, True):
        ref = cm.reference_tuple(xs, ys, grouped)
        assert ref[3] == got[3] == len(xs)
        for k in range(3):
            assert abs(Fraction(got[k]) - truth[k]) <= abs(Fraction(ref[k]) - truth[k])
