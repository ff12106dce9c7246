"""tests/fourth_moment_model.py against independent statements of the same quantities: the power-sum identities against the central sums
taken directly, the final values against scipy's bias-corrected estimators, the edge rules of n = 0 .. 4 and of a vanishing variance, the
docId-order restatement and combine() against the exact value within the reference test's RELATIVE_EPSILON (StatisticalQueriesTest: random
INT / LONG / FLOAT / DOUBLE columns, 2 000 docs, 10 groups), and the serialized bytes."""
import math
from fractions import Fraction

import numpy as np
import pytest

from tests import fourth_moment_model as fm

RELATIVE_EPSILON = 0.0001   # StatisticalQueriesTest
NUM_RECORDS, NUM_GROUPS = 2000, 10


def _columns():
    rng = np.random.default_rng(424242)
    return {
        "INT": ("INT", rng.integers(-2**31, 2**31, NUM_RECORDS).tolist()),
        "LONG": ("LONG", rng.integers(-2**63, 2**63, NUM_RECORDS).tolist()),
        "FLOAT": ("FLOAT", rng.uniform(0.0, 1.0, NUM_RECORDS).astype(np.float32).tolist()),
        "DOUBLE": ("DOUBLE", rng.uniform(0.0, 1.0, NUM_RECORDS).tolist()),
    }


COLUMNS = _columns()


@pytest.mark.parametrize("name", sorted(fm.VECTORS))
def test_power_sum_identities_equal_the_central_sums(name):
    data_type, values = fm.VECTORS[name]
    doubles = fm.as_doubles(values, data_type)[:300]
    assert fm.exact_moments(doubles) == fm.direct_moments(doubles)


def test_final_values_equal_scipy():
    stats = pytest.importorskip("scipy.stats")
    for name in ("mean1e9_double", "floats", "alternating", "negative_skew", "n4", "at_2_200"):
        data_type, values = fm.VECTORS[name]
        doubles = fm.as_doubles(values, data_type)
        t = fm.exact_tuple(doubles)
        if name == "at_2_200":   # scipy's own float moments overflow at 2^800: the statistics are scale-free
            doubles = [v * 2.0**-200 for v in doubles]
        centred = np.asarray(doubles, dtype=np.longdouble) - np.longdouble(t[1] if name != "at_2_200" else t[1] * 2.0**-200)
        assert fm.skewness(t) == pytest.approx(float(stats.skew(np.asarray(centred, dtype=np.float64), bias=False)), rel=1e-9, abs=1e-12), name
        assert fm.kurtosis(t) == pytest.approx(float(stats.kurtosis(np.asarray(centred, dtype=np.float64), fisher=True, bias=False)), rel=1e-9, abs=1e-12), name


def test_edge_rules():
    assert fm.same_tuple(fm.exact_tuple([]), (0, fm.NAN, fm.NAN, fm.NAN, fm.NAN))
    assert fm.exact_tuple([3.5]) == (1, 3.5, 0.0, 0.0, 0.0)
    t2, t3, t4 = (fm.exact_tuple([1.5, 2.5, 7.0, -3.25][:n]) for n in (2, 3, 4))
    assert math.isnan(fm.skewness(fm.exact_tuple([]))) and math.isnan(fm.skewness(fm.exact_tuple([3.5]))) and math.isnan(fm.skewness(t2))
    assert not math.isnan(fm.skewness(t3)) and math.isnan(fm.kurtosis(t3)) and not math.isnan(fm.kurtosis(t4))
    # the variance threshold: m2 / (n - 1) < 10E-20 gives 0.0 whatever m3 and m4 are
    below, above = (10, 0.0, 8.9e-19, 1e-30, 1e-40), (10, 0.0, 9.1e-19, 1e-30, 1e-40)
    assert fm.skewness(below) == 0.0 and fm.kurtosis(below) == 0.0
    assert fm.skewness(above) != 0.0 and fm.kurtosis(above) != 0.0
    assert fm.skewness(fm.exact_tuple([0.1] * 100)) == 0.0


def _close(got, want):
    return got == want or abs(got - want) <= RELATIVE_EPSILON * abs(want)


@pytest.mark.parametrize("name", sorted(COLUMNS))
def test_the_doc_order_restatement_stays_close_to_the_exact_value(name):
    data_type, values = COLUMNS[name]
    doubles = fm.as_doubles(values, data_type)
    groups = [doubles[g::NUM_GROUPS] for g in range(NUM_GROUPS)] + [doubles]
    for xs in groups:
        exact, ref = fm.exact_tuple(xs), fm.reference_tuple(xs)
        assert ref[0] == exact[0]
        for function in fm.FUNCTIONS:
            assert _close(fm.final(function, ref), fm.final(function, exact)), (name, function)
        # m3 itself is not held to a relative bound: on these symmetric random columns it is a small difference of large terms, close
        # to zero against its own rounding noise; the skewness above is m3 on the scale of m2^1.5, which is the bound that means something
        assert _close(ref[1], exact[1]) and _close(ref[2], exact[2]) and _close(ref[4], exact[4])


@pytest.mark.parametrize("name", sorted(COLUMNS))
def test_combine_of_two_halves_is_the_whole(name):
    data_type, values = COLUMNS[name]
    doubles = fm.as_doubles(values, data_type)
    half = len(doubles) // 2
    whole = fm.exact_tuple(doubles)
    merged = fm.combine(fm.exact_tuple(doubles[:half]), fm.exact_tuple(doubles[half:]))
    assert merged[0] == whole[0]
    for function in fm.FUNCTIONS:
        assert _close(fm.final(function, merged), fm.final(function, whole))
    assert fm.combine(fm.exact_tuple([]), whole) == whole and fm.combine(whole, fm.exact_tuple([])) == whole


def test_serialized_bytes():
    t = (5, 1.5, 2.0, -0.75, 1024.0)
    assert fm.to_bytes(t) == bytes.fromhex("0000000000000005" "3ff8000000000000" "4000000000000000" "bfe8000000000000" "4090000000000000")
    assert len(fm.to_bytes(fm.exact_tuple([]))) == 40 and fm.to_bytes(fm.exact_tuple([]))[:8] == bytes(8)


def test_rounding_is_once():
    # m2 of {1, 1 + 2^-52}: exactly 2^-105, far below one ulp of the sums it is the difference of
    t = fm.exact_tuple([1.0, 1.0 + 2.0**-52])
    assert t[2] == 2.0**-105 and t[4] == 2.0**-211 and t[3] == 0.0
    assert Fraction(t[2]) == fm.exact_moments([1.0, 1.0 + 2.0**-52])[2]
