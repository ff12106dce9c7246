"""tests/variance_model.py against the reference's own test (VarianceAggregationFunctionTest: the column 1, null, 2, 3, null, 6 — 1, 0, 2, 3, 6, 0
with null handling off, 1, 2, 3, 6 with it on — checked with RELATIVE_EPSILON = 1e-4 against commons-math's Variance / StandardDeviation) and
against itself: the exact tuple is the correctly rounded value, so it is never further from the truth than the docId-order restatement."""
import math
import statistics
from fractions import Fraction

import pytest

from pinot_amd.executor import variance_final, variance_merge
from tests import variance_model as vm

RELATIVE_EPSILON = 1e-4
SCENARIOS = ([1, 0, 2, 3, 6, 0], [1, 2, 3, 6])
PYTHON = {"VARPOP": statistics.pvariance, "VARSAMP": statistics.variance, "STDDEVPOP": statistics.pstdev, "STDDEVSAMP": statistics.stdev}


@pytest.mark.parametrize("values", SCENARIOS)
@pytest.mark.parametrize("function", vm.FUNCTIONS)
@pytest.mark.parametrize("grouped", [False, True])
def test_final_values_of_the_reference_scenarios(values, function, grouped):
    d = vm.as_doubles(values, "INT")
    want = PYTHON[function](values)
    for t in (vm.exact_tuple(d), vm.reference_tuple(d, grouped)):
        assert t[0] == len(values) and t[1] == sum(values)
        for got in (vm.final(function, t), variance_final(function, t)):
            assert abs(got - want) <= RELATIVE_EPSILON * abs(want), (function, t, got, want)


@pytest.mark.parametrize("function", vm.FUNCTIONS)
def test_defaults_over_no_value_and_one_value(function):
    for fin in (vm.final, variance_final):
        assert fin(function, (0, 0.0, 0.0)) == vm.NEG_INF
        one = fin(function, vm.exact_tuple([7.5]))
        assert one == (vm.NEG_INF if function in ("VARSAMP", "STDDEVSAMP") else 0.0)
    assert vm.exact_tuple([]) == (0, 0.0, 0.0) == vm.reference_tuple([])


def test_rounding_once():
    assert vm.round_fraction(Fraction(1, 3)) == 1 / 3 and vm.round_fraction(Fraction(-1, 3)) == -1 / 3
    assert vm.round_fraction(Fraction(2**53 + 1)) == 2.0**53           # a tie: to even
    assert vm.round_fraction(Fraction(2**53 + 3)) == 2.0**53 + 4
    assert vm.round_fraction(Fraction(1, 2**1075)) == 0.0              # half of the smallest subnormal: to even
    assert vm.round_fraction(Fraction(3, 2**1076)) == 5e-324
    assert vm.round_fraction(Fraction(2) ** 1024) == math.inf
    assert vm.as_doubles([2**53 + 1, -(2**62) - 1], "LONG") == [2.0**53, -(2.0**62)]   # the (double) cast comes first


@pytest.mark.parametrize("name", sorted(vm.VECTORS))
def test_exact_tuple_is_never_further_from_the_truth(name):
    data_type, values = vm.VECTORS[name]
    d = vm.as_doubles(values, data_type)
    n, sx, m2 = vm.exact_moments(d)
    got = vm.exact_tuple(d)
    assert got[0] == n and got[2] >= 0.0 and math.copysign(1.0, got[2]) == 1.0
    for grouped in (False, True):
        ref = vm.reference_tuple(d, grouped)
        assert ref[0] == n
        assert abs(Fraction(got[1]) - sx) <= abs(Fraction(ref[1]) - sx)
        assert abs(Fraction(got[2]) - m2) <= abs(Fraction(ref[2]) - m2)


@pytest.mark.parametrize("name", vm.ILL_CONDITIONED)
def test_the_reference_drifts_on_the_ill_conditioned_columns(name):
    """... so the GPU test's |gpu - exact| <= |reference - exact| is neither vacuous nor false on them: the restatement is finite and off"""
    data_type, values = vm.VECTORS[name]
    d = vm.as_doubles(values, data_type)
    _, _, m2 = vm.exact_moments(d)
    drifts = [abs(Fraction(vm.reference_tuple(d, g)[2]) - m2) for g in (False, True)]
    assert all(math.isfinite(vm.reference_tuple(d, g)[2]) for g in (False, True))
    assert max(drifts) > abs(Fraction(vm.exact_tuple(d)[2]) - m2)


def test_merge_restates_the_tuple_merge():
    a, b = [1.0, 2.0, 4.0], [8.0, 16.0]
    t = variance_merge(vm.exact_tuple(a), vm.exact_tuple(b))
    want = vm.exact_tuple(a + b)
    assert t[0] == 5 and t[1] == want[1] and abs(t[2] - want[2]) <= 1e-12 * want[2]
    assert variance_merge((0, 0.0, 0.0), vm.exact_tuple(b)) == vm.exact_tuple(b)
    assert variance_merge(vm.exact_tuple(a), (0, 0.0, 0.0)) == vm.exact_tuple(a)
    assert vm.to_bytes((3, 1.5, 0.25)).hex() == "0000000000000003" + "3ff8000000000000" + "3fd0000000000000"
