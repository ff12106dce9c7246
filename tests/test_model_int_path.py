"""The integer power-sum path of the variance, covariance and fourth-moment models (exact_tuple_of_ints: numpy sums totalled as Python ints,
what tests/test_gpu_side_scale.py holds the kernels to over millions of docs) against their Fraction path, bit for bit: every INT / LONG
vector of each model's VECTORS, and random vectors of up to 5 000 values with the types' extremes planted."""
import numpy as np
import pytest

from tests import covariance_model as cm
from tests import fourth_moment_model as fm
from tests import variance_model as vm

INT_EXTREMES = [-2**31, 2**31 - 1, 0, -1, 1]
LONG_EXTREMES = [-2**63, 2**63 - 1, 2**62 + 1, -(2**62) - 1, 2**53 + 1, -(2**53) - 3, 0]   # (double) rounds some of them, 2^63 - 1 up to 2^63


def _random(data_type, n, seed, extremes=True):
    rng = np.random.default_rng(seed)
    if data_type == "INT":
        v = rng.integers(-2**31, 2**31, n, dtype=np.int64)
        planted = INT_EXTREMES
    else:
        v = rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64) >> rng.integers(0, 60, n)   # every magnitude
        planted = LONG_EXTREMES
    if extremes:
        v[rng.permutation(n)[:len(planted)]] = planted[:n]
    return v.tolist()


def _single():
    cases = []
    for model in (vm, fm):
        for name, (data_type, values) in model.VECTORS.items():
            if data_type in ("INT", "LONG"):
                cases.append(pytest.param(data_type, values, id=f"{model.__name__.split('.')[-1]}-{name}"))
    for data_type in ("INT", "LONG"):
        for n, seed in ((0, 1), (1, 2), (2, 3), (63, 4), (1000, 5), (5000, 6)):
            cases.append(pytest.param(data_type, _random(data_type, n, seed), id=f"random-{data_type}-{n}"))
        cases.append(pytest.param(data_type, _random(data_type, 5000, 7, extremes=False), id=f"random-{data_type}-5000-plain"))
    cases.append(pytest.param("INT", [2**31 - 1] * 5000, id="int-max-5000"))        # the largest sums an INT column reaches
    cases.append(pytest.param("INT", [-2**31] * 4999, id="int-min-4999"))
    cases.append(pytest.param("LONG", [2**63 - 1] * 3000 + [-2**63] * 2000, id="long-extremes-5000"))
    cases.append(pytest.param("LONG", [3] * 100 + [-4] * 50, id="small-longs"))       # every power stays in int64
    return cases


@pytest.mark.parametrize("data_type, values", _single())
def test_variance_and_fourth_moment_tuples(data_type, values):
    doubles = vm.as_doubles(values, data_type)
    got, want = vm.exact_tuple_of_ints(values, data_type), vm.exact_tuple(doubles)
    assert got[0] == want[0] and vm.same_bits(got[1], want[1]) and vm.same_bits(got[2], want[2]), (got, want)
    got4, want4 = fm.exact_tuple_of_ints(values, data_type), fm.exact_tuple(doubles)
    assert fm.same_tuple(got4, want4), (got4, want4)


def test_power_sums_are_python_sums():
    for data_type in ("INT", "LONG"):
        values = _random(data_type, 777, 11)
        ints = vm.integer_values(values, data_type)
        exact = [int(v) for v in vm.as_doubles(values, data_type)]
        assert vm.int_power_sums(ints, 4) == tuple(sum(v ** k for v in exact) for k in (1, 2, 3, 4))
    a = np.array([-2**63, 2**63 - 1, -1, 2**32, -2**32 - 1] * 1000, dtype=np.int64)
    assert vm.sum_int64(a) == sum(int(v) for v in a)


def _pairs():
    cases = []
    for name, (tx, xs, ty, ys) in cm.VECTORS.items():
        if tx in ("INT", "LONG") and ty in ("INT", "LONG"):
            cases.append(pytest.param(tx, xs, ty, ys, id=name))
    for tx, ty, n, seed in (("INT", "INT", 5000, 21), ("INT", "LONG", 4000, 22), ("LONG", "INT", 1, 23), ("LONG", "LONG", 5000, 24), ("INT", "INT", 0, 25)):
        cases.append(pytest.param(tx, _random(tx, n, seed), ty, _random(ty, n, seed + 100), id=f"random-{tx}-{ty}-{n}"))
    same = _random("LONG", 3000, 31)
    cases.append(pytest.param("LONG", same, "LONG", same, id="same-column"))
    return cases


@pytest.mark.parametrize("tx, xs, ty, ys", _pairs())
def test_covariance_tuples(tx, xs, ty, ys):
    got = cm.exact_tuple_of_ints(xs, tx, ys, ty)
    want = cm.exact_tuple(cm.as_doubles(xs, tx), cm.as_doubles(ys, ty))
    assert got[3] == want[3] and all(cm.same_bits(g, w) for g, w in zip(got[:3], want[:3])), (got, want)


def test_exact_sum_of_array_is_exact_sum():
    rng = np.random.default_rng(41)
    d = np.concatenate((rng.standard_normal(2000) * 2.0 ** rng.integers(-200, 200, 2000), [0.0, -0.0, 5e-324, -5e-324, 1.7e308, -1.7e308, 2.0**126]))
    assert cm.exact_sum_of_array(d) == cm.exact_sum(d.tolist())
    assert cm.exact_sum_of_array(np.zeros(0)) == 0
