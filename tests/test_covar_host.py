"""The exact sums of pinot_amd/csrc/pg_covar.h — the digits the kernels of pg_kernels_covar.hip add and the one rounding per sum of the
host — as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer: tests/covar_main.cpp reads vectors from stdin and
prints limbs and result bits, which must equal tests/covariance_model.py's Fraction model bit for bit wherever the window holds every
digit, and stay within the documented bound where it does not.  (The library loaded into Python is not run under a sanitizer.)"""
import os
import struct
import subprocess
from fractions import Fraction

import pytest

from tests import covariance_model as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(v: float) -> str:
    return "%016x" % struct.unpack("<Q", struct.pack("<d", v))[0]


def _from_bits(h: str) -> float:
    return struct.unpack("<d", struct.pack("<Q", int(h, 16)))[0]


def _edge_vectors(k):
    """One pair of DOUBLE columns whose bounds are Ex = Ey = 16 (a 1.0 in each), so Ep = 32 and the products' scale is qp = Ep - 32 L + 1.
    name -> (xs, ys, exact?)"""
    qp = cm.prod_scale(32, k)
    full = float(2**53 - 1)   # 53 significant bits
    half = 2.0 ** (qp // 2)
    rest = 2.0 ** (qp - qp // 2)
    return {
        # the lowest bit of a 53-bit product weighs exactly 2^qp: the last product the window holds whole, 32 L - 53 orders below 2^Ep
        "edge_inside": ([1.0, full * half, -3.0 * half], [1.0, rest, rest], True),
        # one order lower its lowest bit weighs 2^(qp - 1): cut off, toward zero, also for a negative product
        "edge_outside": ([1.0, full * half, -full * half], [1.0, rest / 2, rest / 4], False),
        # a product below 2^qp altogether adds nothing
        "below": ([1.0, half], [1.0, rest * 0.75], False),
    }


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("covar")
    exe = str(d / "covar_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",   # the runtimes linked in: the program runs in the environment as it is
                           os.path.join(ROOT, "tests", "covar_main.cpp"), "-o", exe])
    k = cm.header_constants()
    cases = {}
    for name, (tx, x, ty, y) in cm.VECTORS.items():
        xs, ys = cm.as_doubles(x, tx), cm.as_doubles(y, ty)
        cases[name] = (tx, cm.column_exp(tx, xs, k), xs, ty, cm.column_exp(ty, ys, k), ys)
    for name, (xs, ys, _) in _edge_vectors(k).items():
        cases[name] = ("DOUBLE", 16, xs, "DOUBLE", 16, ys)
    overflow = [(1008, 16), (1008, 0), (512, 512), (496, 512), (1024, -16), (64, 960), (64, 944), (32, 32)]
    lines = ["K"] + ["O %d %d" % o for o in overflow]
    for name, (tx, Ex, xs, ty, Ey, ys) in cases.items():
        lines.append("P %s %d %s %d %d %s %s" % ("I" if tx == "INT" else "D", Ex, "I" if ty == "INT" else "D", Ey, len(xs),
                                                  " ".join(_bits(v) for v in xs), " ".join(_bits(v) for v in ys)))
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    got = out.stdout.splitlines()
    assert got[-1] == "covar ok"
    assert got[0] == "K %d %d %d %d %d" % (k["PG_COVAR_PROD_LIMBS"], k["PG_COVAR_INT_EXP"], k["PG_COVAR_MAX_COLS"], k["PG_COVAR_MAX_PAIRS"], k["PG_COVAR_WINDOW"])
    answers = {"overflow": {o: int(line.split()[1]) for o, line in zip(overflow, got[1:1 + len(overflow)])}}
    pos = 1 + len(overflow)
    for name, case in cases.items():
        q, limbs, r = got[pos].split(), got[pos + 1], got[pos + 2].split()
        assert q[0] == "Q" and limbs.startswith("L ") and r[0] == "R"
        sx, sy, sp = ([int(v) for v in part.split()] for part in limbs[2:].split("|"))
        answers[name] = {"case": case, "q1x": int(q[1]), "q1y": int(q[2]), "qp": int(q[3]), "sx": sx, "sy": sy, "sp": sp,
                         "tuple": (_from_bits(r[1]), _from_bits(r[2]), _from_bits(r[3]), int(r[4]))}
        pos += 3
    assert pos == len(got) - 1
    return answers


def _limb_value(limbs, q):
    return sum(v << (32 * j) for j, v in enumerate(limbs)) * Fraction(2) ** q


def test_the_header_keeps_its_window():
    k = cm.header_constants()
    # SUM(mult(x, y)) keeps 75 binary orders below its measured bound; the plan-time bound can sit 32 above the largest product
    assert k["PG_COVAR_WINDOW"] == 32 * k["PG_COVAR_PROD_LIMBS"] - 53 >= 75 + 32
    assert k["PG_COVAR_PROD_LIMBS"] <= 5   # what pg_limbs_to_double takes
    assert k["PG_COVAR_INT_EXP"] == 32 and k["PG_VAR_LONG_EXP"] == 64 and k["PG_COVAR_MAX_COLS"] >= 8 and k["PG_COVAR_MAX_PAIRS"] >= 8
    # integer-valued products are always exact: the scale of two LONG columns is not above 2^0
    assert cm.prod_scale(2 * k["PG_VAR_LONG_EXP"], k) <= 0


@pytest.mark.parametrize("name", sorted(cm.VECTORS))
def test_tuples_equal_the_fraction_model_bit_for_bit(harness, name):
    tx, x, ty, y = cm.VECTORS[name]
    a = harness[name]
    _, Ex, xs, _, Ey, ys = a["case"]
    assert cm.in_exact_window(xs, ys, tx, ty), name   # the model alone decides
    assert a["qp"] == cm.prod_scale(Ex + Ey)
    # the limbs hold the three sums exactly
    assert _limb_value(a["sx"], a["q1x"]) == cm.exact_sum(xs)
    assert _limb_value(a["sy"], a["q1y"]) == cm.exact_sum(ys)
    assert _limb_value(a["sp"], a["qp"]) == cm.exact_sum(cm.products(xs, ys))
    assert all(abs(v) < 2**63 for v in a["sx"] + a["sy"] + a["sp"])
    want = cm.exact_tuple(xs, ys)
    for got, w in zip(a["tuple"][:3], want[:3]):
        assert cm.same_bits(got, w), (name, a["tuple"], want)
    assert a["tuple"][3] == want[3] == len(xs)


def test_the_product_is_the_rounded_double_not_the_integer_product(harness):
    tx, x, ty, y = cm.VECTORS["int_products_beyond_2_53"]
    rounded = sum(Fraction(float(a) * float(b)) for a, b in zip(x, y))
    assert rounded != sum(a * b for a, b in zip(x, y))   # the int64 products sum to another value
    a = harness["int_products_beyond_2_53"]
    assert _limb_value(a["sp"], a["qp"]) == rounded


def test_special_values(harness):
    t = harness["alternating_to_zero"]["tuple"]
    assert _bits(t[0]) == _bits(0.0) and _bits(t[2]) == _bits(0.0) and t[1] == 3000.0   # +0.0 for a zero sum
    _, _, xs, _, _, ys = harness["underflowing_products"]["case"]
    prods = cm.products(xs, ys)
    assert any(p == 0.0 for p in prods) and any(0.0 < p < 2.0**-1022 for p in prods)   # underflow to 0.0 and to subnormals
    assert harness["underflowing_products"]["tuple"][2] > 0.0
    assert harness["one_doc"]["tuple"] == (7.0, 0.5, 3.5, 1)
    same = harness["same_column"]["tuple"]
    assert _bits(same[0]) == _bits(same[1])


def test_the_window_edges(harness):
    k = cm.header_constants()
    edges = _edge_vectors(k)
    qp = cm.prod_scale(32, k)
    for name, (xs, ys, exact) in edges.items():
        a = harness[name]
        assert a["qp"] == qp
        true = cm.exact_sum(cm.products(xs, ys))
        got = _limb_value(a["sp"], a["qp"])
        if exact:
            assert got == true and cm.same_bits(a["tuple"][2], cm.round_fraction(true)), name
        else:
            # truncated toward zero per product, by less than 2^qp each: the documented bound n 2^qp before the rounding
            errs = [Fraction(p) - (abs(Fraction(p)) // Fraction(2) ** qp) * Fraction(2) ** qp * (1 if p >= 0 else -1) for p in cm.products(xs, ys)]
            assert got == true - sum(errs) and got != true, name
            assert all(abs(e) < Fraction(2) ** qp and (e == 0 or (e > 0) == (p > 0)) for e, p in zip(errs, cm.products(xs, ys)))
            assert abs(got - true) < len(xs) * Fraction(2) ** qp
            assert cm.same_bits(a["tuple"][2], cm.round_fraction(got))
    # the edge sits where the header says: the exact vector's smallest product is PG_COVAR_WINDOW orders below the bound 2^Ep
    xs, ys, _ = edges["edge_inside"]
    p = abs(cm.products(xs, ys)[1])
    assert 2.0 ** (32 - k["PG_COVAR_WINDOW"]) <= p < 2.0 ** (32 - k["PG_COVAR_WINDOW"] + 1)


def test_the_overflow_refusal_bound(harness):
    # refused as soon as the two bounds' exponents reach 1024 together: |x y| < 2^(Ex + Ey) excludes an infinity only below that
    assert harness["overflow"] == {(1008, 16): 1, (1008, 0): 0, (512, 512): 1, (496, 512): 0, (1024, -16): 0, (64, 960): 1, (64, 944): 0, (32, 32): 0}
