"""The exact power sums of pinot_amd/csrc/pg_moments.h — the digits the kernels of pg_kernels_var.hip add, the 512-bit helper and the one
rounding of the host — as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer: tests/moments_main.cpp reads vectors
from stdin and prints limbs and result bits, which must equal tests/variance_model.py's Fraction model bit for bit wherever the window holds
every digit, and stay within the documented bound where it does not.  (The library loaded into Python is not run under a sanitizer.)"""
import math
import os
import random
import struct
import subprocess
from fractions import Fraction

import pytest

from tests import variance_model as vm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_ONES = (1 << 512) - 1
U512 = [   # (op, a, b): carry and borrow chains through every limb
    ("mul", (1 << 256) - 1, (1 << 256) - 1), ("mul", ALL_ONES, ALL_ONES), ("mul", ALL_ONES, 1), ("mul", (1 << 511) | 1, 2), ("mul", 0, ALL_ONES),
    ("mul", int("f" * 40, 16), int("f" * 79, 16)), ("sub", 1 << 511, 1), ("sub", 0, 1), ("sub", ALL_ONES, ALL_ONES), ("sub", 1 << 320, (1 << 319) + 1),
    ("cmp", 1 << 511, (1 << 511) - 1), ("cmp", 5, 5), ("cmp", 4, 1 << 32),
    ("shl", ALL_ONES, 0), ("shl", ALL_ONES, 1), ("shl", ALL_ONES, 31), ("shl", ALL_ONES, 32), ("shl", ALL_ONES, 63), ("shl", ALL_ONES, 96), ("shl", ALL_ONES, 511), ("shl", 1, 511),
    ("mulu", ALL_ONES, 0xFFFFFFFF), ("mulu", (1 << 416) - 1, 0x7FFFFFFF), ("mulu", 12345, 0),
    ("div", ALL_ONES, 1), ("div", ALL_ONES, 0xFFFFFFFF), ("div", ALL_ONES, 0x7FFFFFFF), ("div", (1 << 416) - 1, 3), ("div", 7, 9), ("div", 1 << 511, 0x80000001),
]
random.seed(11)
U512 += [(op, random.getrandbits(random.randint(1, 512)), random.getrandbits(random.randint(1, 512))) for op in ("mul", "sub", "cmp") for _ in range(40)]
U512 += [("shl", random.getrandbits(random.randint(1, 512)), random.randint(0, 511)) for _ in range(40)]
U512 += [(op, random.getrandbits(random.randint(1, 512)), random.randint(1, 2**32 - 1)) for op in ("mulu", "div") for _ in range(40)]


def _bits(v: float) -> str:
    return "%016x" % struct.unpack("<Q", struct.pack("<d", v))[0]


def _from_bits(h: str) -> float:
    return struct.unpack("<d", struct.pack("<Q", int(h, 16)))[0]


def _exponent(data_type, doubles, k):
    return k["PG_VAR_LONG_EXP"] if data_type == "LONG" else vm.fx_exp_of(max((abs(v) for v in doubles), default=0.0))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("moments")
    exe = str(d / "moments_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",   # the runtimes linked in: the program runs in the environment as it is
                           os.path.join(ROOT, "tests", "moments_main.cpp"), "-o", exe])
    k = vm.header_constants()
    names = sorted(vm.VECTORS) + ["wide_range"]
    lines = ["K"]
    for name in names:
        data_type, values = vm.VECTORS[name] if name != "wide_range" else vm.WIDE_RANGE
        if data_type == "INT":
            lines.append("I %d %s" % (len(values), " ".join(str(int(v)) for v in values)))
        else:
            doubles = vm.as_doubles(values, data_type)
            lines.append("D %d %d %s" % (_exponent(data_type, doubles, k), len(doubles), " ".join(_bits(v) for v in doubles)))
    for op, a, b in U512:
        lines.append("U %s %x %s" % (op, a, "%x" % b if op in ("mul", "sub", "cmp") else "%d" % b))
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    got = out.stdout.splitlines()
    assert got[-1] == "moments ok"
    assert got[0] == "K %d %d %d %d" % (k["PG_VAR_SUM_LIMBS"], k["PG_VAR_SQ_LIMBS"], k["PG_VAR_INT_SLOTS"], k["PG_VAR_LONG_EXP"])
    answers, pos = {}, 1
    for name in names:
        q, limbs, r = got[pos].split(), got[pos + 1], got[pos + 2].split()
        assert q[0] == "Q" and limbs.startswith("L ") and r[0] == "R"
        sx, sq = ([int(x) for x in part.split()] for part in limbs[2:].split("|"))
        answers[name] = {"q1": int(q[1]), "q2": int(q[2]), "sx": sx, "sq": sq, "n": int(r[1]), "sum": _from_bits(r[2]), "m2": _from_bits(r[3])}
        pos += 3
    answers["u512"] = [line[2:] for line in got[pos:pos + len(U512)]]
    assert pos + len(U512) == len(got) - 1
    return answers


def test_the_header_keeps_its_window():
    k = vm.header_constants()
    assert k["PG_VAR_SUM_LIMBS"] == 4 and 4 <= k["PG_VAR_SQ_LIMBS"] <= 8 and k["PG_VAR_INT_SLOTS"] == 3 and k["PG_VAR_LONG_EXP"] == 64
    # exact-window inputs (magnitudes within 2^10 of each other, E up to 16 above the largest exponent): s = 25 must fit 2 s <= 32 L2 - 107
    assert 2 * 25 <= 32 * k["PG_VAR_SQ_LIMBS"] - 107


@pytest.mark.parametrize("name", sorted(vm.VECTORS))
def test_tuples_equal_the_fraction_model_bit_for_bit(harness, name):
    data_type, values = vm.VECTORS[name]
    doubles = vm.as_doubles(values, data_type)
    assert data_type in ("INT", "LONG") or vm.in_exact_window(doubles), name
    a = harness[name]
    n, sx, m2 = vm.exact_moments(doubles)
    # the limbs hold the power sums exactly
    assert sum(v << (32 * j) for j, v in enumerate(a["sx"])) * Fraction(2) ** a["q1"] == sx
    assert sum(v << (32 * j) for j, v in enumerate(a["sq"])) * Fraction(2) ** a["q2"] == sum(Fraction(v) ** 2 for v in doubles)
    assert all(v >= 0 for v in a["sq"]) and all(abs(v) < 2**63 for v in a["sx"] + a["sq"])
    want = vm.exact_tuple(doubles)
    assert a["n"] == want[0] == n
    assert vm.same_bits(a["sum"], want[1]), (a["sum"], want[1])
    assert vm.same_bits(a["m2"], want[2]), (a["m2"], want[2])
    assert a["m2"] >= 0.0 and math.copysign(1.0, a["m2"]) == 1.0   # never negative, never -0.0


def test_special_values(harness):
    assert harness["all_equal"]["m2"] == 0.0 and harness["n1"]["m2"] == 0.0 and harness["n2"]["m2"] == 0.5
    assert harness["subnormals"]["m2"] == 0.0 and harness["subnormals"]["sum"] > 0.0
    assert 0.0 < harness["tiny_m2"]["m2"] < 2.0**-1022   # a subnormal result, rounded once


def test_wide_range_stays_within_the_documented_bound(harness):
    data_type, values = vm.WIDE_RANGE
    doubles = vm.as_doubles(values, data_type)
    assert not vm.in_exact_window(doubles)
    a = harness["wide_range"]
    k = vm.header_constants()
    E = _exponent(data_type, doubles, k)
    assert (a["q1"], a["q2"]) == vm.scales(E, k)
    n, sx, m2 = vm.exact_moments(doubles)
    bound = vm.truncation_bound(n, E, k)
    assert abs(Fraction(a["m2"]) - m2) <= bound + vm.ulp(a["m2"]) / 2
    assert abs(Fraction(a["sum"]) - sx) <= n * Fraction(2) ** a["q1"] + vm.ulp(a["sum"]) / 2
    # the limbs themselves: truncation toward zero, below the scale per value
    got_sq = sum(v << (32 * j) for j, v in enumerate(a["sq"])) * Fraction(2) ** a["q2"]
    true_sq = sum(Fraction(v) ** 2 for v in doubles)
    assert 0 <= true_sq - got_sq < n * Fraction(2) ** a["q2"]


def test_the_512_bit_helper(harness):
    for (op, a, b), got in zip(U512, harness["u512"]):
        if op == "mul":
            want = "%0128x" % ((a * b) & ALL_ONES)
        elif op == "sub":
            want = "%0128x" % ((a - b) & ALL_ONES)
        elif op == "cmp":
            want = "%d" % ((a > b) - (a < b))
        elif op == "shl":
            want = "%0128x" % ((a << b) & ALL_ONES)
        elif op == "mulu":
            want = "%0128x" % ((a * b) & ALL_ONES)
        else:
            want = "%0128x %d" % (a // b, a % b)
        assert got == want, (op, hex(a), b)
