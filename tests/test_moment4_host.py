"""The exact power sums of pinot_amd/csrc/pg_moment4.h — the digits the kernels of pg_kernels_moment.hip add, the wide integer and the one
rounding per double of the host — as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer: tests/moment4_main.cpp
reads vectors from stdin and prints limbs and result bits, which must equal tests/fourth_moment_model.py's Fraction model bit for bit wherever
the windows hold every digit, and stay within the documented bounds where they do not.  (The library loaded into Python is not run under a
sanitizer.)"""
import math
import os
import random
import struct
import subprocess
from fractions import Fraction

import pytest

from tests import fourth_moment_model as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = fm.header_constants()
BITS = 32 * K["PG_WIDE_WORDS"]
HEX = BITS // 4
ALL_ONES = (1 << BITS) - 1
WIDE = [   # (op, a, b): carry and borrow chains through every limb
    ("mul", (1 << (BITS // 2)) - 1, (1 << (BITS // 2)) - 1), ("mul", ALL_ONES, ALL_ONES), ("mul", ALL_ONES, 1), ("mul", (1 << (BITS - 1)) | 1, 2), ("mul", 0, ALL_ONES),
    ("mul", int("f" * 40, 16), int("f" * 79, 16)), ("add", ALL_ONES, 1), ("add", ALL_ONES, ALL_ONES), ("add", (1 << 600) - 1, 1), ("add", 0, 0),
    ("sub", 1 << (BITS - 1), 1), ("sub", 0, 1), ("sub", ALL_ONES, ALL_ONES), ("sub", 1 << 640, (1 << 639) + 1),
    ("cmp", 1 << (BITS - 1), (1 << (BITS - 1)) - 1), ("cmp", 5, 5), ("cmp", 4, 1 << 32),
    ("shl", ALL_ONES, 0), ("shl", ALL_ONES, 1), ("shl", ALL_ONES, 31), ("shl", ALL_ONES, 32), ("shl", ALL_ONES, 63), ("shl", ALL_ONES, 160), ("shl", ALL_ONES, BITS - 1),
    ("shl", 1, BITS - 1),
    ("mulu", ALL_ONES, 0xFFFFFFFF), ("mulu", (1 << 796) - 1, 0x7FFFFFFF), ("mulu", 12345, 0),
    ("div", ALL_ONES, 1), ("div", ALL_ONES, 0xFFFFFFFF), ("div", ALL_ONES, 0x7FFFFFFF), ("div", (1 << 796) - 1, 3), ("div", 7, 9), ("div", 1 << (BITS - 1), 0x80000001),
]
random.seed(13)
WIDE += [(op, random.getrandbits(random.randint(1, BITS)), random.getrandbits(random.randint(1, BITS))) for op in ("mul", "add", "sub", "cmp") for _ in range(40)]
WIDE += [("shl", random.getrandbits(random.randint(1, BITS)), random.randint(0, BITS - 1)) for _ in range(40)]
WIDE += [(op, random.getrandbits(random.randint(1, BITS)), random.randint(1, 2**32 - 1)) for op in ("mulu", "div") for _ in range(40)]


def _bits(v: float) -> str:
    return "%016x" % struct.unpack("<Q", struct.pack("<d", v))[0]


def _from_bits(h: str) -> float:
    return struct.unpack("<d", struct.pack("<Q", int(h, 16)))[0]


def _exponent(data_type, doubles):
    return K["PG_VAR_LONG_EXP"] if data_type == "LONG" else fm.fx_exp_of(max((abs(v) for v in doubles), default=0.0))


def _value(limbs, q):
    return sum(v << (32 * j) for j, v in enumerate(limbs)) * Fraction(2) ** q


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("moment4")
    exe = str(d / "moment4_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",   # the runtimes linked in: the program runs in the environment as it is
                           os.path.join(ROOT, "tests", "moment4_main.cpp"), "-o", exe])
    names = sorted(fm.VECTORS) + ["wide_range"]
    lines = ["K"]
    for name in names:
        data_type, values = fm.VECTORS[name] if name != "wide_range" else fm.WIDE_RANGE
        if data_type == "INT":
            lines.append("I %d %s" % (len(values), " ".join(str(int(v)) for v in values)))
        else:
            doubles = fm.as_doubles(values, data_type)
            lines.append("D %d %d %s" % (_exponent(data_type, doubles), len(doubles), " ".join(_bits(v) for v in doubles)))
    for op, a, b in WIDE:
        lines.append("U %s %x %s" % (op, a, "%x" % b if op in ("mul", "add", "sub", "cmp") else "%d" % b))
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    got = out.stdout.splitlines()
    assert got[-1] == "moment4 ok"
    assert got[0] == "K %d %d %d %d %d %d %d %d" % (fm.limbs(K) + (K["PG_M4_INT_SLOTS"], K["PG_VAR_LONG_EXP"], K["PG_WIDE_WORDS"], K["PG_WIDE_GUARD"]))
    answers, pos = {}, 1
    for name in names:
        q, limbs, r = got[pos].split(), got[pos + 1], got[pos + 2].split()
        assert q[0] == "Q" and limbs.startswith("L ") and r[0] == "R"
        answers[name] = {"q": [int(x) for x in q[1:5]], "s": [[int(x) for x in part.split()] for part in limbs[2:].split("|")], "n": int(r[1]),
                         "m": [_from_bits(x) for x in r[2:6]]}
        pos += 3
    answers["wide"] = [line[2:] for line in got[pos:pos + len(WIDE)]]
    assert pos + len(WIDE) == len(got) - 1
    return answers


def test_the_header_keeps_its_windows():
    L1, L2, L3, L4 = fm.limbs(K)
    assert (L1, L2) == (4, 6) and K["PG_VAR_LONG_EXP"] == 64
    # the rule of pg_moment4.h, k (s + 53) <= 32 L_k - 1, at the window L2 = 6 keeps (s = 42): the smallest lengths that hold it
    s = (32 * L2 - 1) // 2 - 53
    assert s == 42
    assert L3 == -(-(3 * (s + 53) + 1) // 32) == 9 and L4 == -(-(4 * (s + 53) + 1) // 32) == 12
    assert K["PG_M4_DBL_SLOTS"] == 31 and K["PG_M4_INT_SLOTS"] == 1 + 2 + 3 + 4
    # a LONG column: every scale is negative, integers have no digit below 2^0
    assert all(q < 0 for q in fm.scales(64, K))
    # the wide integer: 14 n^4 2^(4E) on the scale 4 q1, shifted up by the guard bits, n < 2^31
    need = (14 * 2 ** 124 * 2 ** (32 * 4 * L1 - 4)).bit_length() + K["PG_WIDE_GUARD"]
    assert need <= 32 * K["PG_WIDE_WORDS"] and K["PG_WIDE_GUARD"] - 93 >= 55


@pytest.mark.parametrize("name", sorted(fm.VECTORS))
def test_tuples_equal_the_fraction_model_bit_for_bit(harness, name):
    data_type, values = fm.VECTORS[name]
    doubles = fm.as_doubles(values, data_type)
    assert data_type in ("INT", "LONG") or fm.in_exact_window(doubles), name
    a = harness[name]
    sums = fm.power_sums(doubles)
    # the limbs hold the power sums exactly
    for k in range(4):
        assert _value(a["s"][k], a["q"][k]) == sums[k + 1], (name, k)
        assert all(abs(v) < 2**63 for v in a["s"][k])
    assert all(v >= 0 for v in a["s"][1] + a["s"][3])
    want = fm.exact_tuple(doubles)
    got = (a["n"],) + tuple(a["m"])
    assert fm.same_tuple(got, want), (got, want)
    assert a["m"][1] >= 0.0 and math.copysign(1.0, a["m"][1]) == 1.0 and a["m"][3] >= 0.0 and math.copysign(1.0, a["m"][3]) == 1.0   # never negative, never -0.0
    assert a["m"][2] != 0.0 or math.copysign(1.0, a["m"][2]) == 1.0   # an exact zero m3 is +0.0


def test_special_values(harness):
    assert harness["all_equal"]["m"][1:] == [0.0, 0.0, 0.0]
    assert harness["n1"]["m"] == [3.5, 0.0, 0.0, 0.0] and harness["n2"]["m"] == [2.0, 0.5, 0.0, 0.125]
    assert harness["n3"]["n"] == 3 and harness["n4"]["n"] == 4 and harness["n4"]["m"][2] != 0.0
    assert harness["symmetric"]["m"][2] == 0.0 and harness["symmetric"]["m"][3] > 0.0
    assert harness["negative_skew"]["m"][2] < 0.0 and harness["alternating"]["m"][0] != 0.0
    assert harness["subnormals"]["m"][1:] == [0.0, 0.0, 0.0] and harness["subnormals"]["m"][0] > 0.0
    assert 0.0 < harness["tiny_m4"]["m"][3] < 2.0**-1022   # a subnormal result, rounded once


def test_wide_range_stays_within_the_documented_bounds(harness):
    data_type, values = fm.WIDE_RANGE
    doubles = fm.as_doubles(values, data_type)
    assert not fm.in_exact_window(doubles)
    a = harness["wide_range"]
    E = _exponent(data_type, doubles)
    assert tuple(a["q"]) == fm.scales(E, K)
    exact = fm.exact_moments(doubles)
    n = exact[0]
    bounds = fm.truncation_bounds(n, E, K)
    for k in range(4):
        assert abs(Fraction(a["m"][k]) - exact[k + 1]) <= bounds[k] + fm.ulp(a["m"][k]) / 2, k
    # the limbs themselves: truncation toward zero, below the scale per value
    sums = fm.power_sums(doubles)
    for k in range(4):
        got = _value(a["s"][k], a["q"][k])
        assert abs(sums[k + 1] - got) < n * Fraction(2) ** a["q"][k], k
    assert sums[4] - _value(a["s"][3], a["q"][3]) > 0   # something was truncated: the bound is exercised


def test_the_wide_integer(harness):
    fmt = "%0" + str(HEX) + "x"
    for (op, a, b), got in zip(WIDE, harness["wide"]):
        if op == "mul":
            want = fmt % ((a * b) & ALL_ONES)
        elif op == "add":
            want = fmt % ((a + b) & ALL_ONES)
        elif op == "sub":
            want = fmt % ((a - b) & ALL_ONES)
        elif op == "cmp":
            want = "%d" % ((a > b) - (a < b))
        elif op == "shl":
            want = fmt % ((a << b) & ALL_ONES)
        elif op == "mulu":
            want = fmt % ((a * b) & ALL_ONES)
        else:
            want = (fmt + " %d") % (a // b, a % b)
        assert got == want, (op, hex(a), b)
