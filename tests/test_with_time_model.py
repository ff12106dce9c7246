"""tests/with_time_model.py against what the reference's FIRSTWITHTIME / LASTWITHTIME classes state: the tie rule of their docId-order loops
(`>=` / `<=`: the greatest docId among the docs at the extreme time, for FIRST and LAST alike), the DEFAULT_VALUE_TIME_PAIR constants of the
eight classes, the Java primitive conversions of a declared type over another stored type, `merge` with its ties, and the bindings' own
with_time_merge."""
import itertools
import struct

import numpy as np
import pytest

from pinot_amd.executor import extract_final, merge_intermediate, with_time_merge
from tests import with_time_model as wm


@pytest.mark.parametrize("function", wm.FUNCTIONS)
def test_equal_times_give_the_greatest_doc(function):
    times = [5] * 9
    assert wm.winner(function, times, range(9)) == 8
    assert wm.winner(function, times, [1, 4, 6]) == 6          # ... among the MATCHING docs
    assert wm.winner(function, times, []) is None
    times = [3, 9, 1, 9, 1, 4]
    assert wm.winner("LASTWITHTIME", times, range(6)) == 3     # the later of the two docs at time 9
    assert wm.winner("FIRSTWITHTIME", times, range(6)) == 4    # the later of the two docs at time 1
    assert wm.winner("LASTWITHTIME", times, [0, 1, 2]) == 1 and wm.winner("FIRSTWITHTIME", times, [0, 1, 2]) == 2


def test_extreme_times_are_ordinary_values():
    times = [wm.LONG_MIN, 0, wm.LONG_MAX, wm.LONG_MIN, wm.LONG_MAX, -1]
    assert wm.winner("LASTWITHTIME", times, range(6)) == 4 and wm.winner("FIRSTWITHTIME", times, range(6)) == 3
    # a doc AT the default time replaces the default pair (>= / <=)
    assert wm.aggregate("LASTWITHTIME", "INT", [7], [wm.LONG_MIN], [0], "INT") == (7, wm.LONG_MIN)
    assert wm.aggregate("FIRSTWITHTIME", "INT", [7], [wm.LONG_MAX], [0], "INT") == (7, wm.LONG_MAX)


def test_default_pairs():
    """Last{Int,Long,Float,Double}ValueWithTime...: (Integer.MIN_VALUE | Long.MIN_VALUE | Float.NaN | Double.NaN, Long.MIN_VALUE); First...:
    the same values with Long.MAX_VALUE"""
    want = {"INT": -2147483648, "LONG": -9223372036854775808, "FLOAT": 0x7FC00000, "DOUBLE": 0x7FF8000000000000}
    for declared, value in want.items():
        assert wm.default_pair("LASTWITHTIME", declared) == (value, -9223372036854775808)
        assert wm.default_pair("FIRSTWITHTIME", declared) == (value, 9223372036854775807)
        assert wm.aggregate("LASTWITHTIME", "DOUBLE", [], [], [], declared) == wm.default_pair("LASTWITHTIME", declared)
    assert struct.unpack("<f", struct.pack("<I", 0x7FC00000))[0] != struct.unpack("<f", struct.pack("<I", 0x7FC00000))[0]   # a NaN


def test_java_primitive_conversions():
    assert wm.convert("DOUBLE", np.float64(2.0**31), "INT") == 2147483647              # (int) saturates
    assert wm.convert("DOUBLE", np.float64(-2.0**31 - 5), "INT") == -2147483648
    assert wm.convert("DOUBLE", np.float64("nan"), "INT") == 0 and wm.convert("DOUBLE", np.float64("nan"), "LONG") == 0
    assert wm.convert("FLOAT", np.float32("nan"), "INT") == 0 and wm.convert("FLOAT", np.float32("inf"), "LONG") == wm.LONG_MAX
    assert wm.convert("DOUBLE", np.float64(2.0**63), "LONG") == wm.LONG_MAX and wm.convert("DOUBLE", np.float64(-1e300), "LONG") == wm.LONG_MIN
    assert wm.convert("DOUBLE", np.float64(-7.9), "INT") == -7 and wm.convert("DOUBLE", np.float64(7.9), "LONG") == 7   # toward zero
    assert wm.convert("LONG", 2**40 + 5, "INT") == 5                                   # (int) of a long keeps the low 32 bits
    assert wm.convert("LONG", 2**31, "INT") == -2147483648 and wm.convert("LONG", -1, "INT") == -1
    assert wm.convert("DOUBLE", np.float64(0.1), "FLOAT") == 0x3DCCCCCD                # (float) rounds once: 0.1f
    assert wm.convert("FLOAT", wm.bits_f32(0x3DCCCCCD), "DOUBLE") == 0x3FB99999A0000000   # a float widens exactly
    assert wm.convert("LONG", 2**53 + 1, "DOUBLE") == wm.f64_bits(2.0**53) and wm.convert("LONG", 2**24 + 1, "FLOAT") == 0x4B800000   # nearest-even
    assert wm.convert("INT", -5, "LONG") == -5 and wm.convert("INT", -5, "DOUBLE") == wm.f64_bits(-5.0)
    # its own type: the bits as they are (NaN payloads, -0.0)
    assert wm.convert("FLOAT", wm.bits_f32(0x7FC12345), "FLOAT") == 0x7FC12345 and wm.convert("FLOAT", wm.bits_f32(0x80000000), "FLOAT") == 0x80000000
    assert wm.convert("DOUBLE", wm.bits_f64(0x7FF8000000ABCDEF), "DOUBLE") == 0x7FF8000000ABCDEF
    assert wm.convert("DOUBLE", wm.bits_f64(0x8000000000000000), "DOUBLE") == 0x8000000000000000


@pytest.mark.parametrize("function", wm.FUNCTIONS)
def test_merge_is_associative_and_the_first_argument_wins_ties(function):
    pairs = [(1, 10), (2, 10), (3, -4), (4, 99), (5, 99), (6, wm.LONG_MIN), (7, wm.LONG_MAX), wm.default_pair(function, "INT")]
    for a, b, c in itertools.product(pairs, repeat=3):
        assert wm.merge(function, wm.merge(function, a, b), c) == wm.merge(function, a, wm.merge(function, b, c))
    assert wm.merge(function, (1, 10), (2, 10)) == (1, 10) and wm.merge(function, (2, 10), (1, 10)) == (2, 10)
    later, earlier = (4, 99), (3, -4)
    assert wm.merge(function, later, earlier) == wm.merge(function, earlier, later) == (later if function == "LASTWITHTIME" else earlier)
    for a, b in itertools.product(pairs, repeat=2):   # the bindings restate the same merge
        assert with_time_merge(function, a, b) == wm.merge(function, a, b) == merge_intermediate(function, a, b)
    assert extract_final(function, (42, 7)) == 42


def test_merging_segments_in_order_equals_one_pass():
    """pairs of consecutive doc ranges merged left to right, later segment as the FIRST argument of a tie, give the one-pass winner"""
    rng = np.random.default_rng(5)
    times = rng.integers(0, 6, 300)
    values = rng.integers(-1000, 1000, 300)
    for function in wm.FUNCTIONS:
        whole = wm.aggregate(function, "INT", values, times, range(300), "INT")
        acc = wm.default_pair(function, "INT")
        for lo in range(0, 300, 50):
            acc = wm.merge(function, wm.aggregate(function, "INT", values, times, range(lo, lo + 50), "INT"), acc)
        assert acc == whole


def test_to_bytes_and_order_keys():
    assert wm.to_bytes((-2, 3), "INT") == bytes.fromhex("fffffffe" "0000000000000003") and wm.OBJECT_TYPE == {"INT": 27, "LONG": 28, "FLOAT": 29, "DOUBLE": 30}
    assert wm.to_bytes((0x3DCCCCCD, -1), "FLOAT") == bytes.fromhex("3dcccccd" "ffffffffffffffff")
    assert wm.to_bytes((-2, 3), "LONG") == bytes.fromhex("fffffffffffffffe" "0000000000000003") and len(wm.to_bytes((0, 0), "DOUBLE")) == 16
    ts = [wm.LONG_MIN, -1, 0, wm.LONG_MAX]
    assert [wm.order_key(t, False) for t in ts] == [0, 2**63 - 1, 2**63, 2**64 - 1]
    assert [wm.order_key(t, True) for t in ts] == [2**64 - 1, 2**63, 2**63 - 1, 0]
    assert wm.doc_bits(1) == 1 and wm.doc_bits(2) == 1 and wm.doc_bits(3) == 2 and wm.doc_bits(2**31 - 1) == 31 and wm.doc_bits(10**6) == 20
    assert wm.packed_ok(2**44 - 2, 20) and not wm.packed_ok(2**44 - 1, 20)
