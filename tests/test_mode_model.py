"""tests/mode_model.py pinned: the scenarios of ModeAggregationFunctionTest (tests/golden/mode_expected.json: data only), the three
extractFinalResult loops against the defined rules wherever the reference's answer does not depend on its iteration order, and a brute-force
collections.Counter cross-check on seeded inputs with forced ties."""
import collections
import decimal
import json
import math
import os
import random

import numpy as np
import pytest

from tests import mode_model as mm

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mode_expected.json")))


def _java(v: float) -> str:
    """Double.toString for the values the scenarios print"""
    if v == -math.inf:
        return "-Infinity"
    if abs(v) < 1e7:
        return repr(v)
    sign, digits, exponent = decimal.Decimal(repr(v)).normalize().as_tuple()   # the shortest digits that round-trip, as Java prints them
    body = "".join(map(str, digits))
    return ("-" if sign else "") + body[0] + "." + (body[1:] or "0") + "E%d" % (exponent + len(body) - 1)


@pytest.mark.parametrize("data_type", ["INT", "LONG", "FLOAT", "DOUBLE"])
def test_the_reference_scenarios(data_type):
    """without null handling a null row holds the column's default null value, which wins 4 : 2 on two instances; the all-null table too"""
    default = float(GOLDEN["default_null_value"][data_type])
    cast = (lambda v: int(v)) if data_type in ("INT", "LONG") else float
    rows = [cast(default) if r is None else cast(r) for r in GOLDEN["rows"]]
    one = mm.value_map(rows, data_type)
    merged = one
    for _ in range(GOLDEN["instances"] - 1):
        merged = mm.merge(merged, mm.value_map(rows, data_type))
    assert dict((float(k), c) for k, c in merged[1]) == {default: 4, 1.0: 2}
    for reducer in mm.REDUCERS:
        assert _java(mm.final(merged, reducer)) == GOLDEN["without_null_handling"][data_type]
    all_null = mm.merge(mm.value_map([cast(default)] * 3, data_type), mm.value_map([cast(default)] * 3, data_type))
    assert _java(mm.final(all_null)) == GOLDEN["all_null_without_null_handling"][data_type]
    # with null handling the nulls are skipped (out of the GPU path's scope: refused there): the map holds 1 alone
    skipped = mm.value_map([cast(r) for r in GOLDEN["rows"] if r is not None], data_type)
    assert _java(mm.final(mm.merge(skipped, skipped))) == GOLDEN["with_null_handling"][data_type]
    assert mm.value_map([], data_type) == ("INT", ()) and mm.final(mm.value_map([], data_type)) == -math.inf   # the empty map's default
    if data_type == "INT":
        g = GOLDEN["group_by"]
        for key, want in g["without_null_handling_INT"].items():
            vals = [cast(default) if v is None else v for v, k in g["rows"] if k == key]
            m = mm.merge(mm.value_map(vals, "INT"), mm.value_map(vals, "INT"))
            assert _java(mm.final(m)) == want


def test_argument_rules():
    assert mm.parse_arguments("x") == ("x", "MIN") and mm.parse_arguments(" x , 'AVG' ") == ("x", "AVG")
    for text, message in (("x,'MIN','MAX'", "Mode expects at most 2 arguments, got: 3"), ("x,'max'", "No enum constant " + mm.ENUM + ".max")):
        with pytest.raises(ValueError) as e:
            mm.parse_arguments(text)
        assert str(e.value) == message


def test_merge_rules():
    a, b = mm.value_map([1, 1, 2], "INT"), mm.value_map([2, 3], "INT")
    assert mm.merge(a, b) == ("INT", ((1, 2), (2, 2), (3, 1))) and mm.merge(("INT", ()), b) is b and mm.merge(a, ("INT", ())) is a
    with pytest.raises(ValueError) as e:
        mm.merge(a, mm.value_map([2.0], "DOUBLE"))
    assert str(e.value) == "Illegal data type for Intermediate Result of MODE aggregation function: Int2LongOpenHashMap, Double2LongOpenHashMap"


@pytest.mark.parametrize("data_type", ["INT", "LONG", "FLOAT", "DOUBLE"])
def test_counter_cross_check_and_the_reference_loops(data_type):
    """seeded inputs with forced ties; tied values have exactly representable sums (integers below 2^53, dyadic fractions), so the
    reference's running sum is exact and its three loops, in ANY iteration order, give the defined values bit for bit"""
    rng = random.Random(5)
    pool = {"INT": [-7, -1, 0, 3, 4, 100, 2**31 - 1, -2**31], "LONG": [-5, 0, 9, 2**40, 2**52, -2**52, 12345],
            "FLOAT": [0.5, 0.25, -1.75, 8.0, 1024.0, -0.125, 3.0], "DOUBLE": [0.5, 0.25, -1.75, 2.0**40, 2.0**-20, -3.0, 7.0, math.inf]}[data_type]
    for trial in range(200):
        ties = rng.randint(1, 4)
        top = rng.randint(1, 6)
        chosen = rng.sample(pool, min(len(pool), rng.randint(ties, len(pool))))
        values = []
        for i, v in enumerate(chosen):
            values += [v] * (top if i < ties else rng.randint(1, max(1, top - 1)) if top > 1 else 0)
        if not values:
            continue
        rng.shuffle(values)
        m = mm.value_map(values, data_type)
        counter = collections.Counter(values)
        assert dict(m[1]) == dict(counter) and [mm.compare_key(k) for k, _ in m[1]] == sorted(mm.compare_key(k) for k in counter)
        best = max(counter.values())
        tied = sorted(k for k, c in counter.items() if c == best)
        assert mm.final(m, "MIN") == float(tied[0]) and mm.final(m, "MAX") == float(tied[-1])
        assert mm.order_free(m)
        for reducer in mm.REDUCERS:
            for _ in range(3):
                order = list(m[1])
                rng.shuffle(order)
                if reducer == "AVG" and math.inf in tied:
                    continue
                assert mm.same_double(mm.reference_final(order, reducer), mm.final(m, reducer)), (values, reducer)


def test_the_defined_rules():
    nan_tie = mm.value_map([math.nan, math.nan, 1.0, 1.0, 0.5], "DOUBLE")
    assert not mm.order_free(nan_tie) and mm.final(nan_tie, "MIN") == 1.0 and math.isnan(mm.final(nan_tie, "MAX")) and math.isnan(mm.final(nan_tie, "AVG"))
    zeros = mm.value_map([0.0, -0.0, 3.0], "DOUBLE")
    assert not mm.order_free(zeros) and math.copysign(1, mm.final(zeros, "MIN")) == -1 and mm.final(zeros, "MAX") == 3.0
    assert mm.order_free(mm.value_map([math.nan, 1.0, 1.0], "DOUBLE"))   # a NaN that is not tied
    inexact = mm.value_map([0.1, 0.2, 0.3], "DOUBLE")                    # the exact sum is no double: one rounding, then one division
    assert mm.final(inexact, "AVG") == 0.6 / 3 and mm.final(inexact, "AVG") != (0.1 + 0.2 + 0.3) / 3
    assert mm.final(mm.value_map([2**53 + 1, 5], "LONG"), "MAX") == float(2**53 + 1) and dict(mm.value_map([2**53 + 1], "LONG")[1]) == {2**53 + 1: 1}
    for m in (nan_tie, zeros, inexact, mm.value_map([1, 2, 2], "INT"), mm.value_map([1.5], "FLOAT"), mm.value_map([], "LONG")):
        kind, body = mm.serialize(m)
        assert mm.same_map(mm.deserialize(kind, body), m)
    assert mm.serialize(mm.value_map([], "DOUBLE")) == (23, b"\0\0\0\0") and mm.serialize(mm.value_map([1.5, 1.5], "FLOAT")) == (25, b"\0\0\0\1\x3f\xc0\0\0" + b"\0" * 7 + b"\2")


def test_the_partial_and_its_combine():
    assert mm.partial_of_row([0, 0]) is None and mm.partial_of_row([0, 3, 1, 3]) == (3, 2, 1, 3) and mm.partial_of_row([2], 7) == (2, 1, 7, 7)
    assert mm.combine(None, None) is None and mm.combine((3, 1, 0, 0), (3, 2, 5, 9)) == (3, 3, 0, 9) and mm.combine((4, 1, 8, 8), (3, 2, 5, 9)) == (4, 1, 8, 8)
