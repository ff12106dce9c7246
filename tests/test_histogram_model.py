"""tests/histogram_model.py pinned to every array of HistogramQueriesTest (tests/golden/histogram_expected.json): the inner-segment arrays,
the filtered ones, the inter-segment ones as four merged copies; the ADD(intColumn,doubleColumn) argument and the CEIL(DIV(intColumn,400))
key are computed here.  Also the two inputs on which the reference throws."""
import math

import numpy as np
import pytest

from tests import histogram_model as hm

G = hm.golden()
DATA, TYPES = hm.golden_columns(G)


def _values(x):
    if x == "ADD(intColumn,doubleColumn)":
        return [float(a) + float(b) for a, b in zip(DATA["intColumn"], DATA["doubleColumn"])]
    return hm.as_doubles(DATA[x], TYPES[x])


def _match(where):
    i, l = DATA["intColumn"].astype(np.int64), DATA["longColumn"]
    if where is None:
        return np.ones(len(i), dtype=bool)
    if where == "intColumn >= 500":
        return i >= 500
    if where == "intColumn < 0":
        return i < 0
    assert where.startswith("longColumn BETWEEN -1000 AND -950 OR")
    return ((l >= -1000) & (l <= -950)) | ((l >= -900) & (l <= 2)) | ((l >= 900) & (l <= 950))


def _run(x, args, where):
    name, spec = hm.parse_arguments(hm.sql_arguments(x, args))
    assert name == x
    vals = np.asarray(_values(x))[_match(where)]
    return hm.histogram(spec, vals)


@pytest.mark.parametrize("case", G["cases"], ids=lambda c: f"{c['x']}|{c['args']}"[:60])
def test_golden_arrays(case):
    got = _run(case["x"], case["args"], case.get("where"))
    assert got == tuple(float(v) for v in case["expected"])
    if "expected_with_filter" in case:
        assert _run(case["x"], case["args"], G["filter"]) == tuple(float(v) for v in case["expected_with_filter"])
    if "expected_four_segments" in case:
        # (the test's inter-segment query of the Infinity case runs WITHOUT the filter)
        total = got
        for _ in range(3):
            total = hm.merge(total, got)
        assert total == tuple(float(v) for v in case["expected_four_segments"])


def test_golden_group_by():
    gb = G["group_by"]
    _, spec = hm.parse_arguments(hm.sql_arguments(gb["x"], gb["args"]))
    keys = np.ceil(DATA["intColumn"].astype(np.float64) / 400.0)
    vals = np.asarray(_values(gb["x"]))
    assert sorted(set(keys)) == [float(k) for k in sorted(map(int, gb["expected"]))]
    for k, want in gb["expected"].items():
        got = hm.histogram(spec, vals[keys == float(k)])
        assert got == tuple(float(v) for v in want)
        four = hm.merge(hm.merge(got, got), hm.merge(got, got))
        assert four == tuple(float(v) for v in gb["expected_four_segments"][k])


@pytest.mark.parametrize("case", G["invalid"], ids=lambda c: c["args"])
def test_invalid_arguments(case):
    x, _, rest = case["args"].partition(",")
    text = hm.sql_arguments(x, rest) if rest else x
    with pytest.raises(ValueError) as e:
        hm.parse_arguments(text)
    assert str(e.value) == case["reason"]


def test_the_two_throwing_inputs():
    x = 0.9999999999999999
    for bins in (3, 7):
        _, spec = hm.parse_arguments(f"x,'0','1','{bins}'")
        assert math.floor(x / spec.bin_length) == bins          # the index rounds up to numBins
        assert hm.bin_of(spec, x) == hm.THROWS_INDEX
        assert hm.bin_of(spec, 1.0) == bins - 1 and hm.bin_of(spec, math.nextafter(x, 0.0)) == bins - 1
        with pytest.raises(hm.Throws):
            hm.histogram(spec, [0.5, x])
    _, spec = hm.parse_arguments("x,'0','1','4'")               # a power of two never rounds up
    assert hm.bin_of(spec, x) == 3
    for text in ("x,'0','1','3'", "x,arrayvalueconstructor('0','1')", "x,arrayvalueconstructor(-Infinity,'0',Infinity)"):
        _, spec = hm.parse_arguments(text)
        assert hm.bin_of(spec, math.nan) == hm.THROWS_NAN
        with pytest.raises(hm.Throws):
            hm.histogram(spec, [math.nan])


def test_bins_edges_and_infinities():
    _, spec = hm.parse_arguments("x,arrayvalueconstructor(-Infinity,'0','0.1',Infinity)")
    assert [hm.bin_of(spec, v) for v in (-math.inf, -1.0, -0.0, 0.0, math.nextafter(0.1, 0), 0.1, float(np.float32(0.1)), math.inf)] == [0, 0, 1, 1, 1, 2, 2, 2]
    _, spec = hm.parse_arguments("x,arrayvalueconstructor('0','0.1','1')")
    assert [hm.bin_of(spec, v) for v in (-math.inf, math.nextafter(0.0, -1), 1.0, math.nextafter(1.0, 2), math.inf)] == [hm.NONE, hm.NONE, 1, hm.NONE, hm.NONE]
    assert hm.bin_of(spec, hm.as_doubles([0.1], "FLOAT")[0]) == 1      # 0.1f widened lies above the double 0.1
    _, spec = hm.parse_arguments("x,'0','9007199254740992','2'")
    assert hm.as_doubles([2**53 + 1], "LONG")[0] == 2.0**53 and hm.bin_of(spec, hm.as_doubles([2**53 + 1], "LONG")[0]) == 1   # rounds onto upper
    assert hm.merge((1.0, 2.0), (3.0, 4.0)) == (4.0, 6.0)
    with pytest.raises(ValueError):
        hm.merge((1.0,), (1.0, 2.0))
