"""tests/time_transform_model.py pinned: to the reference's DateTruncTransformFunctionTest expectations
(tests/golden/time_transform_expected.json), to Python's datetime for the calendar floors, and to the semantics of Java longs for the
truncating families and the saturating conversions."""
import datetime
import json
import os
import random

import pytest

from tests import time_transform_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "time_transform_expected.json")))
EPOCH = datetime.datetime(1970, 1, 1)
UNITS = ["second", "minute", "hour", "day", "week", "month", "quarter", "year"]


@pytest.mark.parametrize("case", GOLDEN["cases"], ids=lambda c: c["tz"])
def test_date_trunc_golden(case):
    assert sorted(case["expected"]) == sorted(UNITS)
    for unit, want in case["expected"].items():
        for text in ("datetrunc('%s',ts,'MILLISECONDS','%s')" % (unit, case["tz"]), "datetrunc('%s',ts,'milliseconds','%s','MILLISECONDS')" % (unit.upper(), case["tz"])):
            assert tm.evaluate(text, [case["input"]]) == [want], text
        if case["tz"] == "UTC":
            assert tm.evaluate("datetrunc('%s',ts)" % unit, [case["input"]]) == [want]
            # ... in seconds in and out, and seconds in, milliseconds out
            assert tm.evaluate("datetrunc('%s',ts,'SECONDS')" % unit, [case["input"] // 1000]) == [want // 1000]
            assert tm.evaluate("datetrunc('%s',ts,'SECONDS','UTC','MILLISECONDS')" % unit, [case["input"] // 1000]) == [want]


def _floor_by_datetime(ms, unit, offset_ms):
    """the same floor through datetime's own calendar (years 1 .. 9999)"""
    local = EPOCH + datetime.timedelta(milliseconds=ms + offset_ms)
    if unit == "week":
        d = local - datetime.timedelta(days=local.weekday())          # Monday
        f = datetime.datetime(d.year, d.month, d.day)
    elif unit == "month":
        f = datetime.datetime(local.year, local.month, 1)
    elif unit == "quarter":
        f = datetime.datetime(local.year, (local.month - 1) // 3 * 3 + 1, 1)
    elif unit == "year":
        f = datetime.datetime(local.year, 1, 1)
    else:
        f = {"day": local.replace(hour=0, minute=0, second=0, microsecond=0), "hour": local.replace(minute=0, second=0, microsecond=0),
             "minute": local.replace(second=0, microsecond=0), "second": local.replace(microsecond=0)}[unit]
    return (f - EPOCH) // datetime.timedelta(milliseconds=1) - offset_ms


def _instants():
    rng = random.Random(20011)
    lo = (datetime.datetime(1600, 1, 1) - EPOCH) // datetime.timedelta(milliseconds=1)
    hi = (datetime.datetime(2400, 1, 1) - EPOCH) // datetime.timedelta(milliseconds=1)
    out = [rng.randrange(lo, hi) for _ in range(400)]
    # leap days and the days around them, year / quarter / week boundaries, on either side of the epoch
    for y in (1600, 1700, 1899, 1900, 1904, 1969, 1970, 1972, 1999, 2000, 2001, 2004, 2100, 2399):
        for m, d in ((1, 1), (2, 28), (3, 1), (4, 1), (6, 30), (7, 1), (10, 1), (12, 31)):
            t = (datetime.datetime(y, m, d) - EPOCH) // datetime.timedelta(milliseconds=1)
            out += [t - 1, t, t + 1, t + tm.DAY_MS - 1, t + tm.DAY_MS]
        if tm.is_leap(y):
            t = (datetime.datetime(y, 2, 29) - EPOCH) // datetime.timedelta(milliseconds=1)
            out += [t - 1, t, t + tm.DAY_MS - 1, t + tm.DAY_MS]
    out += [0, -1, 1, 4 * tm.DAY_MS, 4 * tm.DAY_MS - 1, -3 * tm.DAY_MS, -3 * tm.DAY_MS - 1]
    return [t for t in out if lo <= t < hi]


@pytest.mark.parametrize("tz,offset", [("UTC", 0), ("+07:09", 25_740_000), ("-03:30", -12_600_000)])
def test_calendar_floors_equal_datetime(tz, offset):
    assert tm.zone_offset(tz) == offset
    xs = _instants()
    assert min(xs) < 0 < max(xs)
    for unit in UNITS:
        got = tm.evaluate("datetrunc('%s',ts,'MILLISECONDS','%s')" % (unit, tz), xs)
        for x, g in zip(xs, got):
            assert g == _floor_by_datetime(x, unit, offset), (unit, tz, x)
            assert g <= x
    assert tm.civil(0) == (1970, 1, 1) and tm.civil(-1) == (1969, 12, 31) and tm.civil(11016) == (2000, 2, 29)
    assert EPOCH.weekday() == 3                                         # a Thursday


def test_truncating_families_at_negative_inputs():
    ev = lambda text, x: tm.evaluate(text, [x])[0]   # noqa: E731
    assert ev("toepochdays(ts)", -1) == 0 and ev("toepochdays(ts)", -tm.DAY_MS) == -1 and ev("toepochdays(ts)", -tm.DAY_MS - 1) == -1
    assert ev("datetrunc('day',ts,'MILLISECONDS','UTC','DAYS')", -1) == -1   # ... where the floor says -1
    assert ev("toepochhours(ts)", -3_599_999) == 0 and ev("toepochseconds(ts)", -1999) == -1
    assert ev("toepochminutesrounded(ts,'5')", -7 * 60_000) == -5 and ev("toepochminutesbucket(ts,'5')", -7 * 60_000) == -1
    assert ev("toepochminutesrounded(ts,'-5')", 7 * 60_000) == 5 and ev("toepochminutesbucket(ts,'-5')", 7 * 60_000) == -1
    assert ev("timeconvert(ts,'MILLISECONDS','DAYS')", -1) == 0 and ev("timeconvert(ts,'SECONDS','HOURS')", -7199) == -1
    assert ev("datetimeconvert(ts,'1:MILLISECONDS:EPOCH','1:MILLISECONDS:EPOCH','15:MINUTES')", -1) == 0
    assert ev("datetimeconvert(ts,'1:MILLISECONDS:EPOCH','1:MILLISECONDS:EPOCH','15:MINUTES')", -900_001) == -900_000
    assert ev("datetimeconvert(ts,'1:SECONDS:EPOCH','5:MINUTES:EPOCH','1:DAYS')", 3 * 86400 + 77) == 3 * 288
    assert ev("toepochdaysbucket(ts,'-1')", tm.MIN) == tm.conv(tm.MIN, "MILLISECONDS", "DAYS") * -1
    assert tm.jdiv(tm.MIN, -1) == tm.MIN and tm.jdiv(-7, 2) == -3 and tm.jdiv(7, -2) == -3 and tm.wrap(tm.MAX + 1) == tm.MIN


def test_saturation_of_scale_up_conversions():
    ev = lambda text, x: tm.evaluate(text, [x])[0]   # noqa: E731
    for text, m in (("timeconvert(ts,'SECONDS','MILLISECONDS')", 1000), ("timeconvert(ts,'DAYS','NANOSECONDS')", 86_400 * 10 ** 9),
                    ("timeconvert(ts,'MINUTES','SECONDS')", 60)):
        assert ev(text, 1 << 62) == tm.MAX and ev(text, -(1 << 62)) == tm.MIN
        edge = tm.MAX // m
        assert ev(text, edge) == edge * m and ev(text, edge + 1) == tm.MAX
        assert ev(text, -edge) == -edge * m and ev(text, -edge - 1) == tm.MIN
    # datetrunc and datetimeconvert convert to milliseconds first: seconds at 2^62 saturate, and the bucket runs on Long.MAX_VALUE
    assert ev("datetimeconvert(ts,'1:SECONDS:EPOCH','1:MILLISECONDS:EPOCH','1:SECONDS')", 1 << 62) == tm.MAX // 1000 * 1000
    assert ev("datetimeconvert(ts,'1:SECONDS:EPOCH','1:MILLISECONDS:EPOCH','1:SECONDS')", -(1 << 62)) == tm.MIN // 1000 * 1000 + 1000
    # ... and the input size multiplies with wrap-around before anything saturates
    assert ev("datetimeconvert(ts,'4:MILLISECONDS:EPOCH','1:MILLISECONDS:EPOCH','1:MILLISECONDS')", 1 << 62) == 0
