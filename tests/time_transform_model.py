"""The time-bucket transforms of DESIGN 4.9 restated in plain Python integers, independently of the library's normal form: timeconvert,
toepoch{seconds,minutes,hours,days}[rounded|bucket], datetimeconvert (EPOCH to EPOCH) and datetrunc (UTC or a fixed offset), as the reference's
TimeConversionTransformFunction, DateTimeFunctions, EpochToEpochTransformer and DateTruncTransformFunction compute them over Java longs.

evaluate(text, values) takes the canonical text ExpressionContext#toString prints and a sequence of ints; columns_of(text) names the value
column.  Only texts the GPU path accepts are modelled (tests spell the refusals out themselves)."""
import re

MAX, MIN = (1 << 63) - 1, -(1 << 63)
NANOS = {"NANOSECONDS": 1, "MICROSECONDS": 10 ** 3, "MILLISECONDS": 10 ** 6, "SECONDS": 10 ** 9, "MINUTES": 60 * 10 ** 9, "HOURS": 3600 * 10 ** 9,
         "DAYS": 86400 * 10 ** 9}
DAY_MS = 86_400_000
WIDTH_MS = {"millisecond": 1, "second": 1000, "minute": 60_000, "hour": 3_600_000, "day": DAY_MS, "week": 7 * DAY_MS}


def wrap(x):
    """a Java long: two's complement wrap-around"""
    return (x - MIN) % (1 << 64) + MIN


def jdiv(a, b):
    """Java's a / b on longs: truncation toward zero; Long.MIN_VALUE / -1 is Long.MIN_VALUE"""
    q = abs(a) // abs(b)
    return wrap(q if (a < 0) == (b < 0) else -q)


def conv(d, frm, to):
    """java.util.concurrent.TimeUnit#convert(d, frm) on the unit `to`"""
    a, b = NANOS[frm], NANOS[to]
    if a == b:
        return d
    if a > b:
        m = a // b
        if d > MAX // m:
            return MAX
        if d < -(MAX // m):
            return MIN
        return d * m
    return jdiv(d, b // a)


def _leaps_through(y):
    return y // 4 - y // 100 + y // 400


def days_before_year(y):
    """days from 1970-01-01 to January 1st of the proleptic Gregorian year y"""
    return 365 * (y - 1970) + _leaps_through(y - 1) - _leaps_through(1969)


def is_leap(y):
    return y % 4 == 0 and (y % 100 != 0 or y % 400 == 0)


def civil(day):
    """(year, month, day of month) of the day number `day` (days since 1970-01-01), proleptic Gregorian"""
    y = 1970 + day * 400 // 146097
    while days_before_year(y) > day:
        y -= 1
    while days_before_year(y + 1) <= day:
        y += 1
    rest = day - days_before_year(y)
    lengths = [31, 29 if is_leap(y) else 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31]
    m = 0
    while rest >= lengths[m]:
        rest -= lengths[m]
        m += 1
    return y, m + 1, rest + 1


def day_number(y, m):
    """the day number of the first of month m of year y"""
    lengths = [31, 29 if is_leap(y) else 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31]
    return days_before_year(y) + sum(lengths[:m - 1])


def round_floor(ms, unit, offset=0):
    """ISOChronology's field.roundFloor in a zone of fixed offset: floor the local instant, go back"""
    local = ms + offset
    if unit in WIDTH_MS:
        w = WIDTH_MS[unit]
        phase = 4 * DAY_MS if unit == "week" else 0     # 1970-01-05 is a Monday
        return wrap((local - phase) // w * w + phase - offset)
    y, m, _ = civil(local // DAY_MS)
    if unit == "quarter":
        m = (m - 1) // 3 * 3 + 1
    elif unit == "year":
        m = 1
    elif unit != "month":
        raise ValueError(unit)
    return wrap(day_number(y, m) * DAY_MS - offset)


def zone_offset(tz):
    if tz.upper() == "UTC":
        return 0
    m = re.fullmatch(r"([+-])(\d\d):(\d\d)", tz)
    if not m:
        raise ValueError(tz)
    return (1 if m.group(1) == "+" else -1) * (int(m.group(2)) * 60 + int(m.group(3))) * 60_000


def _format(f):
    """(size, unit) of an EPOCH DateTimeFormatSpec"""
    if f[0].isdigit():
        size, unit, kind = f.split(":")
    else:
        tok = f.split("|")
        kind, unit, size = tok[0], (tok[1] if len(tok) > 1 else "MILLISECONDS"), (tok[2] if len(tok) > 2 else "1")
    if kind != "EPOCH":
        raise ValueError(f)
    return int(size), unit


def arguments(text):
    """(canonical function name, [arguments with their quotes dropped]) of fn(arg,...) whose arguments are columns or quoted literals"""
    m = re.fullmatch(r"\s*([A-Za-z_]+)\((.*)\)\s*", text)
    name = m.group(1).lower().replace("_", "")
    args = [a if q == "" else q[1:-1] for q, a in re.findall(r"\s*(?:('[^']*')|([^,'\s]+))\s*(?:,|$)", m.group(2))]
    return name, args


def columns_of(text):
    name, args = arguments(text)
    return [args[1] if name == "datetrunc" else args[0]]


def function_of(text):
    """the transform as a function int -> int"""
    name, a = arguments(text)
    if name == "timeconvert":
        return lambda x: conv(x, a[1].upper(), a[2].upper())
    m = re.fullmatch(r"toepoch(seconds|minutes|hours|days)(rounded|bucket)?", name)
    if m:
        unit, n = m.group(1).upper(), (int(a[1]) if m.group(2) else None)
        if m.group(2) == "rounded":
            return lambda x: wrap(jdiv(conv(x, "MILLISECONDS", unit), n) * n)
        if m.group(2) == "bucket":
            return lambda x: jdiv(conv(x, "MILLISECONDS", unit), n)
        return lambda x: conv(x, "MILLISECONDS", unit)
    if name == "datetimeconvert":
        (in_size, in_unit), (out_size, out_unit) = _format(a[1]), _format(a[2])
        g_size, g_unit = a[3].split(":") if a[3][0].isdigit() else (a[3].split("|") + ["1"])[1::-1]
        gran = conv(int(g_size), g_unit, "MILLISECONDS")

        def f(x):
            ms = conv(wrap(x * in_size), in_unit, "MILLISECONDS")
            g = wrap(jdiv(ms, gran) * gran)
            return jdiv(conv(g, "MILLISECONDS", out_unit), out_size)
        return f
    if name == "datetrunc":
        unit = a[0].lower()
        in_unit = a[2].upper() if len(a) > 2 else "MILLISECONDS"
        offset = zone_offset(a[3]) if len(a) > 3 else 0
        out_unit = a[4].upper() if len(a) > 4 else in_unit
        return lambda x: conv(round_floor(conv(x, in_unit, "MILLISECONDS"), unit, offset), "MILLISECONDS", out_unit)
    raise ValueError(text)


# ISOChronology's year range (Joda-Time): beyond it dateTrunc's roundFloor throws in the reference, and the GPU path's value is unspecified
JODA_MIN_YEAR, JODA_MAX_YEAR = -292275054, 292278993


def defined(text, x):
    """does the reference define the transform's value at x?  (everywhere, but for datetrunc outside Joda's year range: one year is kept clear
    of either end, where a floor could leave the range)"""
    name, a = arguments(text)
    if name != "datetrunc":
        return True
    ms = conv(int(x), a[2].upper() if len(a) > 2 else "MILLISECONDS", "MILLISECONDS") + (zone_offset(a[3]) if len(a) > 3 else 0)
    return days_before_year(JODA_MIN_YEAR + 1) * DAY_MS <= ms < days_before_year(JODA_MAX_YEAR) * DAY_MS and MIN <= ms <= MAX


def evaluate(text, values):
    f = function_of(text)
    return [f(int(v)) for v in values]
