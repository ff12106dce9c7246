"""pinot_amd/csrc/pg_mode.h — the argument-list parser, the selection's combine rule (the single statement the kernels of
pg_kernels_mode.hip use) and AVG's exact sum — as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer:
tests/mode_main.cpp parses every well-formed and malformed text, combines random rows over random chunkings and sums lists of doubles, which
must equal tests/mode_model.py's.  (The library loaded into Python is not run under a sanitizer.)"""
import math
import os
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from pinot_amd import capi
from tests import mode_model as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WELL_FORMED = ["x", " x ", "x,'MIN'", "x , 'MAX'", "x,'AVG'", "col.umn,'AVG'", "add(a,b)", "add(a,b),'MAX'", "*"]
MALFORMED = [   # (text, message): the reference's texts where it has one
    ("x,'MIN','MAX'", "Mode expects at most 2 arguments, got: 3"), ("x,y,z,w", "Mode expects at most 2 arguments, got: 4"),
    ("x,'avg'", "No enum constant " + mm.ENUM + ".avg"), ("x,'Min'", "No enum constant " + mm.ENUM + ".Min"), ("x,'MEDIAN'", "No enum constant " + mm.ENUM + ".MEDIAN"),
    ("x,''", "No enum constant " + mm.ENUM + "."), ("x,MAX", "quoted MultiModeReducerType"), ("x,y", "quoted MultiModeReducerType"),
    ("'x'", "the first argument must be a column"), ("x,'MAX", "unterminated quote"), ("x,", "empty argument"), (",'MAX'", "empty argument"),
    ("", "empty argument list"), ("   ", "empty argument list"), ("add(a,b,'MAX'", "unbalanced parentheses"), ("x),'MAX'", "unbalanced parentheses"),
    ("x 'MAX'", "text next to a quoted literal"), ("x,'MAX'y", "text next to a quoted literal"),
]


def _bits(v):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", v))[0]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mode") / "mode_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",   # the runtimes linked in: the program runs in the environment as it is
                           os.path.join(ROOT, "tests", "mode_main.cpp"), "-o", exe])

    def run(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
        got = out.stdout.splitlines()
        assert got[-1] == "mode ok" and len(got) == len(lines) + 1
        return got[:-1]
    return run


def test_well_formed_and_malformed_texts(harness):
    got = harness(["P " + t for t in WELL_FORMED] + ["P " + t for t, _ in MALFORMED])
    for text, line in zip(WELL_FORMED, got):
        column, reducer = mm.parse_arguments(text)
        assert line == "ok %d x=%s" % (mm.REDUCERS.index(reducer), column), (text, line)
    for (text, message), line in zip(MALFORMED, got[len(WELL_FORMED):]):
        assert line.startswith("err %d " % capi.PG_ERR_INVALID_ARGUMENT) and message in line, (text, line)
        with pytest.raises(ValueError) as e:
            mm.parse_arguments(text)
        if message[0].isupper():   # the reference's texts are the model's
            assert str(e.value) == line.split(" ", 2)[2], text


def _rows(rng):
    """random rows with forced ties, a single-id row, all-zero rows, ties that straddle every chunk border"""
    rows = [[0], [5], [0, 0, 0, 0], [3, 3], [3, 3, 3, 3, 3], [1, 2, 3, 3, 2, 1], [0, 7, 0, 7, 0, 7, 0], [2] * 130, [0] * 64 + [1] + [0] * 64 + [1]]
    for _ in range(120):
        n = int(rng.integers(1, 200))
        r = rng.integers(0, int(rng.integers(1, 6)), n)   # few distinct counts: many ties
        if rng.integers(0, 3) == 0:
            r[rng.integers(0, n, 3)] = 9                 # up to three ids tied at the top, anywhere
        rows.append([int(c) for c in r])
    return rows


def test_any_chunking_gives_the_whole_rows_partial(harness):
    rng = np.random.default_rng(7)
    lines, wants = [], []
    for row in _rows(rng):
        whole = mm.partial_of_row(row)
        chunkings = [[], list(range(1, len(row))), [len(row) // 2], [0, 0, len(row)]] + [sorted(int(c) for c in rng.integers(0, len(row) + 1, int(rng.integers(1, 9)))) for _ in range(4)]
        for cuts in chunkings:
            lines.append("C " + " ".join(map(str, cuts)) + " | " + " ".join(map(str, row)))
            wants.append("none" if whole is None else "%d %d %d %d" % whole)
            # the model's own combine over the same chunks agrees with the definition
            p, at = None, 0
            for cut in cuts + [len(row)]:
                p = mm.combine(p, mm.partial_of_row(row[at:cut], at) if cut > at else None)
                at = max(at, cut)
            assert p == whole
    assert harness(lines) == wants


def test_the_exact_sum_is_rounded_once(harness):
    rng = np.random.default_rng(11)
    lists = [[0.1, 0.2, 0.3], [0.5, 0.25], [1e308, 1e308, -1e308], [1e308, 1e308], [-1e308, -1e308, -1e308], [2.0**53, 1.0, 1.0], [2.0**53, 1.0, -1.0, 1.0],
             [1.0, 2.0**-53, 2.0**-53], [1.0, 2.0**-53], [1.0, 2.0**-53, 2.0**-1074], [5e-324, 5e-324, -5e-324], [5e-324] * 3, [2.2250738585072014e-308, -5e-324],
             [0.0, -0.0], [-0.0, -0.0], [1.0, -1.0], [math.inf, 1.0], [-math.inf, 1e308], [math.inf, -math.inf], [math.nan, 1.0], [3.0], [],
             [float(i) for i in range(1, 200)], [0.1] * 10, [1e16, 1.0, -1e16], [1.7976931348623157e308, 9.9e291], [1.7976931348623157e308, 9.979201547673598e291, 1e200]]
    for _ in range(150):
        n = int(rng.integers(1, 40))
        lists.append([float(math.ldexp(rng.uniform(-1, 1), int(rng.integers(-1074, 1023)))) for _ in range(n)])
        lists.append([float(rng.integers(-2**53, 2**53)) * 2.0 ** int(rng.integers(-60, 60)) for _ in range(n)])
    got = harness(["S " + " ".join(_bits(v) for v in l) for l in lists])
    for l, line in zip(lists, got):
        if any(v != v for v in l) or (math.inf in l and -math.inf in l):
            want = math.nan
        elif math.inf in l or -math.inf in l:
            want = math.inf if math.inf in l else -math.inf
        else:
            exact = sum((Fraction(v) for v in l), Fraction(0))
            try:
                want = float(exact)
            except OverflowError:
                want = math.inf if exact > 0 else -math.inf
        have = struct.unpack("<d", struct.pack("<Q", int(line, 16)))[0]
        assert (want != want and have != have) or have == want, (l[:6], have, want)   # (an exact zero sum is +0.0)
