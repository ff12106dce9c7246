"""pinot_amd/csrc/pg_histogram.h — the argument-list parser, the bin specification and pg_hist_bin, the single statement of getBinId the
kernels of pg_kernels_hist.hip use — as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer: tests/histogram_main.cpp
parses every well-formed and malformed text and bins a list of values, which must equal tests/histogram_model.py's.  (The library loaded
into Python is not run under a sanitizer.)"""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

from pinot_amd import capi
from tests import histogram_model as hm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGES_1001 = ",".join(f"'{i * 0.37 - 100}'" for i in range(1001))
WELL_FORMED = [
    "x,'0','1000','10'", " x , '0' ,'1000', '10' ", "x,'0','1','3'", "x,'0','1','7'", "x,'-999.5','500.5','15'", "x,'0','1','1'", "x,'1e-3','1e3','65'",
    "x,'0','100','65536'", "x,'0','100','65537'", "x,'-1e308','1e308','4'", "x,'-Infinity','5','2'", "x,'0','Infinity','2'",
    "x,arrayvalueconstructor('0','1')", "x,arrayvalueconstructor('0','0.1','1')", "x,arrayvalueconstructor(-Infinity,'0','0.1',Infinity)",
    "col.umn,arrayvalueconstructor( -Infinity , '-999','-800','-500','500','600','800', Infinity )", "x,arrayvalueconstructor('0.5','1.5','2.5','3.5','4.5','5.5')",
    "x,arrayvalueconstructor(%s)" % EDGES_1001, "add(a,b),'0','2000','20'", "x,'0','9007199254740992','2'",
]
MALFORMED = [   # (text, message): the reference's texts
    ("x", "Histogram expects 2 or 4 arguments, got: 1;"), ("x,'0','1'", "Histogram expects 2 or 4 arguments, got: 3;"),
    ("x,'0','1','2','3'", "Histogram expects 2 or 4 arguments, got: 5;"),
    ("x,'5'", "Please use the format of `Histogram(columnName, ARRAY[1,10,100])` to specify the bin edges"),
    ("x,y", "Please use the format of `Histogram(columnName, ARRAY[1,10,100])` to specify the bin edges"),
    ("x,arrayconstructor('0','1')", "Please use the format of `Histogram(columnName, ARRAY[1,10,100])` to specify the bin edges"),
    ("x,arrayvalueconstructor('0')", "The number of bin edges must be greater than 1"), ("x,arrayvalueconstructor()", "The number of bin edges must be greater than 1"),
    ("x,arrayvalueconstructor('0','0','1','2')", "The bin edges must be strictly increasing"), ("x,arrayvalueconstructor('1','0')", "The bin edges must be strictly increasing"),
    ("x,arrayvalueconstructor('0',NaN)", "The bin edges must be strictly increasing"),
    ("x,'1000','1000','10'", "The right most edge must be greater than left most edge, given 1000.0 and 1000.0"),
    ("x,'2.5','-1','10'", "The right most edge must be greater than left most edge, given 2.5 and -1.0"),
    ("x,'0','1000','-1'", "The number of bins must be greater than zero, given -1"), ("x,'0','1000','0'", "The number of bins must be greater than zero, given 0"),
    ("x,'a','1','3'", 'For input string: "a"'), ("x,'0','b','3'", 'For input string: "b"'), ("x,'0','1','3.5'", 'For input string: "3.5"'),
    ("x,arrayvalueconstructor('0','one')", 'For input string: "one"'),
    ("x,'0','1','3", "unterminated quote"), ("x,,'1','3'", "empty argument"), ("", "empty argument list"), ("x,arrayvalueconstructor('0','1'", "unbalanced parentheses"),
    ("'x','0','1','3'", "the first argument must be a column"),
]


def _bits(v):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", v))[0]


def _values(spec):
    """every edge and one ulp to either side of it, the zeros, the infinities, a NaN, 2^53 + 1 as a LONG, 0.1f, the two rounding cases"""
    edges = spec.edges if spec.kind == "edges" else [spec.lower + i * spec.bin_length for i in range(min(spec.n_bins, 2000))] + [spec.upper]
    out = []
    for e in edges:
        out += [e] + ([math.nextafter(e, -math.inf), math.nextafter(e, math.inf)] if math.isfinite(e) else [])
    out += [0.0, -0.0, math.inf, -math.inf, math.nan, hm.as_doubles([2**53 + 1], "LONG")[0], hm.as_doubles([0.1], "FLOAT")[0], 0.1, 0.9999999999999999,
            0.5, 1.0, -1.0, 1e300, -1e300, 5e-324]
    return out


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("histogram") / "histogram_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",   # the runtimes linked in: the program runs in the environment as it is
                           os.path.join(ROOT, "tests", "histogram_main.cpp"), "-o", exe])

    def run(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
        got = out.stdout.splitlines()
        assert got[-1] == "histogram ok" and len(got) == len(lines) + 1
        return got[:-1]
    return run


def test_well_formed_texts_and_bins(harness):
    lines, specs = [], []
    for text in WELL_FORMED:
        x, spec = hm.parse_arguments(text)
        specs.append((x, spec, _values(spec)))
        lines += ["P " + text, "S", "B " + " ".join(_bits(v) for v in specs[-1][2])]
    got = harness(lines)
    for k, (text, (x, spec, values)) in enumerate(zip(WELL_FORMED, specs)):
        parsed, supported, bins = got[3 * k:3 * k + 3]
        f = parsed.split()
        assert f[0] == "ok" and int(f[1]) == (0 if spec.kind == "equal" else 1) and int(f[2]) == spec.n_bins, (text, parsed)
        assert f[3:5] == [_bits(spec.lower), _bits(spec.upper)] and f[6] == "x=" + x
        if spec.kind == "equal":
            assert f[5] == _bits(spec.bin_length) and len(f) == 7      # (upper - lower) / numBins, rounded as the model rounds it
        else:
            assert f[7:] == [_bits(e) for e in spec.edges]
        ok = spec.n_bins <= hm.MAX_BINS and (spec.kind == "edges" or (math.isfinite(spec.lower) and math.isfinite(spec.upper)))
        assert supported.startswith("supported" if ok else "unsupported"), (text, supported)
        assert [int(b) for b in bins.split()] == [hm.bin_of(spec, v) for v in values], text
    assert hm.header_constants()["PG_HIST_MAX_BINS"] == hm.MAX_BINS and hm.header_constants()["PG_HIST_MAX_SPECS"] == hm.MAX_SPECS


def test_the_rounding_cases_and_the_values_the_issue_names(harness):
    x = 0.9999999999999999
    got = harness(["P x,'0','1','3'", "B " + " ".join(_bits(v) for v in (x, math.nan, 1.0, 0.0, -0.0)), "P x,'0','1','7'", "B " + _bits(x),
                   "P x,arrayvalueconstructor('0','0.1','1')", "B " + " ".join(_bits(v) for v in (float(np.float32(0.1)), 0.1, math.nan, math.inf, -math.inf)),
                   "P x,arrayvalueconstructor(-Infinity,'0',Infinity)", "B " + " ".join(_bits(v) for v in (-math.inf, math.inf, -0.0, math.nan))])
    assert got[1] == "-3 -2 2 0 0" and got[3] == "-3"
    assert got[5] == "1 1 -2 -1 -1" and got[7] == "0 1 1 -2"


def test_malformed_texts(harness):
    got = harness(["P " + text for text, _ in MALFORMED])
    for (text, message), line in zip(MALFORMED, got):
        assert line.startswith("err %d " % capi.PG_ERR_INVALID_ARGUMENT) and message in line, (text, line)
        if message[0].isupper() and not message.endswith(";"):   # the reference's texts are the model's
            with pytest.raises(ValueError) as e:
                hm.parse_arguments(text)
            assert str(e.value) == line.split(" ", 2)[2], text
