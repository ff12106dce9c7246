"""pinot_amd/csrc/pg_with_time.h — the order keys, the packed bound and the pack / unpack of FIRSTWITHTIME / LASTWITHTIME, shared by the
kernels of pg_kernels_withtime.hip and the executor — as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer:
tests/with_time_main.cpp reads cases from stdin, and every answer must equal tests/with_time_model.py's Python integers.  (The library
loaded into Python is not run under a sanitizer.)"""
import os
import subprocess

import pytest

from tests import with_time_model as wm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = 2**64 - 1
DOC_COUNTS = [1, 2, 3, 4, 5, 64, 65, 2049, 10**6, 2**20, 2**20 + 1, 2**30, 2**30 + 1, 2**31 - 1]
TIMES = [wm.LONG_MIN, wm.LONG_MIN + 1, -2**31, -1, 0, 1, 2**31 - 1, 1_700_000_000_000, wm.LONG_MAX - 1, wm.LONG_MAX]


def _ranges(d):
    """(tmin, tmax) from both sides of the packed bound beside `d` doc bits, at several places of the long line"""
    bound = wm.packed_max_range(d)
    out = []
    for rng in (0, 1, bound - 1, bound, bound + 1, M64):
        for tmin in (wm.LONG_MIN, -5, 0, wm.LONG_MAX - rng):
            if wm.LONG_MIN <= tmin and tmin + rng <= wm.LONG_MAX:
                out.append((tmin, tmin + rng))
    return out


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    d = tmp_path_factory.mktemp("with_time")
    exe = str(d / "with_time_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",   # the runtimes linked in: the program runs in the environment as it is
                           os.path.join(ROOT, "tests", "with_time_main.cpp"), "-o", exe])

    def go(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
        got = out.stdout.splitlines()
        assert got[-1] == "with_time ok" and len(got) == len(lines) + 1
        return got[:-1]
    return go


def test_constants_and_doc_bits(run):
    k = wm.header_constants()
    got = run(["K"] + ["D %d" % n for n in DOC_COUNTS])
    assert got[0] == "K %d %d %d" % (k["PG_WT_MAX_SLOTS"], k["PG_WT_MAX_AGGS"], k["PG_WT_LDS_SLOTS"])
    assert (k["PG_WT_MAX_SLOTS"], k["PG_WT_MAX_AGGS"], k["PG_WT_LDS_SLOTS"]) == (4, 8, 16384)
    assert got[1:] == ["D %d" % wm.doc_bits(n) for n in DOC_COUNTS]
    assert wm.doc_bits(1) == 1 and wm.doc_bits(2**31 - 1) == 31


def test_order_keys(run):
    cases = [(t, first) for t in TIMES for first in (0, 1)]
    got = run(["O %d %d" % c for c in cases])
    assert got == ["O %016x %d" % (wm.order_key(t, bool(first)), t) for t, first in cases]
    for first in (False, True):   # the key orders the times: ascending for LAST, descending for FIRST
        keys = [wm.order_key(t, first) for t in TIMES]
        assert keys == sorted(keys, reverse=first) and len(set(keys)) == len(keys)
    assert wm.order_key(wm.LONG_MIN, False) == 0 == wm.order_key(wm.LONG_MAX, True)
    assert wm.order_key(wm.LONG_MAX, False) == M64 == wm.order_key(wm.LONG_MIN, True)


@pytest.mark.parametrize("d", [1, 2, 20, 30, 31])
def test_eligibility_from_both_sides_of_the_bound(run, d):
    cases = _ranges(d)
    got = run(["E %d %d %d" % (lo, hi, d) for lo, hi in cases])
    assert got == ["E %016x %016x %d" % (hi - lo, wm.packed_max_range(d), wm.packed_ok(hi - lo, d)) for lo, hi in cases]
    bound = wm.packed_max_range(d)
    assert wm.packed_ok(bound, d) and not wm.packed_ok(bound + 1, d)
    assert wm.pack(bound, 2**d - 1, d) == M64 and wm.pack(bound + 1, 0, d) > M64   # the largest admitted rel fills the word exactly; one more overflows
    assert any(g.endswith(" 1") for g in got) and any(g.endswith(" 0") for g in got)


@pytest.mark.parametrize("d", [1, 20, 31])
def test_pack_round_trips(run, d):
    cases = []
    for lo, hi in _ranges(d):
        if not wm.packed_ok(hi - lo, d):
            continue
        for t in {lo, hi, lo + (hi - lo) // 2}:          # rel = 0 and the largest admitted rel, for both directions
            for doc in {0, 1, 2**d - 1, 2**(d - 1)}:
                for first in (0, 1):
                    cases.append((lo, hi, t, doc, d, first))
    got = run(["P %d %d %d %d %d %d" % c for c in cases])
    want = []
    for lo, hi, t, doc, d_, first in cases:
        rel = hi - t if first else t - lo
        v = wm.pack(rel, doc, d)
        assert 0 < v <= M64
        want.append("P %016x %d %016x %d" % (v, doc, rel, t))
    assert got == want
    # the packed order is the order of (time, doc): later time wins for LAST, earlier for FIRST, the greater doc among equal times
    lo, hi = 100, 100 + min(wm.packed_max_range(d), 1000)
    docs = sorted({0, 1, 2**d - 1})
    for first in (False, True):
        items = [(t, doc) for t in (lo, lo + 1, hi) for doc in docs]
        best = max(items, key=lambda it: wm.pack(hi - it[0] if first else it[0] - lo, it[1], d))
        assert best == ((lo if first else hi), docs[-1])
