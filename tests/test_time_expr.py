"""The time-bucket transform parser (pinot_amd/csrc/pg_time_expr.cpp) and the per-value function the key kernel shares with the host
(pg_time_eval, pinot_amd/csrc/pg_time_program.h) as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer:
tests/time_expr_main.cpp parses every text of tests/time_transform_cases.py and evaluates the accepted ones over the committed inputs of
tests/golden/time_transform_inputs.json.  Every value must equal tests/time_transform_model.py's, every refusal carry its status and text, and the
multiply-high reciprocals equal the divisions they replace.  (The library loaded into Python is not run under a sanitizer.)"""
import json
import os
import subprocess

import pytest

from pinot_amd import capi
from tests import time_transform_cases as cases
from tests import time_transform_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUTS = json.load(open(os.path.join(ROOT, "tests", "golden", "time_transform_inputs.json")))["inputs"]


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    d = tmp_path_factory.mktemp("time_expr")
    exe = str(d / "time_expr_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",   # the runtimes linked in: the program runs in the environment as it is
                           os.path.join(ROOT, "tests", "time_expr_main.cpp"), os.path.join(ROOT, "pinot_amd", "csrc", "pg_time_expr.cpp"), "-o", exe])
    texts = [t for t, _ in cases.ACCEPTED] + [s for s, _ in cases.SPELLINGS] + [t for t, _, _ in cases.REFUSED] + cases.NOT_OF_THE_FAMILY
    assert all("\n" not in t for t in texts)
    (d / "texts").write_text("".join(t + "\n" for t in texts))
    (d / "inputs").write_text("".join("%d\n" % v for v in INPUTS))
    out = subprocess.run([exe, str(d / "texts"), str(d / "inputs")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    lines = out.stdout.splitlines()
    assert lines[-1] == "time expr ok" and not any(line.startswith("FAIL") for line in lines)
    got, k = {}, 0
    for t in texts:
        head = lines[k].split(" ", 3)
        assert head[0] == "T", lines[k]
        status, family, rest = int(head[1]), head[2] == "1", head[3] if len(head) > 3 else ""
        k += 1
        values = None
        if status == capi.PG_OK:
            assert lines[k].startswith("V "), lines[k]
            values = [int(v) for v in lines[k].split()[1:]]
            k += 1
        got[t] = (status, family, rest, values)
    assert k == len(lines) - 1
    return got


def test_inputs_cover_the_edges():
    assert {0, -1, tm.MAX, tm.MIN, 1 << 62, -(1 << 62)} <= set(INPUTS) and len(INPUTS) == len(set(INPUTS))
    assert all(tm.MIN <= v <= tm.MAX for v in INPUTS)


@pytest.mark.parametrize("text,column", cases.ACCEPTED)
def test_values_equal_the_model(answers, text, column):
    status, family, rest, values = answers[text]
    assert status == capi.PG_OK and family and rest == column == tm.columns_of(text)[0]
    want = tm.evaluate(text, INPUTS)
    ok = [tm.defined(text, x) for x in INPUTS]       # (datetrunc beyond Joda's year range: the reference throws)
    assert sum(ok) >= len(INPUTS) - 12
    assert [v for v, k in zip(values, ok) if k] == [w for w, k in zip(want, ok) if k], [(x, g, w) for x, g, w, k in zip(INPUTS, values, want, ok) if k and g != w][:5]


@pytest.mark.parametrize("given,canonical", cases.SPELLINGS)
def test_spellings(answers, given, canonical):
    status, family, rest, values = answers[given]
    assert status == capi.PG_OK and family and values == tm.evaluate(canonical, INPUTS)


@pytest.mark.parametrize("text,status,piece", cases.REFUSED)
def test_refusals(answers, text, status, piece):
    got, family, error, values = answers[text]
    assert got == status and family and values is None
    assert error.startswith("time function: ") and piece in error, error


def test_other_functions_are_not_of_the_family(answers):
    for text in cases.NOT_OF_THE_FAMILY:
        status, family, error, _ = answers[text]
        assert not family and status == capi.PG_ERR_INVALID_ARGUMENT and "expected at" in error, text
