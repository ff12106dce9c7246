"""The CASE half of the expression parser (pinot_amd/csrc/pg_expr.cpp) as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/case_parse_main.cpp checks the lowering order, the operation and column limits reached through CASE, every
malformed shape and a host-side run of each accepted program against hand values, and would trip the sanitizers on a read out of bounds.
g++ builds the project's host tools already: a missing compiler fails the test.  (The library loaded into Python is not run under a sanitizer.)"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_case_parser_under_sanitizers(tmp_path):
    exe = str(tmp_path / "case_parse_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",   # the runtimes linked in: the program runs in the environment as it is
                           os.path.join(ROOT, "tests", "case_parse_main.cpp"), os.path.join(ROOT, "pinot_amd", "csrc", "pg_expr.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert "case parse ok" in out.stdout and "FAIL" not in out.stdout
    for what in ("lowering order", "a 16th operation through CASE", "a 9th column in a condition", "an even argument count", "a non-comparison WHEN: a column",
                 "a comparison outside a WHEN: the argument", "an unterminated string literal", "mod inside a WHEN"):
        assert "ok   " + what in out.stdout, what
    assert out.stdout.count("ok   value") == 19      # the host-side runs against hand values
