"""The expression parser (pinot_amd/csrc/pg_expr.cpp) as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer:
tests/expr_parse_main.cpp parses well-formed texts nested to the limits and malformed ones, checks every status and every reference of the
programs, and would trip the sanitizers on a read out of bounds.  g++ builds the project's host tools already: a missing compiler fails the test.  (The library loaded into Python is not run under a sanitizer.)"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_parser_under_sanitizers(tmp_path):
    exe = str(tmp_path / "expr_parse_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",   # the runtimes linked in: the program runs in the environment as it is
                           os.path.join(ROOT, "tests", "expr_parse_main.cpp"), os.path.join(ROOT, "pinot_amd", "csrc", "pg_expr.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert "expr parse ok" in out.stdout and "FAIL" not in out.stdout
    for what in ("a 16th operation (nested)", "a 9th column", "an unterminated quote", "an empty argument", "a very long identifier",
                 "unbalanced: no closing parenthesis", "15 operations through the second argument"):
        assert "ok   " + what in out.stdout, what
