"""The query splitter of the side passes (pinot_amd/csrc/pg_side_query.cpp) as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/side_query_main.cpp splits queries with side aggregations first, in the middle, last, everywhere and
nowhere, with every kind of ORDER BY, with and without agg_params and under both paths' flag sets, and checks base_index, the kept
specs, params, order and flags field by field; and asks pg::side_tier — where a slot-table path keeps its table — at both sides of every
boundary.  (The library loaded into Python is not run under a sanitizer.)"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_splitter_under_sanitizers(tmp_path):
    exe = str(tmp_path / "side_query_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",   # the runtimes linked in: the program runs in the environment as it is
                           os.path.join(ROOT, "tests", "side_query_main.cpp"), os.path.join(ROOT, "pinot_amd", "csrc", "pg_side_query.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert "side query ok" in out.stdout and "FAIL" not in out.stdout
    for what in ("no side aggregation: nothing left out", "every aggregation a side one: COUNT(*) is inserted",
                 "a side aggregation first: the ORDER BY index shifts by 1", "side aggregations first and in the middle: the ORDER BY index shifts by 2",
                 "a side aggregation last: no shift", "ORDER BY a side aggregation: ORDER BY is dropped, LIMIT stays",
                 "ORDER BY a key column and an aggregation mixed", "ORDER BY aggregation -1: invalid argument", "ORDER BY aggregation n: invalid argument",
                 "agg_params null: the ordinary part's is null", "agg_params given: the kept aggregations' params",
                 "the percentile path's flags: FINAL_PERCENTILE and KEEP_DEVICE_TABLE cleared",
                 "the expression path: a PERCENTILE stays with its param and FINAL_PERCENTILE, KEEP_DEVICE_TABLE is cleared"):
        assert "ok   " + what in out.stdout, what
    # the tier choice: REG 0, LDS 1, HBM 2, refused -1
    for what, tier in (("no GROUP BY, one slot", 0), ("no GROUP BY, more slots than any limit", 0), ("GROUP BY, one slot", 1),
                       ("slots == LDS ceiling", 1), ("slots == LDS ceiling + 1", 2), ("a lowered LDS knob: slots == knob", 1),
                       ("a lowered LDS knob: slots == knob + 1", 2), ("bytes == HBM limit", 2), ("bytes == HBM limit + 8", -1),
                       ("double width: bytes == HBM limit at half the slots", 2), ("double width: refused at half the slots + 1", -1),
                       ("double width below the LDS ceiling: the slot count decides", 1), ("an HBM limit below the LDS ceiling: LDS is asked first", 1)):
        assert f"ok   tier: {what}: {tier} (want {tier})" in out.stdout, what
