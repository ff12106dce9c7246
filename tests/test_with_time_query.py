"""FIRSTWITHTIME / LASTWITHTIME from SQL to the C ABI: every spelling parses to the two canonical names (AggregationFunctionType strips
underscores and ignores case), CQuery fills the function ids 21 / 22 and the argument list "x,t,'TYPE'", the header and the bindings agree on
the new constants, the ABI version, the query struct and the export list are unchanged, the argument lexer splits the lists and refuses
malformed ones (tests/with_time_args_main.cpp over pg_expr.cpp, under the sanitizers), and a record with the two functions passes through the
shim's C half (tests/shim_with_time_records.c against integration/jni/pinot_gpu_shim.c)."""
import os
import subprocess

import pytest

from pinot_amd import capi
from pinot_amd.query import CQuery, SqlError, parse_sql, with_time_arguments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPELLINGS = {
    "FIRSTWITHTIME": ["FIRSTWITHTIME", "FIRST_WITH_TIME", "firstwithtime", "firstWithTime", "First_With_Time", "FIRSTWITH_TIME"],
    "LASTWITHTIME": ["LASTWITHTIME", "LAST_WITH_TIME", "lastwithtime", "lastWithTime", "Last_With_Time", "LAST_WITHTIME"],
}
IDS = {"FIRSTWITHTIME": 21, "LASTWITHTIME": 22}
INVALID = capi.PG_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("function,spelling", [(f, s) for f, ss in SPELLINGS.items() for s in ss])
def test_every_spelling_parses(function, spelling):
    qc = parse_sql(f"SELECT {spelling}(x, ts, 'DOUBLE') FROM t")
    assert [(a.function, a.column) for a in qc.aggregations] == [(function, "x,ts,'DOUBLE'")]
    qc = parse_sql(f"SELECT g, COUNT(*), {spelling}( lat ,ts, 'int' ) AS v FROM t WHERE s < 5 GROUP BY g ORDER BY {spelling}(lat, ts, 'int') DESC LIMIT 3")
    assert [(a.function, a.column) for a in qc.aggregations] == [("COUNT", None), (function, "lat,ts,'int'")]   # the literal as given: the column's name keeps it
    assert qc.resolved_order_by() == [(capi.ORDER_BY_AGGREGATION, 1, False)]   # any spelling names the same aggregation
    cq = CQuery(qc)
    assert cq.query.n_aggregations == 2 and cq.query.aggregations[1].function == IDS[function] and cq.query.aggregations[1].column == b"lat,ts,'int'"
    assert not cq.query.agg_params   # the functions take no parameter
    assert with_time_arguments(qc.aggregations[1].column) == ("lat", "ts", "INT")


def test_function_ids_next_to_the_other_side_aggregations():
    qc = parse_sql("SELECT LASTWITHTIME(a, ts, 'LONG'), FIRST_WITH_TIME(b, ts, 'FLOAT'), VAR_POP(a), PERCENTILE(a, 95), SUM(a * b), COUNT(*) FROM t GROUP BY g")
    cq = CQuery(qc)
    assert [cq.query.aggregations[i].function for i in range(6)] == [22, 21, 17, 16, 1, 0]
    assert cq.query.aggregations[0].column == b"a,ts,'LONG'" and cq.query.aggregations[1].column == b"b,ts,'FLOAT'"
    assert cq.query.agg_params[3] == 95.0 and cq.query.agg_params[0] == 0.0
    # an ORDER BY over another spelling, another case of the literal and other blanks names the same aggregation; another column does not
    qc = parse_sql("SELECT g, LASTWITHTIME(a, ts, 'long') FROM t GROUP BY g ORDER BY last_with_time( a,ts,'LONG' )")
    assert qc.resolved_order_by() == [(capi.ORDER_BY_AGGREGATION, 0, True)]
    assert parse_sql("SELECT g, LASTWITHTIME(a, ts, 'long') FROM t GROUP BY g ORDER BY LASTWITHTIME(b, ts, 'long')").resolved_order_by() is None
    # an expression argument travels as its canonical text (the library refuses it: "<FN> over an expression")
    qc = parse_sql("SELECT LASTWITHTIME(a + b, ts, 'DOUBLE') FROM t")
    assert qc.aggregations[0].column == "plus(a,b),ts,'DOUBLE'"
    for bad in ("SELECT LASTWITHTIME(a, ts) FROM t", "SELECT LASTWITHTIME(a, ts, INT) FROM t", "SELECT LASTWITHTIME(a, ts, 5) FROM t",
                "SELECT FIRSTWITHTIME(a) FROM t", "SELECT FIRSTWITHTIME(a, ts, 'INT', 'x') FROM t", "SELECT FIRSTWITHTIME(*) FROM t"):
        with pytest.raises(SqlError):
            parse_sql(bad)


def test_header_and_bindings_agree():
    header = open(os.path.join(ROOT, "include", "pinot_gpu.h")).read()
    assert "#define PG_ABI_VERSION 5" in header and capi.PG_ABI_VERSION == 5
    for name, fid in IDS.items():
        assert f"PG_AGG_{name} = {fid}" in header and capi.AGG_FUNCTIONS[name] == fid
    assert capi.WITH_TIME_FUNCTIONS == tuple(IDS) and capi.WITH_TIME_TYPES == ("INT", "LONG", "FLOAT", "DOUBLE")
    assert "PG_RESULT_VALUE_TIME_PAIR = 9" in header and capi.RESULT_VALUE_TIME_PAIR == 9
    assert capi.PgQuery._fields_[-1][0] == "agg_params"   # the query struct is unchanged
    assert [f[0] for f in capi.PgAggSpec._fields_] == ["function", "log2m", "column"]   # ... and the aggregation's: the list travels in `column`
    # no new exported function: the pair is read through pg_result_longs / pg_result_doubles
    exports = open(os.path.join(ROOT, "pinot_amd", "csrc", "libpinot_gpu.map")).read()
    assert "time" not in exports.lower().replace("runtime", "") and "pg_result_longs" in exports and "pg_result_doubles" in exports
    knobs = open(os.path.join(ROOT, "pinot_amd", "csrc", "pg_api.cpp")).read()
    assert '"PG_WT_HBM_MAX_BYTES", (int64_t)256 << 20' in knobs
    java = open(os.path.join(ROOT, "integration", "java", "org", "apache", "pinot", "gpu", "PinotGpu.java")).read()
    assert "RESULT_VALUE_TIME_PAIR = 9" in java


SPLITS = [   # (text, status, arguments: (text, quoted))
    ("x,t,'DOUBLE'", 0, [("x", False), ("t", False), ("DOUBLE", True)]),
    ("  x ,\tt , 'int' ", 0, [("x", False), ("t", False), ("int", True)]),
    ("x,t", 0, [("x", False), ("t", False)]),                                   # the count is the caller's to judge
    ("x,t,INT", 0, [("x", False), ("t", False), ("INT", False)]),               # ... and so is a bare third argument
    ("plus(a,b),t,'INT'", 0, [("plus(a,b)", False), ("t", False), ("INT", True)]),   # commas at depth 0 only
    ("add(a,mult(b,'2')),t,'LONG'", 0, [("add(a,mult(b,'2'))", False), ("t", False), ("LONG", True)]),
    ("x,t,'A,B'", 0, [("x", False), ("t", False), ("A,B", True)]),              # a comma inside a literal
    ("x,t,''", 0, [("x", False), ("t", False), ("", True)]),
    ("", INVALID, []), ("x,,'INT'", INVALID, []), ("x,t,", INVALID, []), (",t,'INT'", INVALID, []),
    ("x,t,'INT", INVALID, []), ("x,t,'INT'x", INVALID, []), ("plus(a,b,t,'INT'", INVALID, []), ("x),t,'INT'", INVALID, []),
    ("f('a,t,'INT'", INVALID, []),
]


def test_the_argument_lexer_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "with_time_args_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",   # the runtimes linked in: the program runs in the environment as it is
                           os.path.join(ROOT, "tests", "with_time_args_main.cpp"), os.path.join(ROOT, "pinot_amd", "csrc", "pg_expr.cpp"), "-o", exe])
    out = subprocess.run([exe], input="".join(text + "\n" for text, _, _ in SPLITS), capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    got = out.stdout.splitlines()
    want = ["%d %d%s" % (st, len(args), "".join((" <%s>" if q else " [%s]") % t for t, q in args)) for _, st, args in SPLITS]
    assert got == want + ["%d null" % INVALID, "split ok"]


def test_with_time_records_through_the_shim(tmp_path):
    if not os.path.exists(capi.GPU_LIB_PATH):
        pytest.skip("libpinot_gpu.so not built here")
    csrc = os.path.join(ROOT, "pinot_amd", "csrc")
    exe = str(tmp_path / "shim_with_time_records")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "integration", "jni"), os.path.join(ROOT, "tests", "shim_with_time_records.c"),
                           os.path.join(ROOT, "integration", "jni", "pinot_gpu_shim.c"), "-L" + csrc, "-lpinot_gpu", "-Wl,-rpath," + csrc, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    for line in ("ids 21 / 22 and their argument lists arrive unchanged", "a truncated record fails cleanly", "the functions take no parameter", "wire format ok"):
        assert line in out.stdout
