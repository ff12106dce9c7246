"""COVAR_POP / COVAR_SAMP from SQL to the C ABI: every spelling parses to the two canonical names (AggregationFunctionType strips
underscores and ignores case), the two arguments travel as the canonical argument list "x,y", CQuery fills the function ids 23 / 24, the
header and the bindings agree on the new constants, the ABI version and the query struct are unchanged, and a record with the two
functions passes through the shim's C half (tests/shim_covariance_records.c against integration/jni/pinot_gpu_shim.c)."""
import os
import subprocess

import pytest

from pinot_amd import capi
from pinot_amd.query import CQuery, SqlError, parse_sql

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPELLINGS = {
    "COVARPOP": ["COVAR_POP", "COVARPOP", "covar_pop", "Covar_Pop", "covarPop"],
    "COVARSAMP": ["COVAR_SAMP", "COVARSAMP", "covar_samp", "covarSamp", "CoVar_Samp"],
}
IDS = {"COVARPOP": 23, "COVARSAMP": 24}


@pytest.mark.parametrize("function,spelling", [(f, s) for f, ss in SPELLINGS.items() for s in ss])
def test_every_spelling_parses(function, spelling):
    qc = parse_sql(f"SELECT {spelling}(x, y) FROM t")
    assert [(a.function, a.column) for a in qc.aggregations] == [(function, "x,y")]
    qc = parse_sql(f"SELECT g, COUNT(*), {spelling}(  lat ,m ) FROM t WHERE s < 5 GROUP BY g ORDER BY {spelling}(lat,  m) DESC LIMIT 3")
    assert [(a.function, a.column) for a in qc.aggregations] == [("COUNT", None), (function, "lat,m")]   # the canonical text: no blank
    assert qc.resolved_order_by() == [(capi.ORDER_BY_AGGREGATION, 1, False)]   # any spelling names the same aggregation
    cq = CQuery(qc)
    assert cq.query.n_aggregations == 2 and cq.query.aggregations[1].function == IDS[function] and cq.query.aggregations[1].column == b"lat,m"
    assert not cq.query.agg_params   # the functions take no parameter


def test_order_by_tells_the_pairs_and_the_functions_apart():
    qc = parse_sql("SELECT g, COVAR_POP(a, b), COVAR_SAMP(a, b), COVAR_POP(b, a) FROM t GROUP BY g ORDER BY covar_pop(b, a), COVARSAMP(a,b) DESC, g")
    assert qc.resolved_order_by() == [(capi.ORDER_BY_AGGREGATION, 2, True), (capi.ORDER_BY_AGGREGATION, 1, False), (capi.ORDER_BY_GROUP_KEY, 0, True)]
    assert parse_sql("SELECT g, COVAR_POP(a, b) FROM t GROUP BY g ORDER BY COVAR_POP(a, c)").resolved_order_by() is None


def test_function_ids_argument_counts_and_an_expression_argument():
    qc = parse_sql("SELECT COVAR_POP(a, b), COVAR_SAMP(a, c), VAR_POP(a), PERCENTILE(a, 95), SUM(a * b) FROM t GROUP BY g")
    cq = CQuery(qc)
    assert [cq.query.aggregations[i].function for i in range(5)] == [23, 24, 17, 16, 1]
    assert [cq.query.aggregations[i].column for i in range(2)] == [b"a,b", b"a,c"]
    assert cq.query.agg_params[3] == 95.0 and cq.query.agg_params[0] == 0.0
    # an expression argument travels as its canonical text (the library refuses it: "<FN> over an expression")
    qc = parse_sql("SELECT COVAR_SAMP(a + b, c) FROM t")
    assert (qc.aggregations[0].function, qc.aggregations[0].column) == ("COVARSAMP", "plus(a,b),c")
    for bad in ("SELECT COVAR_POP(a) FROM t", "SELECT COVAR_POP(a, b, c) FROM t"):
        with pytest.raises(SqlError):
            parse_sql(bad)


def test_header_and_bindings_agree():
    header = open(os.path.join(ROOT, "include", "pinot_gpu.h")).read()
    assert "#define PG_ABI_VERSION 5" in header and capi.PG_ABI_VERSION == 5
    for name, fid in IDS.items():
        assert f"PG_AGG_{name} = {fid}" in header and capi.AGG_FUNCTIONS[name] == fid
    assert capi.COVARIANCE_FUNCTIONS == tuple(IDS)
    assert "PG_RESULT_COVARIANCE_TUPLE = 10" in header and capi.RESULT_COVARIANCE_TUPLE == 10
    assert capi.PgQuery._fields_[-1][0] == "agg_params"   # the query struct is unchanged
    # no new exported function: the tuple is read through pg_result_longs / pg_result_doubles
    exports = open(os.path.join(ROOT, "pinot_amd", "csrc", "libpinot_gpu.map")).read()
    assert "covar" not in exports.lower() and "pg_result_longs" in exports and "pg_result_doubles" in exports
    knobs = open(os.path.join(ROOT, "pinot_amd", "csrc", "pg_api.cpp")).read()
    assert '"PG_COVAR_HBM_MAX_BYTES", (int64_t)256 << 20' in knobs
    java = open(os.path.join(ROOT, "integration", "java", "org", "apache", "pinot", "gpu", "NativeQuery.java")).read()
    assert "CovarianceAggregationFunction ? 23 : -1" in java and "CovarianceAggregationFunction ? 24 : -1" in java


def test_covariance_records_through_the_shim(tmp_path):
    if not os.path.exists(capi.GPU_LIB_PATH):
        pytest.skip("libpinot_gpu.so not built here")
    csrc = os.path.join(ROOT, "pinot_amd", "csrc")
    exe = str(tmp_path / "shim_covariance_records")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "integration", "jni"), os.path.join(ROOT, "tests", "shim_covariance_records.c"),
                           os.path.join(ROOT, "integration", "jni", "pinot_gpu_shim.c"), "-L" + csrc, "-lpinot_gpu", "-Wl,-rpath," + csrc, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    for line in ("two covariance functions round-trip with their argument list", "a truncated record fails cleanly",
                 "a percentile next to them keeps its parameter", "a covariance takes no parameter", "wire format ok"):
        assert line in out.stdout
