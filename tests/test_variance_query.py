"""VAR_POP / VAR_SAMP / STDDEV_POP / STDDEV_SAMP from SQL to the C ABI: every spelling parses to the four canonical names
(AggregationFunctionType strips underscores and ignores case), CQuery fills the function ids 17-20, the header and the bindings agree on the
new constants, the ABI version and the query struct are unchanged, and a record with the four functions passes through the shim's C half
(tests/shim_variance_records.c against integration/jni/pinot_gpu_shim.c)."""
import os
import subprocess

import pytest

from pinot_amd import capi
from pinot_amd.query import CQuery, parse_sql

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPELLINGS = {
    "VARPOP": ["VAR_POP", "VARPOP", "var_pop", "Var_Pop", "varPop"],
    "VARSAMP": ["VAR_SAMP", "VARSAMP", "var_samp", "varSamp"],
    "STDDEVPOP": ["STDDEV_POP", "STDDEVPOP", "stddev_pop", "stdDevPop", "STD_DEV_POP"],
    "STDDEVSAMP": ["STDDEV_SAMP", "STDDEVSAMP", "stddev_samp", "stdDevSamp", "STD_DEV_SAMP"],
}
IDS = {"VARPOP": 17, "VARSAMP": 18, "STDDEVPOP": 19, "STDDEVSAMP": 20}


@pytest.mark.parametrize("function,spelling", [(f, s) for f, ss in SPELLINGS.items() for s in ss])
def test_every_spelling_parses(function, spelling):
    qc = parse_sql(f"SELECT {spelling}(x) FROM t")
    assert [(a.function, a.column) for a in qc.aggregations] == [(function, "x")]
    qc = parse_sql(f"SELECT g, COUNT(*), {spelling}( lat ) FROM t WHERE s < 5 GROUP BY g ORDER BY {spelling}(lat) DESC LIMIT 3")
    assert [(a.function, a.column) for a in qc.aggregations] == [("COUNT", None), (function, "lat")]
    assert qc.resolved_order_by() == [(capi.ORDER_BY_AGGREGATION, 1, False)]   # any spelling names the same aggregation
    cq = CQuery(qc)
    assert cq.query.n_aggregations == 2 and cq.query.aggregations[1].function == IDS[function] and cq.query.aggregations[1].column == b"lat"
    assert not cq.query.agg_params   # the functions take no parameter


def test_function_ids_and_an_expression_argument():
    qc = parse_sql("SELECT VAR_POP(a), VAR_SAMP(a), STDDEV_POP(b), STDDEV_SAMP(b), PERCENTILE(a, 95), SUM(a * b) FROM t GROUP BY g")
    cq = CQuery(qc)
    assert [cq.query.aggregations[i].function for i in range(6)] == [17, 18, 19, 20, 16, 1]
    assert cq.query.agg_params[4] == 95.0 and cq.query.agg_params[0] == 0.0
    # an expression argument travels as its canonical text (the library refuses it: "<FN> over an expression")
    qc = parse_sql("SELECT STDDEV_POP(a + b) FROM t")
    assert (qc.aggregations[0].function, qc.aggregations[0].column) == ("STDDEVPOP", "plus(a,b)")


def test_header_and_bindings_agree():
    header = open(os.path.join(ROOT, "include", "pinot_gpu.h")).read()
    assert "#define PG_ABI_VERSION 5" in header and capi.PG_ABI_VERSION == 5
    for name, fid in IDS.items():
        assert f"PG_AGG_{name} = {fid}" in header and capi.AGG_FUNCTIONS[name] == fid
    assert capi.VARIANCE_FUNCTIONS == tuple(IDS)
    assert "PG_RESULT_VARIANCE_TUPLE = 8" in header and capi.RESULT_VARIANCE_TUPLE == 8
    assert capi.PgQuery._fields_[-1][0] == "agg_params"   # the query struct is unchanged
    # no new exported function: the tuple is read through pg_result_longs / pg_result_doubles
    exports = open(os.path.join(ROOT, "pinot_amd", "csrc", "libpinot_gpu.map")).read()
    assert "var" not in exports.lower() and "pg_result_longs" in exports and "pg_result_doubles" in exports
    knobs = open(os.path.join(ROOT, "pinot_amd", "csrc", "pg_api.cpp")).read()
    assert '"PG_VAR_HBM_MAX_BYTES", (int64_t)256 << 20' in knobs


def test_variance_records_through_the_shim(tmp_path):
    if not os.path.exists(capi.GPU_LIB_PATH):
        pytest.skip("libpinot_gpu.so not built here")
    csrc = os.path.join(ROOT, "pinot_amd", "csrc")
    exe = str(tmp_path / "shim_variance_records")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "integration", "jni"), os.path.join(ROOT, "tests", "shim_variance_records.c"),
                           os.path.join(ROOT, "integration", "jni", "pinot_gpu_shim.c"), "-L" + csrc, "-lpinot_gpu", "-Wl,-rpath," + csrc, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    for line in ("four variance functions round-trip without parameters", "a truncated record fails cleanly",
                 "a percentile next to them keeps its parameter", "a variance takes no parameter", "wire format ok"):
        assert line in out.stdout
