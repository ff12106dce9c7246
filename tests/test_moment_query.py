"""SKEWNESS / KURTOSIS from SQL to the C ABI: every spelling parses to the two canonical names, CQuery fills the function ids 25 / 26, the
header and the bindings agree on the new constants, the ABI version and the query struct are unchanged, a record with the two functions
passes through the shim's C half (tests/shim_moment_records.c against integration/jni/pinot_gpu_shim.c), and the data table names the
columns skewness(x) / kurtosis(x) as objects of type 34."""
import os
import re
import subprocess

import pytest

from pinot_amd import capi
from pinot_amd.query import CQuery, parse_sql

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPELLINGS = {"SKEWNESS": ["SKEWNESS", "skewness", "Skewness", "sKeWnEsS"], "KURTOSIS": ["KURTOSIS", "kurtosis", "Kurtosis"]}
IDS = {"SKEWNESS": 25, "KURTOSIS": 26}


@pytest.mark.parametrize("function,spelling", [(f, s) for f, ss in SPELLINGS.items() for s in ss])
def test_every_spelling_parses(function, spelling):
    qc = parse_sql(f"SELECT {spelling}(x) FROM t")
    assert [(a.function, a.column) for a in qc.aggregations] == [(function, "x")]
    qc = parse_sql(f"SELECT g, COUNT(*), {spelling}( lat ) FROM t WHERE s < 5 GROUP BY g ORDER BY {spelling.upper()}(lat) DESC LIMIT 3")
    assert [(a.function, a.column) for a in qc.aggregations] == [("COUNT", None), (function, "lat")]
    assert qc.resolved_order_by() == [(capi.ORDER_BY_AGGREGATION, 1, False)]   # any spelling names the same aggregation
    cq = CQuery(qc)
    assert cq.query.n_aggregations == 2 and cq.query.aggregations[1].function == IDS[function] and cq.query.aggregations[1].column == b"lat"
    assert not cq.query.agg_params   # the functions take no parameter


def test_function_ids_and_an_expression_argument():
    qc = parse_sql("SELECT SKEWNESS(a), KURTOSIS(a), VAR_POP(b), PERCENTILE(a, 95), SUM(a * b), COVAR_POP(a, b) FROM t GROUP BY g")
    cq = CQuery(qc)
    assert [cq.query.aggregations[i].function for i in range(6)] == [25, 26, 17, 16, 1, 23]
    assert cq.query.agg_params[3] == 95.0 and cq.query.agg_params[0] == 0.0
    # an expression argument travels as its canonical text (the library refuses it: "<FN> over an expression")
    qc = parse_sql("SELECT KURTOSIS(a + b) FROM t")
    assert (qc.aggregations[0].function, qc.aggregations[0].column) == ("KURTOSIS", "plus(a,b)")


def test_header_and_bindings_agree():
    header = open(os.path.join(ROOT, "include", "pinot_gpu.h")).read()
    assert "#define PG_ABI_VERSION 5" in header and capi.PG_ABI_VERSION == 5
    for name, fid in IDS.items():
        assert f"PG_AGG_{name} = {fid}" in header and capi.AGG_FUNCTIONS[name] == fid
    assert capi.FOURTH_MOMENT_FUNCTIONS == tuple(IDS)
    assert "PG_RESULT_FOURTH_MOMENT = 11" in header and capi.RESULT_FOURTH_MOMENT == 11
    assert capi.PgQuery._fields_[-1][0] == "agg_params"   # the query struct is unchanged
    # no new exported function: the tuple is read through pg_result_longs / pg_result_doubles
    exports = open(os.path.join(ROOT, "pinot_amd", "csrc", "libpinot_gpu.map")).read()
    assert "moment" not in exports.lower() and "pg_result_longs" in exports and "pg_result_doubles" in exports
    knobs = open(os.path.join(ROOT, "pinot_amd", "csrc", "pg_api.cpp")).read()
    assert '"PG_MOMENT_HBM_MAX_BYTES", (int64_t)256 << 20' in knobs
    # the doubles accessor reaches m3 and m4 of this kind only
    assert "a.kind == PG_RESULT_FOURTH_MOMENT ? 4" in knobs
    # the per-query column limit the header comment states is the kernels'
    limit = int(re.search(r"#define PG_MOMENT_MAX_COLS (\d+)", open(os.path.join(ROOT, "pinot_amd", "csrc", "pg_moment4.h")).read()).group(1))
    assert limit >= 2 and f"more\n   * than {limit} distinct argument columns in one query" in header


def test_the_data_table_names_the_columns():
    src = open(os.path.join(ROOT, "pinot_amd", "csrc", "pg_datatable.cpp")).read()
    assert 'case PG_AGG_SKEWNESS: return "skewness";' in src and 'case PG_AGG_KURTOSIS: return "kurtosis";' in src
    assert re.search(r"case PG_RESULT_FOURTH_MOMENT: \{.*?object\(34, p\);", src, re.S)


def test_final_values_and_merge_of_the_bindings():
    from pinot_amd import executor
    from tests import fourth_moment_model as fm
    xs = [1.0, 2.0, 4.0, 8.0, 16.0, 3.5, -2.25]
    t = fm.exact_tuple(xs)
    assert executor.skewness_final(t) == fm.skewness(t) and executor.kurtosis_final(t) == fm.kurtosis(t)
    assert executor.extract_final("SKEWNESS", t) == fm.skewness(t) and executor.extract_final("KURTOSIS", t) == fm.kurtosis(t)
    a, b = fm.exact_tuple(xs[:3]), fm.exact_tuple(xs[3:])
    assert executor.fourth_moment_merge(a, b) == fm.combine(a, b) == executor.merge_intermediate("KURTOSIS", a, b)
    empty = fm.exact_tuple([])
    assert executor.fourth_moment_merge(empty, b) == b and executor.fourth_moment_merge(a, empty) == a
    assert str(executor.skewness_final(fm.exact_tuple(xs[:2]))) == "nan" and str(executor.kurtosis_final(fm.exact_tuple(xs[:3]))) == "nan"
    assert executor.skewness_final(fm.exact_tuple([5.0] * 9)) == 0.0 and executor.kurtosis_final(fm.exact_tuple([5.0] * 9)) == 0.0


def test_moment_records_through_the_shim(tmp_path):
    if not os.path.exists(capi.GPU_LIB_PATH):
        pytest.skip("libpinot_gpu.so not built here")
    csrc = os.path.join(ROOT, "pinot_amd", "csrc")
    exe = str(tmp_path / "shim_moment_records")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "integration", "jni"), os.path.join(ROOT, "tests", "shim_moment_records.c"),
                           os.path.join(ROOT, "integration", "jni", "pinot_gpu_shim.c"), "-L" + csrc, "-lpinot_gpu", "-Wl,-rpath," + csrc, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    for line in ("the two functions round-trip without parameters", "a truncated record fails cleanly",
                 "a percentile next to them keeps its parameter", "a fourth moment takes no parameter", "wire format ok"):
        assert line in out.stdout
