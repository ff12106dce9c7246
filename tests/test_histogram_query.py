"""HISTOGRAM from SQL to the C ABI: every spelling and both forms parse to the canonical argument list, CQuery fills the function id 27, the
header and the bindings agree on the new constants, the ABI version, the query struct and the library's exports are unchanged, the malformed
forms raise SqlError with the reference's texts, a record with the function passes through the shim's C half (tests/shim_histogram_records.c
against integration/jni/pinot_gpu_shim.c), and the bindings' merge and final value are the model's."""
import os
import re
import subprocess

import pytest

from pinot_amd import capi, executor
from pinot_amd.query import CQuery, SqlError, parse_sql
from tests import histogram_model as hm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = hm.golden()


@pytest.mark.parametrize("spelling", ["HISTOGRAM", "histogram", "Histogram", "hIsToGrAm"])
def test_every_spelling_and_both_forms(spelling):
    qc = parse_sql(f"SELECT {spelling}(x, 0, 1000, 10) FROM t")
    assert [(a.function, a.column) for a in qc.aggregations] == [("HISTOGRAM", "x,'0','1000','10'")]
    qc = parse_sql(f"SELECT {spelling}( x , -999.5, '500.5' ,15 ) FROM t")
    assert qc.aggregations[0].column == "x,'-999.5','500.5','15'"
    qc = parse_sql(f'SELECT g, COUNT(*), {spelling}(lat, ARRAY["-Infinity", -1, 0.5, 1e3, "Infinity"]) FROM t WHERE s < 5 GROUP BY g '
                   f'ORDER BY {spelling.upper()}(lat, ARRAY["-Infinity",-1,0.5,1e3,"Infinity"]) DESC LIMIT 3')
    assert [(a.function, a.column) for a in qc.aggregations] == [("COUNT", None), ("HISTOGRAM", "lat,arrayvalueconstructor(-Infinity,'-1','0.5','1e3',Infinity)")]
    assert qc.resolved_order_by() == [(capi.ORDER_BY_AGGREGATION, 1, False)]   # any spelling names the same aggregation
    cq = CQuery(qc)
    assert cq.query.n_aggregations == 2 and cq.query.aggregations[1].function == 27
    assert cq.query.aggregations[1].column == b"lat,arrayvalueconstructor(-Infinity,'-1','0.5','1e3',Infinity)"
    assert not cq.query.agg_params   # the function takes no parameter: its bins travel in the argument list


@pytest.mark.parametrize("case", G["cases"] + [G["group_by"]], ids=lambda c: f"{c['x']}|{c['args']}"[:60])
def test_the_golden_queries_parse_to_the_canonical_list(case):
    qc = parse_sql(f"SELECT HISTOGRAM({case['x']},{case['args']}) FROM testTable")
    x = "add(intColumn,doubleColumn)" if case["x"].startswith("ADD") else case["x"]      # an expression argument travels as its canonical text
    assert qc.aggregations[0].column == hm.sql_arguments(x, case["args"])
    name, spec = hm.parse_arguments(qc.aggregations[0].column)
    assert name == x and spec.n_bins == len(case["expected"]["0"] if isinstance(case["expected"], dict) else case["expected"])


def test_next_to_other_aggregations():
    qc = parse_sql("SELECT HISTOGRAM(a, 0, 1, 4), KURTOSIS(a), VAR_POP(b), PERCENTILE(a, 95), SUM(a * b), COVAR_POP(a, b), HISTOGRAM(b, ARRAY[0, 1]) AS h FROM t GROUP BY g")
    cq = CQuery(qc)
    assert [cq.query.aggregations[i].function for i in range(7)] == [27, 26, 17, 16, 1, 23, 27]
    assert cq.query.agg_params[3] == 95.0 and cq.query.agg_params[0] == 0.0 and cq.query.agg_params[6] == 0.0
    assert parse_sql("SELECT HISTOGRAM(a + b, 0, 1, 4) FROM t").aggregations[0].column == "plus(a,b),'0','1','4'"


@pytest.mark.parametrize("case", G["invalid"], ids=lambda c: c["args"])
def test_the_reference_refusals_are_sql_errors(case):
    with pytest.raises(SqlError) as e:
        parse_sql(f"SELECT HISTOGRAM({case['args']}) FROM testTable")
    assert str(e.value) == case["reason"]


@pytest.mark.parametrize("sql,text", [
    ("SELECT HISTOGRAM(x, 0, 1000) FROM t", "Histogram expects 2 or 4 arguments, got: 3;"),
    ("SELECT HISTOGRAM(x, 0, 1, 2, 3) FROM t", "Histogram expects 2 or 4 arguments, got: 5;"),
    ("SELECT HISTOGRAM(x, 5) FROM t", "Please use the format of `Histogram(columnName, ARRAY[1,10,100])` to specify the bin edges"),
    ("SELECT HISTOGRAM(x, ARRAY[]) FROM t", "The number of bin edges must be greater than 1"),
    ("SELECT HISTOGRAM(x, ARRAY[3, 2]) FROM t", "The bin edges must be strictly increasing"),
    ("SELECT HISTOGRAM(x, ARRAY[\"Infinity\", 2]) FROM t", "The bin edges must be strictly increasing"),
    ("SELECT HISTOGRAM(x, 2.5, -1, 10) FROM t", "The right most edge must be greater than left most edge, given 2.5 and -1.0"),
    ("SELECT HISTOGRAM(x, 0, 1, 0) FROM t", "The number of bins must be greater than zero, given 0"),
    ("SELECT HISTOGRAM(x, 'a', 1, 3) FROM t", 'For input string: "a"'), ("SELECT HISTOGRAM(x, 0, 1, 2.5) FROM t", 'For input string: "2.5"'),
    ("SELECT HISTOGRAM(x, ARRAY[0, 'one']) FROM t", 'For input string: "one"'),
])
def test_malformed_forms(sql, text):
    with pytest.raises(SqlError) as e:
        parse_sql(sql)
    assert text in str(e.value)


def test_header_and_bindings_agree():
    header = open(os.path.join(ROOT, "include", "pinot_gpu.h")).read()
    assert "#define PG_ABI_VERSION 5" in header and capi.PG_ABI_VERSION == 5
    assert "PG_AGG_HISTOGRAM = 27" in header and capi.AGG_FUNCTIONS["HISTOGRAM"] == 27 and capi.HISTOGRAM_FUNCTIONS == ("HISTOGRAM",)
    assert "PG_RESULT_DOUBLE_ARRAY = 12" in header and capi.RESULT_DOUBLE_ARRAY == 12
    assert len(set(capi.AGG_FUNCTIONS.values())) == len(capi.AGG_FUNCTIONS) == 28
    assert capi.PgQuery._fields_[-1][0] == "agg_params"   # the query struct is unchanged
    # no new exported function: the arrays are read through pg_result_set_sizes / pg_result_set_values_double, and the exports are the header's
    exports = open(os.path.join(ROOT, "pinot_amd", "csrc", "libpinot_gpu.map")).read()
    assert "hist" not in exports.lower() and "pg_result_set_sizes" in exports and "pg_result_set_values_double" in exports
    declared = set(re.findall(r"\b(pg_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    exported = set(re.findall(r"\b(pg_[a-z0-9_]+);", exports))
    assert declared == exported
    api = open(os.path.join(ROOT, "pinot_amd", "csrc", "pg_api.cpp")).read()
    assert '"PG_HIST_HBM_MAX_BYTES", (int64_t)256 << 20' in api
    assert "{MERGED_HISTOGRAM," in api and api.index("{MERGED_WITH_TIME,") < api.index("{MERGED_HISTOGRAM,")   # the sixth side path of the (bit, refusal) table after PERCENTILE
    assert len(re.findall(r"\{MERGED_[A-Z_]+, \"", api)) == 7
    # the limits the header comment states are the code's
    k = hm.header_constants()
    assert k["PG_HIST_MAX_BINS"] == 65536 and "more than 65 536 bins in one histogram" in header
    assert k["PG_HIST_MAX_SPECS"] == 4 and "more than 4 distinct (column, bin specification) pairs" in header


def test_the_data_table_names_the_column():
    src = open(os.path.join(ROOT, "pinot_amd", "csrc", "pg_datatable.cpp")).read()
    assert 'case PG_AGG_HISTOGRAM: return "histogram";' in src
    assert re.search(r"case PG_RESULT_DOUBLE_ARRAY: \{.*?object\(3, p\);", src, re.S)


def test_merge_and_final_value_of_the_bindings():
    _, spec = hm.parse_arguments("x,'0','10','5'")
    a, b = hm.histogram(spec, [0.0, 1.0, 9.5, 10.0, 11.0]), hm.histogram(spec, [2.0, 2.5, -1.0])
    assert executor.histogram_merge(a, b) == hm.merge(a, b) == executor.merge_intermediate("HISTOGRAM", a, b) == (2.0, 2.0, 0.0, 0.0, 2.0)
    assert executor.extract_final("HISTOGRAM", list(a)) == a and isinstance(executor.extract_final("HISTOGRAM", list(a)), tuple)
    with pytest.raises(ValueError) as e:
        executor.histogram_merge(a, a[:-1])
    assert "not of the same size" in str(e.value)
    with pytest.raises(ValueError):
        executor.merge_intermediate("HISTOGRAM", a[:-1], a)
    four = a
    for _ in range(3):
        four = executor.histogram_merge(four, a)
    assert four == tuple(4 * v for v in a)


def test_histogram_records_through_the_shim(tmp_path):
    if not os.path.exists(capi.GPU_LIB_PATH):
        pytest.skip("libpinot_gpu.so not built here")
    csrc = os.path.join(ROOT, "pinot_amd", "csrc")
    exe = str(tmp_path / "shim_histogram_records")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "integration", "jni"), os.path.join(ROOT, "tests", "shim_histogram_records.c"),
                           os.path.join(ROOT, "integration", "jni", "pinot_gpu_shim.c"), "-L" + csrc, "-lpinot_gpu", "-Wl,-rpath," + csrc, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    for line in ("the function round-trips with its argument lists and without parameters", "a truncated record fails cleanly",
                 "a percentile next to it keeps its parameter", "a histogram takes no parameter", "wire format ok"):
        assert line in out.stdout
