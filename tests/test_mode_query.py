"""MODE above the executor, without a GPU: the spellings parse_sql takes and the reference's error texts, the ids / kind / flag of header
and binding, the unchanged export list, mode_merge / extract_final against tests/mode_model.py, the shim record, and the data table's
object layout in pg_datatable.cpp against the model's serializer."""
import math
import os
import re
import subprocess

import pytest

from pinot_amd import capi, executor
from pinot_amd.query import SqlError, parse_sql
from tests import mode_model as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_select_mode_parses():
    q = parse_sql("SELECT MODE(x) FROM t")   # a SqlError before MODE was carried
    assert [(a.function, a.column) for a in q.aggregations] == [("MODE", "x")]


@pytest.mark.parametrize("sql, column", [
    ("SELECT MODE(x) FROM t", "x"), ("select mode( x ) from t", "x"), ("SELECT Mode(x, 'MIN') FROM t", "x,'MIN'"), ("SELECT MODE(x ,'MAX' ) AS m FROM t", "x,'MAX'"),
    ("SELECT g, mOdE(lat.ms, 'AVG') FROM t WHERE s < 5 GROUP BY g", "lat.ms,'AVG'"),
])
def test_spellings(sql, column):
    q = parse_sql(sql)
    assert (q.aggregations[-1].function, q.aggregations[-1].column) == ("MODE", column)
    assert mm.parse_arguments(column) == (column.split(",")[0], executor.mode_reducer_of(column))


@pytest.mark.parametrize("sql, text", [
    ("SELECT MODE(x, 'MIN', 'MAX') FROM t", "Mode expects at most 2 arguments, got: 3"),
    ("SELECT MODE(x, 'MIN', 'MAX', 3) FROM t", "Mode expects at most 2 arguments, got: 4"),
    ("SELECT MODE(x, 'avg') FROM t", "No enum constant " + mm.ENUM + ".avg"),
    ("SELECT MODE(x, 'MEDIAN') FROM t", "No enum constant " + mm.ENUM + ".MEDIAN"),
    ("SELECT MODE(x, MAX) FROM t", "quoted MultiModeReducerType"),
    ("SELECT MODE(x, 5) FROM t", "quoted MultiModeReducerType"),
])
def test_malformed_forms(sql, text):
    with pytest.raises(SqlError) as e:
        parse_sql(sql)
    assert text in str(e.value)


def test_order_by_names_a_mode_by_its_canonical_list():
    q = parse_sql("SELECT g, MODE(x), mode(x, 'MAX'), COUNT(*) FROM t GROUP BY g ORDER BY Mode( x ,'MAX') DESC, MODE(x), g LIMIT 5")
    assert q.resolved_order_by() == [(capi.ORDER_BY_AGGREGATION, 1, False), (capi.ORDER_BY_AGGREGATION, 0, True), (capi.ORDER_BY_GROUP_KEY, 0, True)]
    assert parse_sql("SELECT g, MODE(x) FROM t GROUP BY g ORDER BY MODE(x, 'AVG')").resolved_order_by() is None   # another aggregation


def test_header_and_bindings_agree():
    header = open(os.path.join(ROOT, "include", "pinot_gpu.h")).read()
    assert "#define PG_ABI_VERSION 5" in header and capi.PG_ABI_VERSION == 5
    assert "PG_AGG_MODE = 28" in header and capi.PG_AGG_MODE == 28 and capi.AGG_FUNCTION_IDS["MODE"] == 28 and capi.MODE_FUNCTIONS == ("MODE",) and capi.MODE_REDUCERS == mm.REDUCERS
    assert "PG_RESULT_VALUE_COUNT_MAP = 13" in header and capi.RESULT_VALUE_COUNT_MAP == 13
    assert "#define PG_QUERY_FLAG_FINAL_MODE 0x400" in header and capi.QUERY_FLAG_FINAL_MODE == 0x400
    assert "#define PG_QUERY_FLAG_FINAL_PERCENTILE 0x200" in header and capi.QUERY_FLAG_FINAL_PERCENTILE == 0x200
    assert len(set(capi.AGG_FUNCTION_IDS.values())) == len(capi.AGG_FUNCTION_IDS) == 29 and dict(capi.AGG_FUNCTION_IDS, MODE=None) == dict(capi.AGG_FUNCTIONS, MODE=None)
    assert capi.PgQuery._fields_[-1][0] == "agg_params"   # the query struct is unchanged
    # no new exported function: the maps are read through the set getters, and the exports are the header's (the export-list test's count is untouched)
    exports = open(os.path.join(ROOT, "pinot_amd", "csrc", "libpinot_gpu.map")).read()
    declared = set(re.findall(r"\b(pg_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    exported = set(re.findall(r"\b(pg_[a-z0-9_]+);", exports))
    assert declared == exported and "mode" not in exports.lower() and "pg_result_set_counts" in exported
    api = open(os.path.join(ROOT, "pinot_amd", "csrc", "pg_api.cpp")).read()
    assert "kinds & MERGED_MODE" in api and "results of MODE aggregations are merged by value on the Java side" in api
    frame = open(os.path.join(ROOT, "pinot_amd", "csrc", "pg_exec_sidepass.hip")).read()
    assert "kPercentileBaseClears = PG_QUERY_FLAG_FINAL_PERCENTILE | PG_QUERY_FLAG_FINAL_MODE | PG_QUERY_FLAG_KEEP_DEVICE_TABLE" in frame
    assert len(re.findall(r"^    \{is_\w+_agg, ", frame, re.M)) == 7   # no new entry in kSidePaths: MODE joins the counting path
    for refusal in ("a STRING / BYTES or multi-value", "an expression x", "a group key space over 2^32", "PG_PCTL_SORT_MAX_BYTES"):
        assert refusal in header[header.index("/* MODE (ModeAggregationFunction.java"):header.index("PG_AGG_MODE = 28")]


def test_merge_and_final_value_of_the_bindings():
    a, b = mm.value_map([1, 1, 2, 7], "INT"), mm.value_map([2, 3, 7, 7], "INT")
    ea, eb = executor.mode_map("INT", [k for k, _ in a[1]], [c for _, c in a[1]]), executor.mode_map("INT", [7, 3, 2], [2, 1, 1])   # any entry order in
    assert ea == a and eb == b
    merged = executor.mode_merge(ea, eb)
    assert merged == mm.merge(a, b) == executor.merge_intermediate("MODE", ea, eb) == ("INT", ((1, 2), (2, 2), (3, 1), (7, 3)))
    assert executor.mode_merge(("INT", ()), eb) == eb and executor.mode_merge(ea, ("INT", ())) == ea
    with pytest.raises(ValueError) as e:
        executor.mode_merge(ea, executor.mode_map("LONG", [1], [1]))
    assert str(e.value) == "Illegal data type for Intermediate Result of MODE aggregation function: Int2LongOpenHashMap, Long2LongOpenHashMap"
    cases = [mm.value_map(v, t) for v, t in (([1, 1, 2, 2, 3], "INT"), ([5, 9, 9, 5, 7, 7], "LONG"), ([0.5, 0.25, 0.5, 0.25], "FLOAT"), ([0.1, 0.2, 0.3], "DOUBLE"),
                                             ([math.nan, math.nan, 1.0, 1.0], "DOUBLE"), ([0.0, -0.0], "DOUBLE"), ([math.inf, -math.inf, 1.0], "DOUBLE"), ([], "DOUBLE"),
                                             ([2**53 + 1, 2**53 + 3], "LONG"), ([1e308, 1e308 * 1.5, -1e308], "DOUBLE"))]
    for m in cases:
        for reducer, column in (("MIN", "x"), ("MIN", "x,'MIN'"), ("MAX", "x,'MAX'"), ("AVG", "x , 'AVG'")):
            assert mm.same_double(executor.extract_final("MODE", m, column), mm.final(m, reducer)), (m, reducer)
    assert executor.extract_final("MODE", ("INT", ()), "x,'AVG'") == -math.inf and executor.extract_final("MODE", 2.5, "x") == 2.5   # a final double stays
    with pytest.raises(ValueError):
        executor.mode_final(a, "avg")


def test_the_data_table_object_layout():
    """pg_datatable.cpp writes what the model's serializer writes: int size, then per entry the key in its own width and a long count, under
    ObjectSerDeUtils type 23 + the key type, 23 for an empty map; the column is mode(x); final values have no data table"""
    src = open(os.path.join(ROOT, "pinot_amd", "csrc", "pg_datatable.cpp")).read()
    assert 'case PG_AGG_MODE: return "mode";' in src
    body = re.search(r"case PG_RESULT_VALUE_COUNT_MAP: \{(.*?)\n        \}", src, re.S).group(1)
    assert re.search(r"p\.i32\(n\);.*case 0: p\.i32\(.*case 1: p\.i64\(.*case 2: .*float.*p\.i32\(b\).*default: p\.f64\(.*p\.i64\(ar\.l\[0\]", body, re.S)
    assert "object(n == 0 ? 23 : 23 + " in body
    assert "final MODE values (PG_QUERY_FLAG_FINAL_MODE) are not intermediate results: no data table" in src
    assert [mm.serialize(mm.value_map(v, t))[0] for v, t in (([1], "INT"), ([1], "LONG"), ([1.0], "FLOAT"), ([1.0], "DOUBLE"), ([], "FLOAT"))] == [23, 24, 25, 26, 23]
    assert mm.serialize(mm.value_map([7, 7, -1], "INT"))[1] == bytes.fromhex("00000002" "ffffffff" "0000000000000001" "00000007" "0000000000000002")


def test_mode_records_through_the_shim(tmp_path):
    if not os.path.exists(capi.GPU_LIB_PATH):
        pytest.skip("libpinot_gpu.so not built here")
    csrc = os.path.join(ROOT, "pinot_amd", "csrc")
    exe = str(tmp_path / "shim_mode_records")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "integration", "jni"), os.path.join(ROOT, "tests", "shim_mode_records.c"),
                           os.path.join(ROOT, "integration", "jni", "pinot_gpu_shim.c"), "-L" + csrc, "-lpinot_gpu", "-Wl,-rpath," + csrc, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    for line in ("the function round-trips with its argument lists and without parameters", "a truncated record fails cleanly",
                 "a percentile next to it keeps its parameter", "a mode takes no parameter", "wire format ok"):
        assert line in out.stdout
