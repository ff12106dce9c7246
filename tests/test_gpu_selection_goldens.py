"""Selection queries on the GPU path against the numbers of the reference's InnerSegmentSelectionSingleValueQueriesTest, on the same
segment as the other single-value goldens (BaseSingleValueQueriesTest), with and without its filter: ExecutionStatistics
(numDocsScanned, numEntriesScannedInFilter, numEntriesScannedPostFilter, numTotalDocs) and the rows it asserts."""
import ctypes as C

import pytest

from pinot_amd import capi
from pinot_amd.executor import NativeSegment
from pinot_amd.query import CQuery, parse_sql
from tests.fixtures import SV_FILTER, sv_segment

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sv(gpu_api, sv_data):
    host = sv_segment(sv_data)
    g = NativeSegment(gpu_api, host)
    yield host, g
    g.destroy()


def _stats(rb):
    s = rb.stats
    return (s.num_docs_scanned, s.num_entries_scanned_in_filter, s.num_entries_scanned_post_filter, s.num_total_docs)


def _col(rb, row, name):
    return rb.selection_rows[row][rb.key_columns.index(name)]


@pytest.mark.parametrize("where", ["", SV_FILTER])
def test_limit_zero(sv, where):
    host, g = sv
    rb = g.execute("SELECT * FROM testTable" + where + " LIMIT 0")
    assert _stats(rb) == (0, 0, 0, 30000)
    assert rb.selection_rows == []
    assert rb.stats.kernel.decode() == "pg_select_empty"


@pytest.mark.parametrize("where,stats,first", [
    ("", (10, 0, 110, 30000), (1578964907, "P")),
    (SV_FILTER, (10, 48204, 110, 30000), (351823652, "t")),
])
def test_select_star(sv, where, stats, first):
    host, g = sv
    rb = g.execute("SELECT * FROM testTable" + where)
    assert _stats(rb) == stats
    assert rb.stats.stats_exact == 1
    assert len(rb.key_columns) == 11 and rb.key_columns == sorted(rb.key_columns)
    assert len(rb.selection_rows) == 10
    assert (_col(rb, 0, "column1"), _col(rb, 0, "column11")) == first


@pytest.mark.parametrize("where,stats,first", [
    ("", (10, 0, 30, 30000), (1578964907, "P")),
    (SV_FILTER, (10, 48204, 30, 30000), (351823652, "t")),
])
def test_select_columns(sv, where, stats, first):
    host, g = sv
    rb = g.execute("SELECT column1, column5, column11 FROM testTable" + where)
    assert _stats(rb) == stats
    assert rb.key_columns == ["column1", "column5", "column11"]
    assert (_col(rb, 0, "column1"), _col(rb, 0, "column11")) == first


@pytest.mark.parametrize("where,stats,last", [
    ("", (30000, 0, 60020, 30000), (6043515, 10542595)),
    (SV_FILTER, (6129, 63064, 12278, 30000), (6043515, 462769197)),
])
def test_order_by(sv, where, stats, last):
    host, g = sv
    rb = g.execute("SELECT column1, column5, column11 FROM testTable" + where + " ORDER BY column6, column1")
    assert _stats(rb) == stats
    assert rb.key_columns == ["column6", "column1", "column5", "column11"]
    rows = rb.selection_rows
    assert len(rows) == 10
    assert rows == sorted(rows, key=lambda r: (r[0], r[1]))
    assert (rows[-1][0], rows[-1][1]) == last
    assert rb.stats.kernel.decode() == "pg_select_topk_lds"


def test_order_by_sorted_column_is_refused(gpu_api, sv):
    host, g = sv
    cq = CQuery(parse_sql("SELECT column1, column5 FROM testTable ORDER BY column5 LIMIT 10"), tuple(host.columns))
    assert host.columns["column5"].is_sorted
    assert gpu_api.f("query_supported")(g.handle, cq.ptr()) == capi.PG_ERR_UNSUPPORTED
    h = C.c_void_p()
    assert gpu_api.f("query_exec")(g.handle, cq.ptr(), C.byref(h)) == capi.PG_ERR_UNSUPPORTED
