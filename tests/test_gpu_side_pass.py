"""What the side passes — exact PERCENTILE (pg_exec_percentile.hip), aggregations over an expression (pg_exec_expr.hip), the variance family
(pg_exec_var.hip), COVAR_POP / COVAR_SAMP (pg_exec_covar.hip) and SKEWNESS / KURTOSIS (pg_exec_moment.hip) — share: the split of the query, the
filter's match words, the join by group key and the statistics written at the end (pg_exec_sidepass.hip).  All paths run the same shapes over
the segments of tests/test_gpu_percentile.py at 1, 64 and 1 003 docs (the last match word of 1 003 docs is partial: with a filter the word
comes from the filter, without one it is made up in the kernel), and are held to the models of their modules.  Between them the sum-table
paths cover the integer path (v7) and the double path (ld, a dictionary LONG).  The last test nests all six side paths of the frame's table
in one query."""
import numpy as np
import pytest

from pinot_amd import capi
from pinot_amd.executor import CancelToken, NativeSegment
from pinot_amd.query import CQuery, parse_sql, with_time_arguments
from tests import covariance_model as cm
from tests import expression_model as em
from tests import fourth_moment_model as fm
from tests import percentile_model as pm
from tests import variance_model as vm
from tests import with_time_model as wm
from tests import test_gpu_covariance as tc
from tests import test_gpu_expressions as te
from tests import test_gpu_moments as tm
from tests import test_gpu_percentile as tp
from tests import test_gpu_variance as tv

pytestmark = pytest.mark.gpu
SIZES = [1, 64, 1003]
SIDE = {"percentile": "PERCENTILE(v7, 50)", "expression": "SUM(add(v7, v3))", "variance": "VAR_POP(v7)", "covariance": "COVAR_SAMP(v7, ld)",
        "moment": "KURTOSIS(ld)"}
SIDE_COLUMNS = {"percentile": ["v7"], "expression": ["v7", "v3"], "variance": ["v7"], "covariance": ["v7", "ld"], "moment": ["ld"]}
CHECK = {"percentile": tp._check, "expression": te._check, "variance": tv._check, "covariance": tc._check, "moment": tm._check}
# the sum-table paths: the kernels' prefix, the slots of a group's row (v7 is an INT column: the integer path; ld a LONG: the double path)
# and the LDS tier's slots (side_tier)
TABLE = {
    "expression": ("pg_expr", 4, 16384),                                                          # the four limbs of one SUM
    "variance": ("pg_var", 1 + tv.K["PG_VAR_INT_SLOTS"], tv.LDS_SLOTS),                          # the doc count, Sx, two digits of Sq
    "covariance": ("pg_covar", cm.slots_per_group(["INT", "LONG"], 1, tc.K), tc.LDS_SLOTS),      # the count, two sums, one pair's products
    "moment": ("pg_moment", 1 + tm.DBL_SLOTS, tm.LDS_SLOTS),                                     # the count, the digits of x .. x^4
}
GROUP_BY = [[], ["rg"], ["g7", "rg"]]   # rg is a raw column: its groups come back as values and are mapped through its virtual dictionary
WHERE = " WHERE s < 700"

_SEGMENTS = {}


@pytest.fixture(scope="module")
def segments(gpu_api, oracle_api):
    def get(n):
        if n not in _SEGMENTS:
            host, data, schema = tp._data(n)
            _SEGMENTS[n] = (host, data, schema, NativeSegment(gpu_api, host), NativeSegment(oracle_api, host))
        return _SEGMENTS[n]
    yield get
    for _, _, _, g, o in _SEGMENTS.values():
        g.destroy()
        o.destroy()
    _SEGMENTS.clear()


def _sql(select, group_by, filtered):
    keys = ", ".join(group_by)
    return "SELECT " + (keys + ", " if keys else "") + select + " FROM t" + (WHERE if filtered else "") + (" GROUP BY " + keys if keys else "")


def _id_bits(data, column):
    """bits of a value-ordered id of the column: a dictionary's dictIds and a virtual dictionary's ids are sized alike"""
    return max(1, (len(np.unique(np.asarray(data[column]))) - 1).bit_length())


def _kernel(path, data, group_by):
    """the tier the default knobs choose: PG_PCTL_LDS_KEYS = 32 768 counters; a sum table in registers without GROUP BY, in LDS up to the
    path's LDS slots (16 384 each), else in HBM"""
    groups = 1
    for g in group_by:
        groups *= len(np.unique(np.asarray(data[g])))
    if path == "percentile":
        return "pg_pctl_lds" if groups * len(np.unique(data["v7"])) <= 32768 else "pg_pctl_hbm"
    prefix, slots, lds_slots = TABLE[path]
    return prefix + ("_reg" if not group_by else ("_lds" if groups * slots <= lds_slots else "_hbm"))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("group_by", GROUP_BY, ids=lambda g: "by_" + "_".join(g) if g else "no_group_by")
@pytest.mark.parametrize("filtered", [False, True], ids=["all_docs", "filtered"])
@pytest.mark.parametrize("path", sorted(SIDE))
def test_statistics_of_both_paths(segments, path, filtered, group_by, n):
    seg = segments(n)
    host, data, schema, gpu, oracle = seg
    sql = _sql(SIDE[path], group_by, filtered)
    # groups, values, numDocsScanned, numEntriesScannedPostFilter, numEntriesScannedInFilter, stats_exact, numTotalDocs and the kernel's name
    b = CHECK[path](seg, sql, kernel=_kernel(path, data, group_by))
    assert b.stats.star_tree_index == -1
    # the pass's bytes on top of the ordinary part's: one read of the ids of every doc, and of the match words when there is a filter
    ordinary = gpu.execute(_sql("COUNT(*)", group_by, filtered))
    id_bits = sum(_id_bits(data, c) for c in SIDE_COLUMNS[path] + group_by)
    n_words = (host.total_docs + 63) // 64
    want = (host.total_docs * id_bits + 7) // 8 + (n_words * 8 if filtered else 0)
    print(f"{sql}: algorithmic_bytes {b.stats.algorithmic_bytes}, ordinary part {ordinary.stats.algorithmic_bytes}, the pass by formula {want}")
    assert b.stats.algorithmic_bytes - ordinary.stats.algorithmic_bytes == want, sql


@pytest.mark.parametrize("path", sorted(SIDE))
def test_profile_flag(segments, path):
    gpu = segments(1003)[3]
    sql = _sql(SIDE[path], ["g7"], True)
    st = gpu.execute(parse_sql(sql), profile=True).stats
    print(f"{sql}: device_ms total {st.device_ms_total}, filter {st.device_ms_filter}, aggregate {st.device_ms_aggregate}")
    assert st.device_ms_aggregate > 0
    # the pass is part of device_ms_aggregate, the filter's pass is device_ms_filter: the total holds both (float sums: 1e-4 ms of slack)
    assert st.device_ms_total >= st.device_ms_filter + st.device_ms_aggregate - 1e-4
    plain = gpu.execute(parse_sql(sql)).stats
    ordinary = gpu.execute(_sql("COUNT(*)", ["g7"], True)).stats
    assert plain.device_ms_aggregate == ordinary.device_ms_aggregate == 0.0   # no events without the flag


def test_cancellation_on_the_expression_path(gpu_api, segments):
    seg = segments(1003)
    sql = _sql(SIDE["expression"], ["g7"], False)
    token = CancelToken(gpu_api)
    try:
        token.request()
        with pytest.raises(capi.NativeError) as e:
            seg[3].execute_native(sql, cancel=token)
        assert e.value.status == capi.PG_ERR_CANCELLED
        token.reset()
        r = seg[3].execute_native(sql, cancel=token)
        rows = r.block().rows()
        r.free()
    finally:
        token.destroy()
    groups = pm.group_docs([seg[1]["g7"]], np.arange(1003))
    v = em.evaluate("add(v7,v3)", seg[1], seg[2])
    assert set(rows) == set(groups)
    for key, gdocs in groups.items():
        assert pm.same_double(rows[key][0], em.agg_sum(v[gdocs])), key


def _three_kinds(seg, group_by):
    """an expression aggregation, a PERCENTILE and a plain aggregation the query is ordered by: aggregation 2 of the query is aggregation 1
    of the expression path's ordinary part and aggregation 0 of the percentile path's"""
    host, data, schema, gpu, oracle = seg
    keys = ", ".join(group_by)
    qc = parse_sql(f"SELECT {keys}, SUM(add(v7,v3)), PERCENTILE(v3, 95), MAX(v7) FROM t{WHERE} GROUP BY {keys} ORDER BY MAX(v7) DESC LIMIT 3")
    qc.min_segment_group_trim_size = 1   # trimSize = max(5 x limit, 1) = 15 groups
    b = gpu.execute(qc)
    assert b.stats.percentile_passes == 1 and b.stats.star_tree_index == -1
    docs, in_filter = tp._filter(oracle, "SELECT COUNT(*) FROM t" + WHERE)
    assert b.stats.num_docs_scanned == len(docs) and b.stats.num_entries_scanned_in_filter == in_filter
    assert b.stats.num_entries_scanned_post_filter == len(docs) * len(set(group_by) | {"v7", "v3"})
    groups = pm.group_docs([data[g] for g in group_by], docs)
    v = em.evaluate("add(v7,v3)", data, schema)
    rows = b.rows()
    for key, (total, runs, mx) in rows.items():
        gdocs = groups[key]
        assert pm.same_double(total, em.agg_sum(v[gdocs])), key
        assert pm.same_runs(runs, pm.runs(pm.as_doubles(np.asarray(data["v3"])[gdocs], "INT"))), key
        assert mx == float(np.max(np.asarray(data["v7"])[gdocs])), key
    return rows, {key: float(np.max(np.asarray(data["v7"])[gdocs])) for key, gdocs in groups.items()}


def test_all_three_kinds_with_order_by_and_limit(segments):
    seg = segments(1003)
    rows, maxima = _three_kinds(seg, ["g7"])
    assert set(rows) == set(maxima) and len(rows) == 7         # seven groups are below the trim size: every one comes back
    rows, maxima = _three_kinds(seg, ["g7", "g20"])              # ~140 groups: the 15 with the largest MAX(v7) survive (ties at the cut: any)
    assert len(maxima) > 15 and len(rows) == 15
    cut = sorted(maxima.values(), reverse=True)[14]
    assert all(maxima[key] >= cut for key in rows)
    assert all(key in rows for key, m in maxima.items() if m > cut)
    # a result that carries both kinds is merged by value on the Java side
    a = seg[3].execute_native("SELECT g7, SUM(add(v7,v3)), PERCENTILE(v3, 95), MAX(v7) FROM t GROUP BY g7")
    b = seg[3].execute_native("SELECT g7, SUM(add(v7,v3)), PERCENTILE(v3, 95), MAX(v7) FROM t GROUP BY g7")
    try:
        with pytest.raises(capi.NativeError) as e:
            a.merge(b)
        assert e.value.status == capi.PG_ERR_UNSUPPORTED and "merged by value" in e.value.message
    finally:
        a.free()
        b.free()


def test_all_four_kinds_nested_in_one_query(gpu_api, segments):
    """the table of side paths end to end, all six entries: the expression pass outside, the FIRSTWITHTIME pass inside it, then the
    covariance's, the SKEWNESS / KURTOSIS pass, the variance's, the PERCENTILE's innermost, a plain SUM in the ordinary part at the bottom —
    and pg_query_supported walking the same nesting"""
    seg = segments(1003)
    host, data, schema, gpu, oracle = seg
    sql = ("SELECT g7, SUM(add(v7,v3)), FIRSTWITHTIME(v3, ld, 'INT'), VAR_POP(v7), PERCENTILE(v3, 95), SUM(s), COVAR_SAMP(v7, ld), KURTOSIS(ld) FROM t"
           + WHERE + " GROUP BY g7")
    qc = parse_sql(sql)
    gpu_api.call("query_supported", gpu.handle, CQuery(qc).ptr())   # PG_OK: anything else raises
    b = gpu.execute(qc)
    assert b.stats.kernel.decode() == "pg_expr_lds" and b.stats.percentile_passes == 1 and b.stats.star_tree_index == -1
    docs, in_filter = tp._filter(oracle, "SELECT COUNT(*) FROM t" + WHERE)
    assert b.stats.num_entries_scanned_in_filter == in_filter
    assert (b.stats.num_docs_scanned, b.stats.num_entries_scanned_post_filter) == pm.statistics(len(docs), {"g7", "v7", "v3", "ld", "s"})
    groups = pm.group_docs([data["g7"]], docs)
    rows = b.rows()
    assert set(rows) == set(groups) and len(rows) == 7
    v = em.evaluate("add(v7,v3)", data, schema)
    x, t, declared = with_time_arguments(qc.aggregations[1].column)
    assert (x, t, declared) == ("v3", "ld", "INT")
    for key, gdocs in groups.items():
        total, first, var, runs, plain, covar, moment = rows[key]
        gdocs = np.sort(np.asarray(gdocs, dtype=np.int64))
        v7, ld = tc._doubles(data, schema, "v7", gdocs), tc._doubles(data, schema, "ld", gdocs)
        assert tc._same_tuple(covar, cm.exact_tuple(v7, ld)), key
        assert fm.same_tuple(moment, fm.exact_tuple(ld)), key
        assert pm.same_double(total, em.agg_sum(v[gdocs])), key
        assert wm.pair_bits(declared, *first) == wm.aggregate("FIRSTWITHTIME", schema[x], data[x], data[t], gdocs, declared), key
        want = vm.exact_tuple(vm.as_doubles(np.asarray(data["v7"])[gdocs], "INT"))
        assert var[0] == want[0] and vm.same_bits(var[1], want[1]) and vm.same_bits(var[2], want[2]), key
        assert pm.same_runs(runs, pm.runs(pm.as_doubles(np.asarray(data["v3"])[gdocs], "INT"))), key
        assert plain == float(np.sum(np.asarray(data["s"], dtype=np.int64)[gdocs])), key
    # a refusal of the innermost path comes up through every level, from the check and from the execution alike
    qc.aggregations[3].percentile = 101.0
    statuses = []
    for call in ("query_supported", "query_exec"):
        with pytest.raises(capi.NativeError) as e:
            if call == "query_supported":
                gpu_api.call(call, gpu.handle, CQuery(qc).ptr())
            else:
                gpu_api.call(call, gpu.handle, CQuery(qc).ptr(), capi.C.byref(capi.C.c_void_p()))
        assert "the percentile must be in [0, 100]" in e.value.message, (call, e.value.message)
        statuses.append(e.value.status)
    assert statuses == [capi.PG_ERR_INVALID_ARGUMENT] * 2
