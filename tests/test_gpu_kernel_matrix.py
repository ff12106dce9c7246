"""Every kernel the dispatcher can name (tests/kernel_inventory.py) against the CPU oracle, at the sizes of the ladder where the planner picks
it: pg_exec_stats.kernel must be exactly the entry's name, the rows and ExecutionStatistics the oracle's, and a second execution of the cached
plan must run the same kernel and return the same answer.  test_kernel_families_back_to_back runs every family of one size in table order and
in reverse on one thread, switching knobs between them: the per-thread state that outlives a query (the aggregation scratch a kernel leaves
zeroed, the counters the reduce kernel resets, the reused buffers) must not leak into the next query, whichever kernel it runs."""
import numpy as np
import pytest

from pinot_amd import capi
from pinot_amd.executor import NativeSegment, _key_repr
from pinot_amd.query import parse_sql
from pinot_amd.segment import decode_column
from tests import distinct_model as dm
from tests import kernel_inventory as ki
from tests import selection_model as sm
from tests.fixtures import compare_with_oracle

pytestmark = pytest.mark.gpu

STATS = ("num_docs_scanned", "num_entries_scanned_in_filter", "num_entries_scanned_post_filter", "num_total_docs", "num_groups_limit_reached",
         "stats_exact")


class Segments:
    """One GPU and one oracle segment per (builder, size, snapshot), both registered from the same host segment."""

    def __init__(self, gpu_api, oracle_api):
        self.gpu_api, self.oracle_api = gpu_api, oracle_api
        self.hosts, self.pairs = {}, {}

    def get(self, builder, n, snapshot):
        key = (builder, n, snapshot)
        if key not in self.pairs:
            if (builder, n) not in self.hosts:
                self.hosts[(builder, n)] = ki.BUILDERS[builder](n)
            host = self.hosts[(builder, n)]
            g, o = NativeSegment(self.gpu_api, host), NativeSegment(self.oracle_api, host)
            if snapshot:
                ids = ki.snapshot_doc_ids(n)
                g.set_queryable_doc_ids(ids)
                o.set_queryable_doc_ids(ids)
            self.pairs[key] = (host, g, o)
        return self.pairs[key]

    def destroy(self):
        for _, g, o in self.pairs.values():
            g.destroy()
            o.destroy()
        self.pairs.clear()
        self.hosts.clear()


@pytest.fixture(scope="module")
def segments(gpu_api, oracle_api):
    s = Segments(gpu_api, oracle_api)
    yield s
    s.destroy()


def _query(e):
    qc = parse_sql(e.sql)
    if e.exact:
        qc.flags |= capi.QUERY_FLAG_EXACT_FILTER_STATS
    if e.groups_limit:
        qc.num_groups_limit = e.groups_limit
    return qc


def _match_docs(o, sql):
    """the oracle's matching docIds of the query's filter (the snapshot's docs when there is none)"""
    where = sql.split(" FROM ", 1)[1].split(" ORDER BY ")[0].split(" LIMIT ")[0]
    return o.filter("SELECT COUNT(*) FROM " + where)


# ---- what the oracle says, once per (entry, size) --------------------------------------------------------------------------------
_EXPECTED = {}


def _decoded(host, col):
    c = host.columns[col]
    if c.has_dictionary:
        ids = decode_column(c, host.total_docs, dict_ids=True).astype(np.int64)
        return np.asarray(c.dict_values, dtype=object)[ids], ids
    v = decode_column(c, host.total_docs)
    return v, None


def _expected(e, n, host, o):
    key = (e.name, n)
    if key in _EXPECTED:
        return _EXPECTED[key]
    qc = parse_sql(e.sql)
    if e.entry == "execute":
        want = o.execute(_query(e))
    elif e.entry == "filter":
        od = o.filter(e.sql)
        want = (od.doc_ids(), od.stats())
        od.free()
    else:
        fd = _match_docs(o, e.sql)
        docs, fstats = fd.doc_ids(), fd.stats()
        fd.free()
        if e.entry == "distinct":
            # per column: the id of every doc (dictIds; value-ordered ids of a raw column) and the value of every id
            cols = [_ids(host, c) for c in qc.distinct]
            ids = [i for i, _ in cols]
            order = [(qc.distinct.index(t), asc) for t, asc in qc.order_by]
            dict_path = " WHERE " not in e.sql and len(cols) == 1 and host.columns[qc.distinct[0]].has_dictionary
            if dict_path:   # DictionaryBasedDistinctOperator: the dictionary's first (last) values, whatever the snapshot
                model = dm.dictionary_path(len(cols[0][1]), qc.limit, bool(order) and not order[0][1])
            else:
                model = dm.distinct(ids, docs, qc.limit, order or None)
            want = (model, [v for _, v in cols], dict_path, fstats)
        else:
            out = qc.extract_expressions(host.columns)
            cols = {c: _decoded(host, c) for c in set(out)}
            values = [cols[c][0] for c in out]
            order, seen = [], set()
            if qc.limit > 0:
                for text, asc in qc.order_by:
                    if text not in seen:
                        seen.add(text)
                        v, i = cols[text]
                        order.append((out.index(text), asc, sm.order_values(None, i) if i is not None else sm.order_values(v, None)))
            model = sm.selection(values, docs, qc.limit, len(set(out)), order or None)
            want = (model, out, cols, fstats)
    _EXPECTED[key] = want
    return want


# ---- one execution on the GPU, checked against the oracle -------------------------------------------------------------------------
def _run(e, host, g):
    """(kernel, comparable answer, raw result) of one execution on the GPU"""
    if e.entry == "filter":
        gd = g.filter(e.sql)
        out = (gd.doc_ids(), gd.stats())
        gd.free()
        return out[1].kernel.decode(), out, out
    rb = g.execute(_query(e))
    if e.entry == "execute":
        answer = (rb.rows(), tuple(getattr(rb.stats, f) for f in STATS))
    elif e.entry == "distinct":
        answer = (list(rb.distinct_rows), tuple(getattr(rb.stats, f) for f in STATS))
    else:
        answer = (list(rb.selection_rows), tuple(getattr(rb.stats, f) for f in STATS))
    return rb.stats.kernel.decode(), answer, rb


def _check(e, n, host, o, raw, what):
    want = _expected(e, n, host, o)
    if e.entry == "execute":
        compare_with_oracle(raw, want, what)
        return
    if e.entry == "filter":
        gdocs, gs = raw
        odocs, os_ = want
        np.testing.assert_array_equal(gdocs, odocs, err_msg=what)
        for f in ("num_docs_scanned", "num_entries_scanned_in_filter", "num_total_docs"):
            assert getattr(gs, f) == getattr(os_, f), (what, f, getattr(gs, f), getattr(os_, f))
        assert gs.stats_exact == 1, what
        return
    qc = parse_sql(e.sql)
    st = raw.stats
    if e.entry == "distinct":
        model, id_values, dict_path, fstats = want

        def decode(row):
            return tuple(_key_repr(_plain(id_values[j][r])) for j, r in enumerate(row))
        got = [tuple(_key_repr(_plain(v)) for v in r) for r in raw.distinct_rows]
        expect = [decode(r) for r in model.rows]
        assert len(got) == len(set(got)), (what, "duplicate tuples")
        if qc.order_by and model.tied:
            certain = set(expect[:model.n_certain])
            assert len(got) == len(expect) and certain <= set(got) and set(got) - certain <= {decode(t) for t in model.tied}, what
        else:
            assert got == expect, what
        assert st.num_docs_scanned == model.num_docs_scanned, what
        assert st.num_entries_scanned_post_filter == model.num_entries_scanned_post_filter, what
        if dict_path:
            assert st.num_entries_scanned_in_filter == 0, what
        elif not model.early_stop:
            assert st.stats_exact == 1 and st.num_entries_scanned_in_filter == fstats.num_entries_scanned_in_filter, what
    else:
        model, out, cols, fstats = want
        got = raw.selection_rows
        if qc.order_by and qc.limit > 0:
            sm.check_ordered(got, [_order_key(r, qc, out, host) for r in got], model)
        else:
            assert got == model.rows, what
        assert st.num_docs_scanned == model.num_docs_scanned, what
        assert st.num_entries_scanned_post_filter == model.num_entries_scanned_post_filter, what
        if qc.limit == 0:
            assert st.num_entries_scanned_in_filter == 0, what
        elif model.n_next < 0:
            assert st.stats_exact == 1 and st.num_entries_scanned_in_filter == fstats.num_entries_scanned_in_filter, what
    assert st.num_total_docs == host.total_docs, what


def _plain(v):
    return v.item() if isinstance(v, np.generic) else v


def _ids(host, col):
    c = host.columns[col]
    if c.has_dictionary:
        return decode_column(c, host.total_docs, dict_ids=True).astype(np.int64), list(c.dict_values)
    return dm.raw_ids(decode_column(c, host.total_docs))


_DICT_INDEX = {}


def _dict_id(host, col, v):
    key = (id(host), col)
    if key not in _DICT_INDEX:
        _DICT_INDEX[key] = {_plain(x): i for i, x in enumerate(host.columns[col].dict_values)}
    return _DICT_INDEX[key][v]


def _order_key(row, qc, out, host):
    """the ORDER BY key of one selection row, as sm.selection orders: dictIds, or the order-preserving integer of a raw value"""
    key, seen = [], set()
    for text, asc in qc.order_by:
        if text in seen:
            continue
        seen.add(text)
        v = _plain(row[out.index(text)])
        c = host.columns[text]
        if c.has_dictionary:
            o = _dict_id(host, text, v)
        else:
            o = int(sm.order_values(np.array([v], dtype=np.float64 if c.data_type in ("FLOAT", "DOUBLE") else np.int64), None)[0])
        key.append(o if asc else -o)
    return tuple(key)


def run_and_check(segments, e, n):
    """one execution of entry `e` on the segments of size `n`: the kernel it ran, checked against the oracle; returns the comparable answer"""
    host, g, o = segments.get(e.builder, n, e.snapshot)
    what = f"{e.name} @ {n}: {e.sql}"
    kernel, answer, raw = _run(e, host, g)
    assert kernel == e.name, (what, kernel)
    _check(e, n, host, o, raw, what)
    return answer


MATRIX = [pytest.param(e, n, id=f"{e.name}-{n}") for e in ki.ENTRIES for n in e.sizes]


@pytest.mark.parametrize("e,n", MATRIX)
def test_kernel_matches_oracle(segments, gpu_knobs, e, n):
    if e.knobs:
        gpu_knobs(**e.knobs)
    first = run_and_check(segments, e, n)
    second = run_and_check(segments, e, n)   # the cached plan, its observed rates: the same kernel, the same answer
    if e.entry == "filter":
        np.testing.assert_array_equal(first[0], second[0])
    else:
        assert first == second, e.name


def _switch_knobs(gpu_knobs, before, after):
    change = {k: None for k in before if k not in after}
    change.update({k: v for k, v in after.items() if before.get(k) != v})
    if change:
        gpu_knobs(**change)


@pytest.mark.parametrize("n", ki.LADDER)
def test_kernel_families_back_to_back(segments, gpu_knobs, n):
    entries = ki.entries_at(n)
    ran = []
    knobs = {}
    for order in (entries, entries[::-1]):
        for e in order:
            _switch_knobs(gpu_knobs, knobs, e.knobs)
            knobs = dict(e.knobs)
            run_and_check(segments, e, n)
            ran.append(e.name)
    assert sorted(ran) == sorted(2 * [e.name for e in entries])
