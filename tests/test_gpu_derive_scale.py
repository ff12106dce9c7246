"""The three derive passes on segments larger than their launch grid: the entries of tests/derive_pass_inventory.py — pg_expr_pred (the match
words of an arithmetic predicate), pg_expr_keys and pg_time_keys (one key per doc of an expression / time-bucket GROUP BY key, from which
vdict_from_keys makes the bit-packed ids and the distinct-key table every later query over that text reads) — bit for bit against the models:
integers equal, doubles by percentile_model.same_double, no tolerances.  One segment per size (2 047 and 2 500 003 docs), built once per
module; the `wraps` fixture recomputes the wrap point for the compute units of the device at hand.

  pg_expr_pred   SELECT band, COUNT(*), SUM(pos), MIN(pos), MAX(pos) ... WHERE <predicate> GROUP BY band, with pos the docId and band =
                 doc / 65 536: count, sum (below 2^53), first and last doc of each of the 39 bands pin which docs matched.  Reference:
                 expression_model.evaluate + expression_filter_model.apply_predicate, folded per band with numpy.  Every predicate kind and
                 operand kind, 1 / 2 / 3 / 8 operand columns; one leaf ANDed with an index leaf, one ORed with a scan, one under NOT, one
                 behind the upsert snapshot, one through pg_filter_exec (docIds and words).  numDocsScanned and stats_exact everywhere;
                 numEntriesScannedInFilter where the leaf stands alone: the doc count, as a drained ExpressionScanDocIdIterator counts every
                 block once — the iterator model (2 to 5 us per returned doc) confirms it for the leaf that matches less than 15 % of the docs
                 (EQ: 227 000).  The entry counts of the combined shapes stay with tests/test_gpu_expression_filters.py (30 011 docs): the model's
                 leapfrog takes 5 s and more per case here.
  pg_expr_keys   moderate keys over every doc against their twin raw DOUBLE column on the oracle (test_gpu_expression_keys._check); 17-bit
                 and 22-bit ids (65 537 and 2^21 + 1 distinct keys, numGroupsLimit above the key space) behind the sparse and the dense
                 filter of tests/side_kernel_inventory.py and under SELECT DISTINCT, against expression_model.evaluate over the matching
                 docs and np.unique.
  pg_time_keys   one text per time_load kind and per family over every doc, against time_transform_model.evaluate over the DISTINCT source
                 values (at most 20 000) mapped back, np.unique counts and integer sums; one key per doc (22-bit ids) behind the two filters,
                 the model over the matching docs only.

At 2 047 docs every entry also runs through the three families' own helpers (_check_filter / _check_stats, _check, _check) against twin
columns on the oracle.

Reference time per case at 2 500 003 docs, measured on the CPU without a GPU (the masks, the models, the folds, the oracle's filter and its
twin query), the slowest case of each pass in seconds: pg_expr_pred 1.2 (EQ alone: the iterator model; 0.4 without it), pg_expr_keys 1.3
(mult(hk2,'3') over every doc: the sort of 2 500 003 keys), pg_time_keys 1.2 (datetrunc('week',ts): np.unique of the source and of the keys).
Building the 2 500 003-doc segment takes 2 to 4 s, once per module."""
import time

import numpy as np
import pytest

from pinot_amd.executor import NativeSegment
from pinot_amd.query import parse_sql
from tests import derive_pass_inventory as di
from tests import expression_filter_model as fm
from tests import kernel_inventory as ki
from tests import percentile_model as pm
from tests import test_gpu_expression_filters as tef
from tests import test_gpu_expression_keys as tek
from tests import test_gpu_time_keys as tgt
from tests import test_gpu_variance as tv

pytestmark = pytest.mark.gpu
MODEL_MAX_SELECTIVITY = 0.15     # the iterator model runs where the leaf matches at most this share of the docs


class Segments:
    """One host segment per size; one GPU and one oracle segment per (size, snapshot)."""

    def __init__(self, gpu_api, oracle_api):
        self.gpu_api, self.oracle_api = gpu_api, oracle_api
        self.hosts, self.pairs = {}, {}

    def get(self, n, wrap, snapshot=False):
        if n not in self.hosts:
            t0 = time.time()
            self.hosts[n] = di.scale_data(n, wrap)
            print(f"segment of {n} docs: {time.time() - t0:.1f} s")
        host, data, schema, twins = self.hosts[n]
        if (n, snapshot) not in self.pairs:
            g, o = NativeSegment(self.gpu_api, host), NativeSegment(self.oracle_api, host)
            if snapshot:
                keep = ki.snapshot_doc_ids(n)
                g.set_queryable_doc_ids(keep)
                o.set_queryable_doc_ids(keep)
            self.pairs[(n, snapshot)] = (g, o)
        g, o = self.pairs[(n, snapshot)]
        return host, data, schema, twins, g, o

    def destroy(self):
        for g, o in self.pairs.values():
            g.destroy()
            o.destroy()
        self.pairs.clear()
        self.hosts.clear()


@pytest.fixture(scope="module")
def segments(gpu_api, oracle_api):
    s = Segments(gpu_api, oracle_api)
    yield s
    s.destroy()


@pytest.fixture(scope="module")
def wraps(gpu_api):
    """pass -> its wrap point on THIS device; the largest size must exceed it by a full round of words for a workgroup, whatever the device"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    c = di.launch_constants()
    points = {p: di.wrap_point(cus, c, p) for p in di.PASSES}
    for p, wrap in points.items():
        assert di.BIG - wrap >= 64 * 64, f"{cus} compute units: {p} wraps at {wrap} docs, which the ladder's {di.BIG} no longer exceeds by {64 * 64}"
    return points


# ---- the conditions on the reference mask, before the GPU is asked ------------------------------------------------------------------------------------
def _words(n, mask):
    m = np.zeros((n + 63) // 64 * 64, dtype=bool)
    m[:n] = mask
    return m.reshape(-1, 64)


def _assert_the_wrap_band_and_the_last_band_match(n, mask, wrap):
    band = np.arange(n) // di.BAND_DOCS
    assert wrap < n and band[wrap] < band[n - 1] and n % di.BAND_DOCS != 0
    assert mask[band == band[wrap]].any(), "no match in the band that holds the wrap point"
    assert mask[band == band[n - 1]].any(), "no match in the last, partial band"
    assert mask[wrap:].any() and mask[:wrap].any()


def _assert_sparse_and_spread(n, mask, wrap):
    words = _words(n, mask)
    assert words[0].any(), "no matching doc in the first 64-doc word"
    assert words[-1].any() and n % 64 != 0, "no matching doc in the last, partial word"
    assert words.any(axis=1).sum() * 2 >= len(words), "fewer than half of the match words hold a doc"
    assert mask[:wrap].any() and mask[wrap:].any() and mask.sum() < n // 40, "the sparse shape is no longer sparse, or stops at the wrap"


def _assert_dense_on_both_sides_of_the_wrap_and_at_the_tail(n, mask, wrap):
    words = _words(n, mask)
    at, full = wrap // 64, di.DENSE_BACK // 64
    assert words[-1][: n % 64].all() and n % 64 != 0 and words[-40:-1].all(), "the tail's match words are not full"
    assert words[at - full: at + full].all(), "no full match words on both sides of the wrap point"
    assert not words[: at - full - 1].any() and not words[at + full + 1: -60].any(), "docs outside the two stretches"
    assert mask.sum() <= 6200


# ---- pg_expr_pred ------------------------------------------------------------------------------------------------------------------------------------------
def _check_predicate(seg, e, shape, n, wrap):
    host, data, schema, twins, gpu, oracle = seg
    where = e.where(shape, n, wrap)
    keep = ki.snapshot_doc_ids(n) if shape == "snapshot" else None
    mask = di.where_mask(where, data, schema, keep)
    docs = np.flatnonzero(mask)
    leaf = di.where_mask(e.text, data, schema)
    assert di.SELECTIVITY[0] <= leaf.mean() <= di.SELECTIVITY[1], (e.text, leaf.mean())
    if n > wrap:
        _assert_the_wrap_band_and_the_last_band_match(n, mask, wrap)
    alone = shape in ("lone", "not", "filter")
    if alone and leaf.mean() <= MODEL_MAX_SELECTIVITY:      # the iterator model, where it is cheap: every block once, whatever matches
        tree = ("not", ("expr", leaf)) if shape == "not" else ("expr", leaf)
        entries, model_docs = fm.entries_scanned_in_filter(tree, n)
        assert entries == n and np.array_equal(model_docs, docs)
    sql = e.sql(shape, n, wrap)
    if shape == "filter":                                    # pg_filter_exec: the docIds and the words themselves
        ds = gpu.filter(sql)
        got, words, card, st = ds.doc_ids(), ds.words(), ds.cardinality(), ds.stats()
        ds.free()
        assert card == len(docs) and np.array_equal(got, docs), (sql, card, len(docs))
        bits = np.unpackbits(np.asarray(words, dtype="<u8").view(np.uint8), bitorder="little")
        assert np.array_equal(np.flatnonzero(bits), docs) and not bits[n:].any(), sql
        assert (st.num_entries_scanned_in_filter, st.stats_exact) == (n, 1), sql
        b = gpu.execute(sql)
        assert b.aggregation_result() == [len(docs)], sql
    else:
        want = di.fold_bands(mask, data)
        b = gpu.execute(sql)
        rows = b.rows()
        assert set(rows) == set(want), (sql, sorted(set(rows) ^ set(want)))
        for key, w in want.items():
            r = rows[key]
            assert r[0] == w[0] and all(pm.same_double(x, y) for x, y in zip(r[1:], w[1:])), (sql, key, r, w)
        assert b.stats.num_entries_scanned_post_filter == len(docs) * 2, sql       # band and pos; the filter's operands do not count there
    assert b.stats.num_docs_scanned == len(docs) and b.stats.stats_exact == 1 and b.stats.num_total_docs == n, sql
    assert b.stats.star_tree_index == -1
    if alone:
        assert b.stats.num_entries_scanned_in_filter == n, (sql, b.stats.num_entries_scanned_in_filter)
    return b


def _small_predicate(seg, e, shape, n, wrap):
    """the family's own helpers at 2 047 docs: the doc set against the model and the twin through the oracle, the statistics against the
    iterator model"""
    data, schema = seg[1], seg[2]
    where = e.where(shape, n, wrap)
    tef._check_filter(seg, where)
    leaf = di.where_mask(e.text, data, schema)
    if shape in ("lone", "filter"):
        assert tef._check_stats(seg, where, ("expr", leaf)) == n
    elif shape == "not":
        assert tef._check_stats(seg, where, ("not", ("expr", leaf))) == n
    elif shape == "and":
        inv = di.where_mask(di.AND_WITH, data, schema)
        assert tef._check_stats(seg, where, ("and", [("index", inv), ("expr", leaf)])) == int(inv.sum())


# ---- the key passes --------------------------------------------------------------------------------------------------------------------------------------
def _keys_of(e, data, schema, docs):
    """(one int64 key per doc of `docs` — Double.doubleToLongBits or the LONG itself —, the weights its SUM adds, the columns the query reads)"""
    text = e.expression()
    if e.kernel == "pg_time_keys":
        return di.time_keys(text, data, docs), np.asarray(data["s"])[docs], set(e.sources()) | {"s"}
    v = di.evaluate(text, data, schema, docs)
    assert not np.isnan(v).any()
    return di.double_bits(v), np.asarray(data["pos"])[docs], set(e.sources()) | {"pos"}


def _check_keys(seg, e, shape, n, wrap):
    """GROUP BY <key> (or SELECT DISTINCT) against the model over the matching docs"""
    host, data, schema, twins, gpu, oracle = seg
    sql = e.sql(shape, n, wrap)
    where = e.where(shape, n, wrap)
    mask = di.where_mask(where, data, schema)
    docs = np.flatnonzero(mask)
    in_filter = 0
    if where:
        odocs, in_filter = tv._filter(oracle, sql)
        assert np.array_equal(np.sort(odocs), docs), sql           # the two sources agree
    if n > wrap and shape == "sparse":
        _assert_sparse_and_spread(n, mask, wrap)
    if n > wrap and shape == "dense":
        _assert_dense_on_both_sides_of_the_wrap_and_at_the_tail(n, mask, wrap)
    keys, weights, read = _keys_of(e, data, schema, docs)
    qc = parse_sql(sql)
    if e.groups_limit:
        qc.num_groups_limit = e.groups_limit
    b = gpu.execute(qc)
    floating = e.kernel == "pg_expr_keys"
    got = b.group_value_columns[0]
    assert got.dtype == (np.float64 if floating else np.int64), (sql, got.dtype)
    got = di.double_bits(got) if floating else got
    if shape == "distinct":
        values = np.sort(np.unique(keys).view(np.float64))[::-1][:qc.limit]
        assert np.array_equal(got, di.double_bits(values)), sql
        assert b.distinct_rows[:3] == [(float(v),) for v in values[:3]] and len(b.distinct_rows) == len(values)
        read = set(e.sources())
    else:
        u, counts, sums = di.fold_keys(keys, weights)
        order = np.argsort(got, kind="stable")
        assert len(got) == len(u) and np.array_equal(got[order], u), (sql, len(got), len(u))
        assert np.array_equal(b.arrays[0][1][order], counts), sql
        assert di.same_doubles(b.arrays[1][1][order], sums.astype(np.float64)), sql
        assert b.stats.num_groups_limit_reached == 0, sql
    assert (b.stats.num_docs_scanned, b.stats.num_entries_scanned_post_filter) == pm.statistics(len(docs), read), sql
    assert b.stats.num_entries_scanned_in_filter == in_filter and b.stats.stats_exact == 1 and b.stats.num_total_docs == n, sql
    assert b.stats.star_tree_index == -1
    return b


def _check_shape(seg, e, shape, n, wrap):
    if e.kernel == "pg_expr_pred":
        if n == di.SMALL and shape != "snapshot":
            _small_predicate(seg, e, shape, n, wrap)
        return _check_predicate(seg, e, shape, n, wrap)
    family = tek if e.kernel == "pg_expr_keys" else tgt
    params = {"num_groups_limit": e.groups_limit} if e.groups_limit else {}
    if shape == "distinct":
        return _check_keys(seg, e, shape, n, wrap)
    if n == di.SMALL:
        family._check(seg, e.sql(shape, n, wrap), **params)
        return _check_keys(seg, e, shape, n, wrap)
    if e.twin:                                                     # every doc, against the twin column on the oracle
        b, _ = family._check(seg, e.sql(shape, n, wrap), **params)
        return b
    return _check_keys(seg, e, shape, n, wrap)


CASES = [pytest.param(i, n, shape, id=f"{e.kernel}-{i}-{shape}-{n}") for i, e in enumerate(di.ENTRIES) for n in e.sizes for shape in e.shapes]


@pytest.mark.parametrize("index, n, shape", CASES)
def test_derive_pass_at_scale(segments, wraps, index, n, shape):
    e = di.ENTRIES[index]
    wrap = wraps[e.kernel]
    seg = segments.get(n, wrap, snapshot=shape == "snapshot")
    t0 = time.time()
    b = _check_shape(seg, e, shape, n, wrap)
    print(f"{e.kernel} {e.text} n={n} {shape}: {b.stats.num_docs_scanned} docs, {time.time() - t0:.2f} s with its reference")
