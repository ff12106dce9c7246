"""Every side-pass kernel on segments larger than its launch grid: the entries of tests/side_kernel_inventory.py against the per-family models
(variance_model, covariance_model, fourth_moment_model, histogram_model, mode_model, percentile_model, with_time_model, expression_model,
case_model) over the ORACLE's match set and a numpy group assignment, bit for bit as in the families' own modules, with numDocsScanned,
numEntriesScannedPostFilter, numEntriesScannedInFilter, stats_exact and the kernel's name.  One segment per ladder size holds only the
columns its entries need (tests/side_kernel_inventory.py: scale_data).

At 2 047 docs every entry runs without a filter, behind a scan filter and behind an index filter, through its family's _check helper.  The
Fraction models take microseconds per doc, so beyond the wrap points (700 001 and 2 500 003 docs) the match sets have three shapes:

  sparse    s < 16, ~1.6 % of the docs: a doc in the first 64-doc word, one in the last (partial) word and one in at least half of all words
            (asserted on the reference mask before the GPU is asked) — every workgroup takes every step of its walk;
  dense     every doc of ~3 000 docs just past the first grid step of the tier under test, and of the last ~3 000 docs: full match words on
            the second step and in the final partial word, nothing else;
  all       no filter (scan.match == nullptr), for the entries whose reference is exact and vectorised: HISTOGRAM (bin counts), MODE and
            PERCENTILE (np.unique runs), FIRST/LASTWITHTIME (lexicographic arg-min / arg-max by (time, doc)), SUM / MIN / MAX / CASE WHEN of
            INT expressions, and the power-sum families over INT and LONG columns through the models' integer path
            (exact_tuple_of_ints, pinned to the Fraction path by tests/test_model_int_path.py).

DOUBLE / FLOAT arguments of the power-sum families (variance, covariance, SKEWNESS / KURTOSIS) and of the expressions are covered at the
large sizes through the two filtered shapes only.

Reference time per case at 2 500 003 docs — the oracle's filter, the group assignment and the models of all shapes of the case together,
measured on the CPU without a GPU; the slowest case of each family, in seconds: variance 1.1, covariance 2.8 (pg_covar_reg_wide: three
pairs), SKEWNESS / KURTOSIS 3.0 (the fourth powers of 2 500 003 LONGs as Python ints), HISTOGRAM 0.8, PERCENTILE 1.5, MODE 0.5, expressions
0.8, CASE WHEN 0.8, FIRST/LASTWITHTIME 2.0 (the lexicographic sort, and the reference's own loop over the first group).  Building the
2 500 003-doc segment takes 5 s, once per module."""
import time

import numpy as np
import pytest

from pinot_amd import capi
from pinot_amd.executor import NativeSegment, covariance_final, extract_final, variance_final
from pinot_amd.query import parse_sql, with_time_arguments
from tests import covariance_model as cm
from tests import fourth_moment_model as fm
from tests import histogram_model as hm
from tests import kernel_inventory as ki
from tests import mode_model as mm
from tests import percentile_model as pm
from tests import side_kernel_inventory as si
from tests import variance_model as vm
from tests import with_time_model as wm
from tests import test_gpu_case_when as tcw
from tests import test_gpu_covariance as tc
from tests import test_gpu_expressions as te
from tests import test_gpu_histogram as th
from tests import test_gpu_mode as tmo
from tests import test_gpu_moments as tm
from tests import test_gpu_percentile as tp
from tests import test_gpu_variance as tv
from tests import test_gpu_with_time as tw

pytestmark = pytest.mark.gpu

FAMILY_CHECK = {"variance": tv._check, "covariance": tc._check, "moment": tm._check, "histogram": th._check, "percentile": tp._check, "mode": tmo._check,
                "expression": te._check, "case": tcw._check, "with_time": tw._check}
# the helpers that stay cheap on a large segment behind a filter: their models run over the matching docs only (the covariance helper checks
# the window over whole columns and the histogram helper bins every doc, one Python call per doc)
SCALES = ("variance", "moment", "percentile", "mode", "expression", "case", "with_time")
# ... and those whose model is vectorised: they take the unfiltered shape too
VECTORISED = ("percentile", "expression", "case")
INTEGER = ("INT", "LONG")


class Segments:
    """One host segment per size; one GPU and one oracle segment per (size, snapshot)."""

    def __init__(self, gpu_api, oracle_api):
        self.gpu_api, self.oracle_api = gpu_api, oracle_api
        self.hosts, self.pairs = {}, {}

    def get(self, n, snapshot=False):
        if n not in self.hosts:
            self.hosts[n] = si.scale_data(n, si.columns_at(n))
        host, data, schema = self.hosts[n]
        if (n, snapshot) not in self.pairs:
            g, o = NativeSegment(self.gpu_api, host), NativeSegment(self.oracle_api, host)
            if snapshot:
                keep = ki.snapshot_doc_ids(n)
                g.set_queryable_doc_ids(keep)
                o.set_queryable_doc_ids(keep)
            self.pairs[(n, snapshot)] = (g, o)
        g, o = self.pairs[(n, snapshot)]
        return host, data, schema, g, o

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
    """entry -> the wrap point of its tier on THIS device; a device with more compute units than the inventory assumed must still be exceeded"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    c = si.launch_constants()
    points = {}
    for i, e in enumerate(si.ENTRIES):
        points[i] = si.wrap_point(e, cus, c)
        if cus > si.ASSUMED_CUS:
            assert max(e.sizes) - points[i] >= 64 * 64, (f"{cus} compute units: the pass of {e.name} ({e.select}) wraps at {points[i]} docs, "
                                                         f"which the ladder's {max(e.sizes)} no longer exceeds")
        else:
            assert points[i] <= si.wrap_point(e, si.ASSUMED_CUS, c)
    return points


def _norm(key):
    return tuple(float(k) if isinstance(k, (int, float, np.integer, np.floating)) else k for k in key)


def _mask(n, docs):
    m = np.zeros((n + 63) // 64 * 64, dtype=bool)
    m[np.asarray(docs, dtype=np.int64)] = True
    return m.reshape(-1, 64)


def _assert_sparse_and_spread(n, docs):
    words = _mask(n, docs)
    assert words[0].any(), "no matching doc in the first 64-doc word"
    assert words[-1].any() and n % 64 != 0, "no matching doc in the last, partial word"
    assert words.any(axis=1).sum() * 2 >= len(words), "fewer than half of the match words hold a doc"
    assert len(docs) < n // 40, "the sparse shape is no longer sparse"


def _assert_dense_at_the_wrap_and_the_tail(n, docs, wrap, snapshot):
    words = _mask(n, docs)
    tail = words[-1][: n % 64]
    full = (lambda w: w.mean() > 0.6) if snapshot else (lambda w: w.all())   # the snapshot drops a tenth of the docs
    assert full(tail) and full(words[-40:-1]), "the tail's match words are not full"
    if 0 < wrap < n - 6200:
        assert full(words[wrap // 64: wrap // 64 + 40]), "no full match words on the second grid step"
        assert not words[: wrap // 64].any() and not words[wrap // 64 + 60: -60].any(), "docs outside the two stretches"
    assert len(docs) <= 6200


# ---- vectorised references of the unfiltered shape ------------------------------------------------------------------------------------------------
def _vector_bins(spec, d):
    """hm.bin_of over a float64 array (no NaN): the same IEEE operations, one numpy call each"""
    d = np.asarray(d, dtype=np.float64)
    assert not np.isnan(d).any()
    if spec.kind == "equal":
        with np.errstate(all="ignore"):
            b = np.floor((d - np.float64(spec.lower)) / np.float64(spec.bin_length))
        b = np.where(np.isnan(b), 0.0, b)
        b = np.where(b >= spec.n_bins, float(hm.THROWS_INDEX), b)
    else:
        b = (np.searchsorted(np.asarray(spec.edges, dtype=np.float64), d, side="right") - 1).astype(np.float64)
    b = np.where(d == spec.upper, float(spec.n_bins - 1), b)
    b = np.where((d > spec.upper) | (d < spec.lower), float(hm.NONE), b)
    return b.astype(np.int64)


def _doubles(data, schema, col, docs):
    return pm.as_doubles(np.asarray(data[col])[docs], schema[col])


def _vector_map(values, data_type):
    """mm.value_map through np.unique: the keys in Double.compare / Long.compare order, every NaN one key"""
    if data_type in INTEGER:
        keys, counts = np.unique(np.asarray(values, dtype=np.int64), return_counts=True)
        entries = tuple((int(k), int(c)) for k, c in zip(keys, counts))
    else:
        d = pm.as_doubles(values, data_type)
        _, first, counts = np.unique(pm.order_keys(d), return_index=True, return_counts=True)
        entries = tuple((float(d[i]), int(c)) for i, c in zip(first, counts))
    return (data_type, entries) if entries else ("INT", ())


def _vector_winners(function, times, code, docs):
    """per group the doc the reference's docId-order loop ends on: LAST `time >= best`, FIRST `time <= best` — the greatest doc among those of
    the extreme time either way"""
    t = np.asarray(times, dtype=np.int64)[docs]
    if function == "LASTWITHTIME":
        order = np.lexsort((docs, t, code))          # by group, then time, then doc: a group's last row wins
        ends = np.flatnonzero(np.concatenate((code[order][1:] != code[order][:-1], [True])))
        return docs[order][ends]
    order = np.lexsort((-docs, t, code))             # by group, then time, then doc descending: a group's first row wins
    starts = np.flatnonzero(np.concatenate(([True], code[order][1:] != code[order][:-1])))
    return docs[order][starts]


def _own_check(seg, e, where, kernel):
    """the family helpers' check restated for large match sets: the same assertions, the per-group reference from the models' vectorised or
    integer paths where the match set is large, from their Fraction / per-doc paths over the matching docs otherwise"""
    host, data, schema, gpu, oracle = seg
    sql = e.sql(where)
    qc = parse_sql(sql)
    docs, in_filter = tv._filter(oracle, sql)
    docs = np.sort(np.asarray(docs, dtype=np.int64))
    large = len(docs) > 100_000
    b = gpu.execute(qc)
    rows = {_norm(k): v for k, v in b.rows().items()}
    finals = None
    if e.family == "mode":
        qf = parse_sql(sql)
        qf.flags |= capi.QUERY_FLAG_FINAL_MODE
        f = gpu.execute(qf)
        finals = {_norm(k): v for k, v in f.rows().items()}
        assert f.stats.kernel.decode() == kernel and f.stats.num_docs_scanned == len(docs), sql
    # the group assignment: one code per matching doc, the groups in order of their codes
    code = np.zeros(len(docs), dtype=np.int64)
    cols = [np.asarray(data[g])[docs] for g in e.group_by]
    for c in cols:
        values, inverse = np.unique(c, return_inverse=True)
        code = code * len(values) + inverse
    _, first, code = np.unique(code, return_index=True, return_inverse=True)
    keys = [_norm(tuple(c[i].item() for c in cols)) for i in first]
    n_groups = len(keys)
    assert set(rows) == set(keys) and len(rows) == n_groups, sql
    read = set(e.group_by) | set(e.reads)
    assert (b.stats.num_docs_scanned, b.stats.num_entries_scanned_post_filter) == pm.statistics(len(docs), read), sql
    assert b.stats.num_entries_scanned_in_filter == in_filter and b.stats.stats_exact == 1 and b.stats.num_total_docs == host.total_docs, sql
    assert b.stats.star_tree_index == -1 and b.stats.kernel.decode() == kernel, (sql, b.stats.kernel)
    order = np.argsort(code, kind="stable")
    bounds = np.concatenate(([0], np.cumsum(np.bincount(code, minlength=n_groups))))
    members = [docs[order[bounds[g]:bounds[g + 1]]] for g in range(n_groups)]      # ascending docs of every group
    for a, spec in enumerate(qc.aggregations):
        got = [rows[k][a] for k in keys]
        if spec.function == "COUNT":
            assert got == [len(m) for m in members], sql
        elif e.family in ("variance", "moment"):
            model, same = (vm, tv._same_tuple) if e.family == "variance" else (fm, fm.same_tuple)
            if spec.function not in model.FUNCTIONS:
                continue
            t = schema[spec.column]
            assert t in INTEGER or not large, "a DOUBLE / FLOAT argument over a large match set: the Fraction model would take minutes"
            v = np.asarray(data[spec.column])
            for g, m in enumerate(members):
                want = model.exact_tuple_of_ints(v[m], t) if large else model.exact_tuple(model.as_doubles(v[m], t))
                assert same(got[g], want), (sql, keys[g], spec, got[g], want)
                if e.family == "variance":
                    assert vm.same_bits(variance_final(spec.function, got[g]), vm.final(spec.function, want)), (sql, keys[g], spec)
        elif e.family == "covariance":
            if spec.function not in cm.FUNCTIONS:
                continue
            x, y = spec.column.split(",")
            tx, ty = schema[x], schema[y]
            assert (tx in INTEGER and ty in INTEGER) or not large, "a DOUBLE / FLOAT argument over a large match set"
            vx, vy = np.asarray(data[x]), np.asarray(data[y])
            if not large:   # the matching docs lie inside the documented window: the model alone decides the expected bits
                assert cm.in_exact_window(cm.as_doubles(vx[docs], tx), cm.as_doubles(vy[docs], ty), tx, ty, tc.K), (x, y)
            for g, m in enumerate(members):
                want = cm.exact_tuple_of_ints(vx[m], tx, vy[m], ty) if large else cm.exact_tuple(cm.as_doubles(vx[m], tx), cm.as_doubles(vy[m], ty))
                assert tc._same_tuple(got[g], want), (sql, keys[g], spec, got[g], want)
                assert cm.same_bits(covariance_final(spec.function, got[g]), cm.final(spec.function, want)), (sql, keys[g], spec)
        elif e.family == "histogram":
            if spec.function != "HISTOGRAM":
                continue
            x, hs = hm.parse_arguments(spec.column)
            d = _doubles(data, schema, x, docs)
            bins = _vector_bins(hs, d)
            probe = np.concatenate((np.arange(min(len(d), 1500)), np.arange(max(0, len(d) - 500), len(d))))   # the vectorised bins are the model's
            assert [hm.bin_of(hs, d[i]) for i in probe] == bins[probe].tolist(), spec.column
            assert (bins >= hm.NONE).all(), "the reference throws on this input"
            inside = bins >= 0
            counts = np.bincount(code[inside] * hs.n_bins + bins[inside], minlength=n_groups * hs.n_bins).reshape(n_groups, hs.n_bins)
            for g in range(n_groups):
                want = tuple(float(c) for c in counts[g])
                assert isinstance(got[g], tuple) and got[g] == want, (sql, keys[g], spec.column[:60], got[g][:12], want[:12])
        elif e.family == "mode":
            if spec.function != "MODE":
                continue
            col, reducer = tmo._column_of(spec), tmo._reducer_of(spec)
            v = np.asarray(data[col])
            for g, m in enumerate(members):
                want = _vector_map(v[m], schema[col])
                if g == 0:   # np.unique's map is the model's
                    assert mm.same_map(_vector_map(v[m][:3000], schema[col]), mm.value_map(v[m][:3000], schema[col]))
                assert mm.same_map(got[g], want), (sql, keys[g], spec.column, got[g][1][:6], want[1][:6])
                want_final = mm.final(want, reducer)
                assert mm.same_double(finals[keys[g]][a], want_final), (sql, keys[g], spec.column, finals[keys[g]][a], want_final)
                assert mm.same_double(extract_final("MODE", got[g], spec.column), want_final)
        elif e.family == "with_time":
            if spec.function not in wm.FUNCTIONS:
                continue
            x, t, declared = with_time_arguments(spec.column)
            winners = _vector_winners(spec.function, data[t], code[order], docs[order])
            for g, m in enumerate(members):
                doc = int(winners[g])
                if g == 0:   # the lexicographic arg-max is the reference's docId-order loop
                    assert wm.winner(spec.function, data[t], m) == doc, (sql, keys[g], spec)
                want = (wm.convert(schema[x], data[x][doc], declared), int(data[t][doc]))
                assert wm.pair_bits(declared, *got[g]) == want, (sql, keys[g], spec, got[g], want, doc)
        else:
            raise AssertionError(e.family)
    return b


def _shapes(e, n, wrap):
    """(name, WHERE) of the match-set shapes of an entry at `n` docs"""
    if n == si.SMALL:
        return [("all", "")] + [("filter%d" % i, w) for i, w in enumerate(si.SMALL_FILTERS)]
    shapes = [("sparse", si.SPARSE), ("dense", si.dense_filter(n, wrap))]
    return shapes + ([("all", "")] if e.unfiltered else [])


def _check_shape(seg, e, n, shape, where, wrap):
    host, data, schema, gpu, oracle = seg
    if shape in ("sparse", "dense"):   # the conditions on the reference mask, before the GPU is asked
        docs, _ = tv._filter(oracle, e.sql(where))
        if shape == "sparse":
            _assert_sparse_and_spread(n, docs)
        else:
            _assert_dense_at_the_wrap_and_the_tail(n, docs, wrap, e.snapshot)
    if n == si.SMALL or e.family in VECTORISED or (shape != "all" and e.family in SCALES):
        return FAMILY_CHECK[e.family](seg, e.sql(where), kernel=e.kernel_at(n))
    return _own_check(seg, e, where, e.kernel_at(n))


CASES = [pytest.param(i, n, id=f"{e.name}-{e.family}{'-snapshot' if e.snapshot else ''}-{i}-{n}") for i, e in enumerate(si.ENTRIES) for n in e.sizes]


@pytest.mark.parametrize("index, n", CASES)
def test_side_kernel_at_scale(segments, wraps, gpu_knobs, index, n):
    e = si.ENTRIES[index]
    wrap = wraps[index]
    assert n == si.SMALL or n > wrap or n < max(e.sizes)
    if e.knobs:
        gpu_knobs(**e.knobs)
    seg = segments.get(n, e.snapshot)
    for shape, where in _shapes(e, n, wrap):
        t0 = time.time()
        b = _check_shape(seg, e, n, shape, where, wrap)
        print(f"{e.name} {e.family} n={n} {shape}: {b.stats.num_docs_scanned} docs, {time.time() - t0:.2f} s with its reference")
        if e.snapshot and shape == "all":
            assert b.stats.num_docs_scanned == len(ki.snapshot_doc_ids(n))


def test_the_packed_bound_moves_with_the_doc_count(segments):
    """tm's range is packed beside the docId on the small segment and takes the two-pass route on the largest: the wide mode reads the match
    words and the time column twice, which the pass's bytes show"""
    bits = {}
    for n in (si.SMALL, si.BIG):
        host, data, schema, gpu, oracle = segments.get(n)
        assert wm.packed_ok(si.TIME_RANGE["tm"][1] - si.TIME_RANGE["tm"][0], wm.doc_bits(n)) == (n == si.SMALL)
        assert wm.packed_ok(si.TIME_RANGE["tp"][1] - si.TIME_RANGE["tp"][0], wm.doc_bits(n))
        for t in ("tp", "tm"):
            assert (int(data[t].min()), int(data[t].max())) == si.TIME_RANGE[t]
            with_t = gpu.execute(f"SELECT LASTWITHTIME(ri, {t}, 'INT') FROM t WHERE s < 900").stats.algorithmic_bytes
            plain = gpu.execute("SELECT COUNT(*) FROM t WHERE s < 900").stats.algorithmic_bytes
            bits[(n, t)] = (with_t - plain) / ((n * 64 + 7) // 8 + (n + 63) // 64 * 8)   # one read of a raw LONG column and of the match words
    print(bits)
    for key, passes in (((si.SMALL, "tp"), 1), ((si.SMALL, "tm"), 1), ((si.BIG, "tp"), 1), ((si.BIG, "tm"), 2)):   # (+ the few gathered bytes)
        assert bits[key] == pytest.approx(passes, abs=0.01), (key, bits)
