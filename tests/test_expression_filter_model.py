"""tests/expression_filter_model.py held to the reference: the row counts of NullHandlingEnabledQueriesTest's expression filter cases
(tests/golden/expression_filter_expected.json), the IN rule of DoubleOpenHashSet, "Invalid range", and the block arithmetic of
ExpressionScanDocIdIterator worked out by hand from the Java."""
import json
import math
import os

import numpy as np
import pytest

from pinot_amd.query import parse_sql
from tests import expression_filter_model as fm
from tests import expression_model as em

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPECTED = json.load(open(os.path.join(ROOT, "tests", "golden", "expression_filter_expected.json")))


def _leaf(filter_ctx):
    return filter_ctx.children[0] if filter_ctx.type == "NOT" else filter_ctx


def _run(case, data):
    qc = parse_sql(case["sql"])
    p = _leaf(qc.filter).predicate
    mask = fm.apply_predicate(em.evaluate(p.column, data, {k: "INT" for k in data}), p)
    tree = ("expr", mask)
    if qc.filter.type == "NOT":
        tree = ("not", tree)
    return qc, fm.entries_scanned_in_filter(tree, len(mask), qc.limit if qc.selection else -1)


@pytest.mark.parametrize("name", ["addition", "addition_inside_not"])
def test_addition_goldens(name):
    case = EXPECTED[name]
    rows = np.array([case["null_replacement"] if v is None else v for v in case["rows"]], dtype=np.int32)
    qc, (entries, docs) = _run(case, {"column1": rows})
    assert _leaf(qc.filter).predicate.column == "add(column1,'0')"
    assert len(docs) == case["rows_per_segment"]
    assert sorted(int(rows[d]) for d in docs) == [-2147483648, -1]
    assert entries == case["num_entries_scanned_in_filter"] == len(rows)


def test_second_projection_block_golden():
    case = EXPECTED["second_block"]
    n = case["null_rows"]
    assert n == fm.MAX_DOC_PER_CALL
    c1 = np.full(n + 1, case["null_replacement"], dtype=np.int32)
    c2 = np.arange(n + 1, dtype=np.int32)
    c1[n], c2[n] = case["last_row"]
    qc, (entries, docs) = _run(case, {"column1": c1, "column2": c2})
    assert qc.limit == 10 and len(docs) == case["rows_per_segment"]
    assert [int(c1[docs[0]]), int(c2[docs[0]])] == case["row"]
    assert entries == case["num_entries_scanned_in_filter"]   # two blocks evaluated: 10 000 docs and 1 doc


def test_in_compares_bit_patterns_and_eq_compares_numbers():
    v = np.array([0.0, -0.0, math.nan, 1.5, math.inf, -math.inf])
    assert fm.apply_eq(v, "0").tolist() == [True, True, False, False, False, False]
    assert fm.apply_not_eq(v, "0").tolist() == [False, False, True, True, True, True]
    assert fm.apply_in(v, ["0"]).tolist() == [True, False, False, False, False, False]
    assert fm.apply_in(v, ["-0.0", "1.5"]).tolist() == [False, True, False, True, False, False]
    assert fm.apply_not_in(v, ["0"]).tolist() == [False, True, True, True, True, True]
    assert fm.apply_in(v, ["NaN"]).tolist() == [False, False, True, False, False, False]
    assert fm.apply_eq(v, "NaN").tolist() == [False] * 6
    other_nan = np.array([0x7FF0000000000001], dtype=np.uint64).view(np.float64)   # any NaN is the one NaN of doubleToLongBits
    assert fm.apply_in(other_nan, ["NaN"]).tolist() == [True]


def test_range_bounds():
    v = np.array([1.0, math.nextafter(1.0, 2.0), 2.0, math.nan, math.inf, -math.inf])
    assert fm.apply_range(v, "1", "2", False, True).tolist() == [False, True, True, False, False, False]
    assert fm.apply_range(v, "1", "2", True, False).tolist() == [True, True, False, False, False, False]
    assert fm.apply_range(v, "1", "*", False, False).tolist() == [False, True, True, False, True, False]
    assert fm.apply_range(v, "*", "Infinity", False, True).tolist() == [True, True, True, False, True, True]
    for lower, upper, li, ui in (("Infinity", "*", False, False), ("*", "-Infinity", False, False), ("NaN", "*", False, False)):
        with pytest.raises(fm.InvalidRange):
            fm.range_bounds(lower, upper, li, ui)
    fm.range_bounds("Infinity", "*", True, False)   # an inclusive bound at infinity is a range (an empty one)


def _mask(n, docs):
    m = np.zeros(n, dtype=bool)
    m[list(docs)] = True
    return m


def test_lone_leaf_counts_every_doc_once():
    for n in (1, 65, 10000, 10001, 30011):
        for docs in ((), (0,), (n - 1,), (0, n - 1)):
            entries, got = fm.entries_scanned_in_filter(("expr", _mask(n, docs)), n)
            assert (entries, got) == (n, sorted(set(docs)))
            entries, got = fm.entries_scanned_in_filter(("not", ("expr", _mask(n, docs))), n)
            assert entries == n and len(got) == n - len(set(docs))


def test_and_with_an_index_is_apply_and():
    n = 30011
    index = _mask(n, range(0, n, 7))
    leaf = _mask(n, range(0, n, 3))
    entries, got = fm.entries_scanned_in_filter(("and", [("expr", leaf), ("index", index)]), n)
    assert entries == int(index.sum()) and got == list(range(0, n, 21))
    # a scan between them is applied first (priority 500 before 1000): the leaf sees the scan's survivors only
    scan = _mask(n, range(0, n, 2))
    entries, got = fm.entries_scanned_in_filter(("and", [("expr", leaf), ("scan", scan), ("index", index)]), n)
    assert entries == int(index.sum()) + int((index & scan).sum()) and got == list(range(0, n, 42))


def test_leapfrog_with_a_scan_by_hand():
    """AND(scan {5, 25000}, leaf {25000}) over 30 011 docs, no index: AndDocIdIterator over [scan, leaf].
    scan.advance(0) reads docs 0..5 (6) -> 5; leaf.advance(5): _blockEndDocId = 5, blocks [5, 10005), [10005, 20005), [20005, 30005) are
    evaluated (30 000) -> 25000; scan.advance(25000) reads 1 doc -> 25000: a match.  Then scan.advance(25001) reads the last 5 010 docs -> EOF."""
    n = 30011
    entries, got = fm.entries_scanned_in_filter(("and", [("expr", _mask(n, [25000])), ("scan", _mask(n, [5, 25000]))]), n)
    assert got == [25000] and entries == 6 + 30000 + 1 + 5010


def test_advance_inside_the_current_block_costs_nothing():
    """AND(scan {100, 200, 20000}, leaf {150, 200, 20000}) over 20 001 docs.  scan.advance(0): 101 docs -> 100; leaf.advance(100): block
    [100, 10100) (10 000) -> 150; scan.advance(150): 51 docs -> 200; leaf.advance(200): inside the block, free -> 200: a match.
    scan.advance(201): 19 800 docs -> 20000; leaf.advance(20000): beyond the block, _blockEndDocId = 20000, block [20000, 20001) (1) -> 20000:
    a match.  scan.advance(20001): nothing left."""
    n = 20001
    entries, got = fm.entries_scanned_in_filter(("and", [("scan", _mask(n, [100, 200, 20000])), ("expr", _mask(n, [150, 200, 20000]))]), n)
    assert got == [200, 20000] and entries == (101 + 51 + 19800) + (10000 + 1)


def test_not_over_the_leaf_is_an_expression_iterator_over_the_rejected_docs():
    """ExpressionFilterOperator#getFalses is a second ExpressionDocIdSet (PredicateEvaluationResult.FALSE), not NotDocIdSet(trues).
    Over 30 011 docs, a leaf that holds everywhere but at doc 25000, so NOT(leaf) = {25000}:
      AND(index {0, 10, .., 30010}, NOT(leaf)): applyAnd evaluates the index's 3 002 docs, nothing else;
      AND(scan {5, 25000}, NOT(leaf)): the leapfrog of test_leapfrog_with_a_scan_by_hand over the complement — 6 + 30 000 + 1 + 5 010.
    (A NotDocIdIterator over the leaf's own iterator would evaluate every block while it steps over the 25 000 matches in front.)
    A leaf that holds from doc 25000 on, NOT(leaf) = [0, 25000), stopped after one doc (a selection's LIMIT 1): the first block holds a
    rejected doc — 10 000 entries.  (A NotDocIdIterator's constructor would pull the leaf's first match: three blocks.)"""
    n = 30011
    leaf = ~_mask(n, [25000])
    index = _mask(n, range(0, n, 10))
    entries, got = fm.entries_scanned_in_filter(("and", [("index", index), ("not", ("expr", leaf))]), n)
    assert (entries, got) == (3002, [25000])
    entries, got = fm.entries_scanned_in_filter(("and", [("not", ("expr", leaf)), ("scan", _mask(n, [5, 25000]))]), n)
    assert (entries, got) == (6 + 30000 + 1 + 5010, [25000])
    late = _mask(n, range(25000, n))
    entries, got = fm.entries_scanned_in_filter(("not", ("expr", late)), n, max_next=1)
    assert (entries, got) == (10000, [0])
    entries, got = fm.entries_scanned_in_filter(("not", ("expr", late)), n)
    assert entries == n and got == list(range(25000))
    # NOT over a plain scan stays a NotDocIdIterator over the scan's iterator: its constructor pulls the scan's first match
    entries, got = fm.entries_scanned_in_filter(("not", ("scan", late)), n, max_next=1)
    assert got == [0] and entries == 25088   # whole 256-doc batches up to the one that holds doc 25000: 98 x 256


def test_or_with_a_scan_drains_both():
    n = 10001
    entries, got = fm.entries_scanned_in_filter(("or", [("scan", _mask(n, [3])), ("expr", _mask(n, [10000]))]), n)
    assert got == [3, 10000] and entries == 2 * n
