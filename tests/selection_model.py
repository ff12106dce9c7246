"""Independent model of a selection query on one segment, for the tests.  It restates, over decoded columns and the oracle's match set:

  SelectionPlanNode.java:58-125          LIMIT 0 -> EmptySelectionOperator; no ORDER BY -> SelectionOnlyOperator; else SelectionOrderByOperator
  SelectionOnlyOperator.java:115-171     the first `limit` matching docs in docId order; numDocsScanned = min(limit, matches),
                                         numEntriesScannedPostFilter = numDocsScanned x the distinct output columns
  DocIdSetOperator.java:59-86            blocks of min(limit, 10 000) docs: the filter iterator stops after ceil(limit / B) x B next() calls
  SelectionOrderByOperator.java:146-368  the `limit` best rows of every match under the comparator of OrderByComparatorFactory.java:87-99
                                         (compareTo: dictIds for dictionary columns, Float.compare / Double.compare for raw floating values);
                                         numDocsScanned = matches, numEntriesScannedPostFilter = matches x ORDER BY columns + rows x the others
  SVScanDocIdIterator.java:76-98         a scan reads whole batches of 256 docs

A row is a tuple of output values in the representation of executor._key_repr (NaN "NaN", -0.0 "-0.0")."""
import math
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from pinot_amd.executor import _key_repr

BLOCK_DOCS = 10_000
SCAN_BATCH = 256


@dataclass
class SelectionModel:
    rows: List[tuple]
    num_docs_scanned: int
    num_entries_scanned_post_filter: int
    n_next: int = -1                         # next() calls of the filter iterator before the operator stopped (-1: drained)
    stop_doc: int = -1                       # the docId the last of them returned
    order_keys: List[tuple] = field(default_factory=list)   # ORDER BY: the sort key of every row
    tied: List[tuple] = field(default_factory=list)         # ORDER BY: every row tied at the cut (any of them may fill it)
    n_certain: int = 0                                      # ORDER BY: the rows before the tie class

    def lone_scan_entries_in_filter(self, num_docs: int) -> int:
        if self.n_next < 0:
            return num_docs
        return min(num_docs, (self.stop_doc // SCAN_BATCH + 1) * SCAN_BATCH)


def order_values(values: np.ndarray, dict_ids: Optional[np.ndarray]) -> np.ndarray:
    """Per doc an int64 (or object) that orders as the reference's comparator does: the dictId of a dictionary column, the value of a raw
    INT / LONG column, an order-preserving integer for a raw FLOAT / DOUBLE (Float.compare: -0.0 < 0.0, every NaN one value above +inf)."""
    if dict_ids is not None:
        return np.asarray(dict_ids, dtype=np.int64)
    v = np.asarray(values)
    if v.dtype.kind == "f":
        bits = v.astype(np.float64).view(np.int64).copy()
        bits[np.isnan(v)] = 0x7FF8000000000000
        return np.where(bits < 0, bits ^ 0x7FFFFFFFFFFFFFFF, bits)
    return v.astype(np.int64)


def _row(cols, d):
    return tuple(_key_repr(c[d].item() if isinstance(c[d], np.generic) else c[d]) for c in cols)


def selection(values: Sequence[Sequence], match_docs: np.ndarray, limit: int, n_distinct: int,
              order: Optional[Sequence[Tuple[int, bool, np.ndarray]]] = None) -> SelectionModel:
    """`values`: per output column the decoded value of every doc; `order`: (output column, ascending, order_values) per distinct ORDER BY
    column, most significant first."""
    docs = np.asarray(match_docs, dtype=np.int64)
    M = len(docs)
    if limit == 0:
        return SelectionModel([], 0, 0)
    if not order:
        n = min(limit, M)
        rows = [_row(values, int(d)) for d in docs[:n]]
        block = min(limit, BLOCK_DOCS)
        n_next = math.ceil(limit / block) * block
        m = SelectionModel(rows, n, n * n_distinct)
        if M >= n_next:
            m.n_next, m.stop_doc = n_next, int(docs[n_next - 1])
        return m
    keys = np.stack([(ov[docs] if asc else -ov[docs]) for _, asc, ov in order], axis=1) if M else np.zeros((0, len(order)), np.int64)
    idx = np.lexsort(keys.T[::-1]) if M else np.zeros(0, np.int64)
    k = min(limit, M)
    keep = idx[:k]
    rows = [_row(values, int(docs[i])) for i in keep]
    okeys = [tuple(int(x) for x in keys[i]) for i in keep]
    n_order_cols = len(order)
    n_other = n_distinct - n_order_cols
    m = SelectionModel(rows, M, M * n_order_cols + k * n_other, order_keys=okeys)
    if k and M > k:
        cut = okeys[-1]
        tied = np.flatnonzero(np.all(keys == np.array(cut, dtype=keys.dtype), axis=1))
        m.tied = [_row(values, int(docs[i])) for i in tied]
        m.n_certain = sum(1 for t in okeys if t < cut)
    else:
        m.n_certain = k
    return m


def check_ordered(got_rows: Sequence[tuple], got_keys: Sequence[tuple], m: SelectionModel) -> None:
    """An ORDER BY answer: sorted by the ORDER BY key, the rows before the cut all present, the rest drawn from the rows tied at the cut."""
    assert len(got_rows) == len(m.rows), (len(got_rows), len(m.rows))
    assert list(got_keys) == m.order_keys, "ORDER BY keys differ"
    from collections import Counter
    got_c = Counter(got_rows)
    certain = Counter(m.rows[:m.n_certain])
    assert not (certain - got_c), "a row before the cut is missing"
    rest = got_c - certain
    pool = Counter(m.tied) if m.tied else Counter(m.rows[m.n_certain:])
    assert not (rest - pool), "a row beyond the cut"
