"""Independent model of SELECT DISTINCT on one segment, for the tests.  It restates, over per-doc ids and the oracle's match set:

  DistinctPlanNode.java:50-77            no filter + one column with a dictionary -> DictionaryBasedDistinctOperator
  DictionaryBasedDistinctOperator.java:104-142,388-391
                                         the first min(limit, cardinality) dictionary values (the last ones under ORDER BY DESC);
                                         numDocsScanned = numEntriesScannedPostFilter = the values kept, numEntriesScannedInFilter = 0
  DistinctOperator.java:58-67            every other shape: blocks of DocIdSetPlanNode.MAX_DOC_PER_CALL = 10 000 matching docs
  DictionaryBasedSingleColumnDistinctExecutor.java:72-88, DictionaryBasedMultiColumnDistinctExecutor.java:102-124,184-188
                                         without ORDER BY: tuples in docId order until `limit` exist; the operator stops after that block
  DictIdDistinctTable.java:46-49, IntDistinctTable.java:108-130, DictionaryBasedMultiColumnDistinctExecutor.java:190-226
                                         with ORDER BY: the top `limit` tuples of the whole filter result (a heap: which tuples tied at the
                                         cut survive is unspecified)
  SVScanDocIdIterator.java:76-98         a scan reads whole batches of 256 docs (BlockDocIdIterator.OPTIMAL_ITERATOR_BATCH_SIZE)

Ids must order as the values do (dictIds; value-ordered ids of a raw column from `raw_ids`)."""
import math
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

BLOCK_DOCS = 10_000
SCAN_BATCH = 256


@dataclass
class DistinctModel:
    rows: List[tuple]                       # ids per column, in the result's order
    num_docs_scanned: int
    num_entries_scanned_post_filter: int
    early_stop: bool = False                # the operator stopped before its filter iterator reached the end
    last_consumed_doc: int = -1             # docId of the last doc consumed (early stop)
    tied: List[tuple] = field(default_factory=list)   # ORDER BY over fewer columns: the tuples tied at the cut (any of them may fill it)
    n_certain: int = 0                      # ... the rows before the tie class, which every valid answer holds

    def lone_scan_entries_in_filter(self, num_docs: int) -> int:
        """numEntriesScannedInFilter of a filter that is one scan predicate."""
        if not self.early_stop:
            return num_docs
        return min(num_docs, (self.last_consumed_doc // SCAN_BATCH + 1) * SCAN_BATCH)


def raw_ids(values: np.ndarray) -> Tuple[np.ndarray, list]:
    """Value-ordered ids of a raw column as the typed executors compare values: Integer / Long order, Float.compare / Double.compare for
    floating values (every NaN one value and the largest, -0.0 below 0.0).  Returns (ids, value of every id)."""
    v = np.asarray(values)
    if v.dtype.kind == "f":
        bits = v.astype(np.float64).view(np.int64).copy()
        bits[np.isnan(v)] = 0x7FF8000000000000            # Double.doubleToLongBits: one NaN
        key = np.where(bits < 0, bits ^ 0x7FFFFFFFFFFFFFFF, bits)   # order-preserving
        uniq, inv = np.unique(key, return_inverse=True)
        back = np.where(uniq < 0, uniq ^ 0x7FFFFFFFFFFFFFFF, uniq).view(np.float64)
        return inv.astype(np.int64), [float(x) for x in back]
    if v.dtype.kind in "iu":
        uniq, inv = np.unique(v.astype(np.int64), return_inverse=True)
        return inv.astype(np.int64), [int(x) for x in uniq]
    uniq, inv = np.unique(np.asarray(v, dtype=object).astype(str), return_inverse=True)   # strings: ids for identity only (no order)
    return inv.astype(np.int64), [str(x) for x in uniq]


def dictionary_path(cardinality: int, limit: int, descending: bool = False) -> DistinctModel:
    n = min(limit, cardinality)
    ids = [(cardinality - 1 - i,) if descending else (i,) for i in range(n)]
    return DistinctModel(ids, n, n)


def distinct(ids: Sequence[np.ndarray], match_docs: np.ndarray, limit: int,
             order_by: Optional[Sequence[Tuple[int, bool]]] = None) -> DistinctModel:
    """DistinctOperator over the matching docs (ascending docIds).  `ids`: per DISTINCT column the id of every doc; `order_by`:
    (column index, ascending) pairs."""
    n_cols = len(ids)
    match_docs = np.asarray(match_docs, dtype=np.int64)
    M = len(match_docs)
    cols = [np.asarray(c, dtype=np.int64)[match_docs] for c in ids]
    if M == 0:
        return DistinctModel([], 0, 0)
    tuples = np.stack(cols, axis=1)
    uniq, first = np.unique(tuples, axis=0, return_index=True)
    if not order_by:
        by_first = np.argsort(first, kind="stable")
        keep = by_first[:limit]
        rows = [tuple(int(x) for x in uniq[i]) for i in keep]
        if len(uniq) < limit:
            return DistinctModel(rows, M, M * n_cols)
        r = int(first[keep[-1]]) + 1                      # rank of the doc that adds the limit-th tuple
        scanned = min(M, BLOCK_DOCS * math.ceil(r / BLOCK_DOCS))
        early = scanned < M or M % BLOCK_DOCS == 0       # a full last block: the iterator was never asked past it
        return DistinctModel(rows, scanned, scanned * n_cols, early, int(match_docs[scanned - 1]))
    seen, ob = set(), []
    for c, asc in order_by:
        if c not in seen:
            seen.add(c)
            ob.append((c, asc))
    def okey(t):
        return tuple(t[c] if asc else -t[c] for c, asc in ob)
    all_rows = sorted((tuple(int(x) for x in u) for u in uniq), key=lambda t: (okey(t), t))
    rows = all_rows[:limit]
    model = DistinctModel(rows, M, M * n_cols)
    if len(all_rows) > limit and len(ob) < n_cols:
        cut = okey(rows[-1])
        model.tied = [t for t in all_rows if okey(t) == cut]
        model.n_certain = sum(1 for t in rows if okey(t) < cut)
    else:
        model.n_certain = len(rows)
    return model


def valid_ordered(got: Sequence[tuple], model: DistinctModel) -> bool:
    """`got` (ids per column, result order ignored) is a valid ORDER BY answer: the rows before the cut and the right number of tied ones."""
    if len(got) != len(model.rows):
        return False
    certain = set(model.rows[:model.n_certain])
    g = set(got)
    if not certain <= g:
        return False
    return (g - certain) <= set(model.tied) if model.tied else g == set(model.rows)
