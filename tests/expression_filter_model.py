"""A Python restatement, from the reference's Java, of what a predicate over an arithmetic expression (ExpressionFilterOperator) matches and of
what it costs in numEntriesScannedInFilter.

Predicates.  The four arithmetic transform functions return DOUBLE, so the reference evaluates the predicate with its raw DOUBLE evaluators:
  RANGE         v >= lo && v <= hi, an exclusive bound moved by Math.nextUp / nextDown first; an exclusive bound at its infinity is
                "Invalid range"                                                  (RangePredicateEvaluatorFactory.java:449-456,532)
  EQ / NOT_EQ   v == x / v != x: -0.0 equals 0.0, NaN equals nothing             (EqualsPredicateEvaluatorFactory.java:336,
                                                                                  NotEqualsPredicateEvaluatorFactory.java:298)
  IN / NOT_IN   membership in a fastutil DoubleOpenHashSet, which compares Double.doubleToLongBits: -0.0 is NOT in {0.0}, NaN IS in a set that
                holds NaN                                                        (InPredicateEvaluatorFactory.java:102,360)

Statistics.  The doc-id iterators, each over the match mask of its leaf (a numpy bool array over all docs), counting as the Java does:
  ExprScanIt    ExpressionScanDocIdIterator.java:81-145  blocks of DocIdSetPlanNode.MAX_DOC_PER_CALL = 10 000 docs; entries += block length
  SVScanIt      SVScanDocIdIterator.java:76-142          next(): batches of 256; advance(): doc by doc; applyAnd: the candidates
  and_iterator  AndDocIdSet.java:72-186                  index-based + scan-based children merged by applyAnd, else the leapfrog
  AndIt / OrIt / NotIt   AndDocIdIterator.java:37-66, OrDocIdIterator.java:50-135, NotDocIdIterator.java:35-70
A filter is a tree of ("expr" | "scan" | "index", mask), ("and" | "or", [children]), ("not", child); entries_scanned_in_filter() orders the
children of an AND by FilterOperatorUtils' priorities (sorted / inverted index 0 / 100 — "index" here —, AND 300, OR 400, scan 500, expression
1000; a NOT has its child's), builds the iterators as getTrues / getFalses do without null handling, drains the root by next() as
DocIdSetOperator does, and sums the scan-based iterators' counts.
NOT.  NotFilterOperator#getTrues (:52-57) is the child's getFalses.  BaseFilterOperator#getFalses (:105-122) is NotDocIdSet(trues) — a
NotDocIdIterator over the child's iterator — but ExpressionFilterOperator OVERRIDES it (ExpressionFilterOperator.java:100-110): its falses
are a second ExpressionDocIdSet with PredicateEvaluationResult.FALSE, so NOT(expression leaf) is itself a scan-based
ExpressionScanDocIdIterator over the docs the predicate rejects: applyAnd inside an AND, 10 000-doc blocks of the complement."""
import math

import numpy as np

EOF = -1
MAX_DOC_PER_CALL = 10000
SCAN_BATCH = 256
UNBOUNDED = "*"
NAN_BITS = 0x7FF8000000000000


class InvalidRange(ValueError):
    pass


# ---- the five evaluators ----------------------------------------------------------------------------------------------------------------------------
def long_bits(values) -> np.ndarray:
    """Double.doubleToLongBits: every NaN is the canonical one"""
    v = np.ascontiguousarray(values, dtype=np.float64)
    bits = v.view(np.uint64).copy()
    bits[np.isnan(v)] = NAN_BITS
    return bits


def range_bounds(lower: str, upper: str, lower_inclusive: bool, upper_inclusive: bool):
    lo = -math.inf if lower == UNBOUNDED else float(lower)
    hi = math.inf if upper == UNBOUNDED else float(upper)
    if lower != UNBOUNDED and not lower_inclusive:
        n = math.nextafter(lo, math.inf)
        if not n > lo:
            raise InvalidRange("Invalid range")
        lo = n
    if upper != UNBOUNDED and not upper_inclusive:
        n = math.nextafter(hi, -math.inf)
        if not n < hi:
            raise InvalidRange("Invalid range")
        hi = n
    return lo, hi


def apply_range(values, lower, upper, lower_inclusive, upper_inclusive) -> np.ndarray:
    lo, hi = range_bounds(lower, upper, lower_inclusive, upper_inclusive)
    v = np.asarray(values, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return (v >= lo) & (v <= hi)


def apply_eq(values, value: str) -> np.ndarray:
    with np.errstate(invalid="ignore"):
        return np.asarray(values, dtype=np.float64) == float(value)


def apply_not_eq(values, value: str) -> np.ndarray:
    with np.errstate(invalid="ignore"):
        return np.asarray(values, dtype=np.float64) != float(value)


def apply_in(values, literals) -> np.ndarray:
    members = long_bits(np.array([float(x) for x in literals], dtype=np.float64))
    return np.isin(long_bits(values), members)


def apply_not_in(values, literals) -> np.ndarray:
    return ~apply_in(values, literals)


def apply_predicate(values, p) -> np.ndarray:
    """`p`: a pinot_amd.query.Predicate (type, values, lower, upper, lower_inclusive, upper_inclusive)"""
    if p.type == "RANGE":
        return apply_range(values, p.lower, p.upper, p.lower_inclusive, p.upper_inclusive)
    if p.type == "EQ":
        return apply_eq(values, p.values[0])
    if p.type == "NOT_EQ":
        return apply_not_eq(values, p.values[0])
    if p.type == "IN":
        return apply_in(values, p.values)
    if p.type == "NOT_IN":
        return apply_not_in(values, p.values)
    raise ValueError(p.type)


# ---- iterators ----------------------------------------------------------------------------------------------------------------------------------------
class _Matches:
    """a leaf's matching docIds, ascending"""

    def __init__(self, mask):
        self.mask = np.asarray(mask, dtype=bool)
        self.n = len(self.mask)
        self.docs = np.flatnonzero(self.mask)

    def first_at_or_after(self, doc, end):
        """the first match in [doc, end), or EOF"""
        i = int(np.searchsorted(self.docs, doc, side="left"))
        if i < len(self.docs) and self.docs[i] < end:
            return int(self.docs[i])
        return EOF


class ExprScanIt:
    scan_based = True

    def __init__(self, mask):
        self.m = _Matches(mask)
        self.end_doc = self.m.n
        self.block_end = 0          # _blockEndDocId
        self.block = None           # _docIdIterator: (next position, end of its block)
        self.entries = 0

    def _from_block(self, at_least):
        pos, end = self.block
        d = self.m.first_at_or_after(max(pos, at_least), end)
        if d == EOF:
            self.block = (end, end)
            return EOF
        self.block = (d + 1, end)
        return d

    def next(self):
        if self.block is not None:
            d = self._from_block(0)
            if d != EOF:
                return d
        while self.block_end < self.end_doc:
            start = self.block_end
            self.block_end = min(start + MAX_DOC_PER_CALL, self.end_doc)
            self.entries += self.block_end - start          # processProjectionBlock: _numEntriesScanned += numDocs
            d = self.m.first_at_or_after(start, self.block_end)
            if d != EOF:
                self.block = (d + 1, self.block_end)
                return d
        return EOF

    def advance(self, target):
        if target < self.block_end:
            if self.block is not None:
                d = self._from_block(target)               # advanceIfNeeded never moves backwards
                if d != EOF:
                    return d
        else:
            self.block_end = target
        self.block = None
        return self.next()

    def apply_and(self, doc_mask):
        self.entries += int(np.count_nonzero(doc_mask))
        return doc_mask & self.m.mask


class SVScanIt:
    scan_based = True

    def __init__(self, mask):
        self.m = _Matches(mask)
        self.next_doc = 0
        self.batch = []
        self.cursor = 0
        self.entries = 0

    def next(self):
        if self.cursor >= len(self.batch):
            self.batch, self.cursor = [], 0
            while True:
                limit = min(self.m.n - self.next_doc, SCAN_BATCH)
                if limit <= 0:
                    break
                lo = self.next_doc
                self.batch = [int(d) for d in self.m.docs[np.searchsorted(self.m.docs, lo):np.searchsorted(self.m.docs, lo + limit)]]
                self.next_doc += limit
                self.entries += limit
                if self.batch:
                    break
            if not self.batch:
                return EOF
        d = self.batch[self.cursor]
        self.cursor += 1
        return d

    def advance(self, target):
        self.batch, self.cursor = [], 0
        self.next_doc = target
        if self.next_doc >= self.m.n:
            return EOF
        d = self.m.first_at_or_after(target, self.m.n)
        if d == EOF:
            self.entries += self.m.n - target
            self.next_doc = self.m.n
            return EOF
        self.entries += d - target + 1
        self.next_doc = d + 1
        return d

    def apply_and(self, doc_mask):
        self.entries += int(np.count_nonzero(doc_mask))
        return doc_mask & self.m.mask


class BitmapIt:
    """BitmapDocIdIterator / SortedDocIdIterator / RangelessBitmapDocIdIterator: index based, nothing is scanned"""
    scan_based = False
    index_based = True

    def __init__(self, mask):
        self.m = _Matches(mask)
        self.pos = 0

    def next(self):
        d = self.m.first_at_or_after(self.pos, self.m.n)
        self.pos = self.m.n if d == EOF else d + 1
        return d

    def advance(self, target):
        self.pos = max(self.pos, target)
        return self.next()


class AndIt:
    scan_based = False

    def __init__(self, its):
        self.its = its
        self.next_doc = 0

    def next(self):
        max_doc, max_index, index = self.next_doc, -1, 0
        while index < len(self.its):
            if index == max_index:
                index += 1
                continue
            d = self.its[index].advance(max_doc)
            if d == EOF:
                return EOF
            if d == max_doc:
                index += 1
            else:
                max_doc, max_index, index = d, index, 0
        self.next_doc = max_doc + 1
        return max_doc

    def advance(self, target):
        self.next_doc = target
        return self.next()


class OrIt:
    scan_based = False

    def __init__(self, its):
        self.its = list(its)
        self.next_ids = [-1] * len(its)
        self.live = len(its)
        self.previous = -1

    def _step(self, stale, move):
        best, exhausted = None, False
        for i in range(self.live):
            d = self.next_ids[i]
            if stale(d):
                d = move(self.its[i])
                self.next_ids[i] = d
                if d == EOF:
                    exhausted = True
                    continue
            best = d if best is None else min(best, d)
        if exhausted:
            i = 0
            while i < self.live:
                if self.next_ids[i] == EOF:
                    self.live -= 1
                    self.its[i] = self.its[self.live]
                    self.next_ids[i] = self.next_ids[self.live]
                else:
                    i += 1
        if best is None:
            return EOF
        self.previous = best
        return best

    def next(self):
        return self._step(lambda d: d == self.previous, lambda it: it.next())

    def advance(self, target):
        return self._step(lambda d: d < target, lambda it: it.advance(target))


class NotIt:
    scan_based = False

    def __init__(self, child, n_docs):
        self.child = child
        self.n = n_docs
        self.next_doc = 0
        d = child.next()
        self.next_non_matching = self.n if d == EOF else d

    def next(self):
        if self.next_doc >= self.n:
            return EOF
        while self.next_doc == self.next_non_matching:
            self.next_doc += 1
            d = self.child.next()
            self.next_non_matching = self.n if d == EOF else d
        if self.next_doc >= self.n:
            return EOF
        self.next_doc += 1
        return self.next_doc - 1

    def advance(self, target):
        self.next_doc = target
        if target > self.next_non_matching:
            d = self.child.advance(target)
            self.next_non_matching = self.n if d == EOF else d
        return self.next()


def and_iterator(its):
    """AndDocIdSet#iterator: with an index-based child beside a scan-based one (or two index-based ones) they merge into one bitmap — the
    scan-based ones by applyAnd over the surviving candidates, in list order — and only the remaining children are leapfrogged"""
    index = [it for it in its if getattr(it, "index_based", False)]
    scans = [it for it in its if it.scan_based]
    remaining = [it for it in its if it not in index and it not in scans]
    if (index and scans) or len(index) > 1:
        docs = index[0].m.mask.copy()
        for it in index[1:]:
            docs &= it.m.mask
        for it in scans:
            docs = it.apply_and(docs)
        merged = BitmapIt(docs)
        return merged if not remaining else AndIt([merged] + remaining)
    return AndIt(list(its))


_PRIORITY = {"index": 100, "and": 300, "or": 400, "scan": 500, "expr": 1000}


def _priority(node):
    return _priority(node[1]) if node[0] == "not" else _PRIORITY[node[0]]


def _build(node, n_docs, counted):
    kind = node[0]
    if kind in ("expr", "scan"):
        it = (ExprScanIt if kind == "expr" else SVScanIt)(node[1])
        counted.append(it)
        return it
    if kind == "index":
        return BitmapIt(node[1])
    if kind == "not":       # NotFilterOperator#getTrues = the child's getFalses
        if node[1][0] == "expr":   # ExpressionFilterOperator#getFalses: an ExpressionDocIdSet over the rejected docs
            it = ExprScanIt(~np.asarray(node[1][1], dtype=bool))
            counted.append(it)
            return it
        return NotIt(_build(node[1], n_docs, counted), n_docs)   # BaseFilterOperator#getFalses: NotDocIdSet(trues)
    children = list(node[1])
    if kind == "and":
        children.sort(key=_priority)   # (stable)
        return and_iterator([_build(c, n_docs, counted) for c in children])
    return OrIt([_build(c, n_docs, counted) for c in children])


def entries_scanned_in_filter(tree, n_docs: int, max_next: int = -1):
    """(numEntriesScannedInFilter, the docs the iterator returned) of the filter drained by next() (or stopped after max_next docs)"""
    counted = []
    it = _build(tree, n_docs, counted)
    docs = []
    while max_next < 0 or len(docs) < max_next:
        d = it.next()
        if d == EOF:
            break
        docs.append(d)
    return sum(c.entries for c in counted), docs
