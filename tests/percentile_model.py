"""numpy model of exact PERCENTILE(col, p) as the reference computes it (PercentileAggregationFunction.java:77-100,155-171):

  - the values of the matching docs as doubles (getDoubleValuesSV: an INT / LONG cast to double, a FLOAT widened exactly);
  - sorted by Arrays.sort(double[]) = Double.compare: -0.0 < 0.0, every NaN equal to every other and greater than everything;
  - final = sorted[(int)((long) n * p / 100)], sorted[n - 1] for p = 100, Double.NEGATIVE_INFINITY over no value;
  - the intermediate result is the list of every matching value (here: ascending, as (value, count) runs);
  - numDocsScanned = matches, numEntriesScannedPostFilter = matches x the distinct columns the query reads.

tests/test_percentile_model.py pins this to the reference's own expected values; the GPU tests hold the library to it."""
import numpy as np

NEG_INF = float("-inf")
_CANONICAL_NAN = np.uint64(0x7FF8000000000000)   # Double.doubleToLongBits collapses every NaN to this one


def as_doubles(values, data_type: str) -> np.ndarray:
    """getDoubleValuesSV of a column's values: (double) of an int / long (round to nearest even), a float widened exactly."""
    if data_type in ("INT", "LONG"):
        return np.asarray(values, dtype=np.int64).astype(np.float64)
    if data_type == "FLOAT":
        return np.asarray(values, dtype=np.float32).astype(np.float64)
    return np.asarray(values, dtype=np.float64)


def order_keys(d: np.ndarray) -> np.ndarray:
    """Unsigned keys ordered as Double.compare orders the doubles (all NaNs one key, the greatest)."""
    bits = np.ascontiguousarray(d, dtype=np.float64).view(np.uint64).copy()
    bits[np.isnan(d)] = _CANONICAL_NAN
    neg = (bits >> np.uint64(63)).astype(bool)
    return np.where(neg, ~bits, bits | np.uint64(1 << 63))


def sort_doubles(d: np.ndarray) -> np.ndarray:
    d = np.asarray(d, dtype=np.float64)
    return d[np.argsort(order_keys(d), kind="stable")]


def index_of(n: int, p: float) -> int:
    """The reference's index: (int)((long) n * p / 100) — a double product, a double quotient, truncation — and n - 1 for p = 100."""
    return n - 1 if p == 100.0 else int(float(n) * p / 100)


def final(d, p: float) -> float:
    d = np.asarray(d, dtype=np.float64)
    if d.size == 0:
        return NEG_INF
    return float(sort_doubles(d)[index_of(d.size, p)])


def runs(d):
    """The intermediate list as ascending (values, counts) runs: equal under Double.compare means one run (a NaN run holds every NaN)."""
    s = sort_doubles(np.asarray(d, dtype=np.float64))
    if s.size == 0:
        return np.zeros(0, dtype=np.float64), np.zeros(0, dtype=np.int64)
    k = order_keys(s)
    first = np.flatnonzero(np.concatenate(([True], k[1:] != k[:-1])))
    counts = np.diff(np.concatenate((first, [s.size]))).astype(np.int64)
    return s[first], counts


def same_double(a: float, b: float) -> bool:
    """Bit for bit, every NaN being the same value (Double.doubleToLongBits)."""
    a, b = np.float64(a), np.float64(b)
    if np.isnan(a) or np.isnan(b):
        return bool(np.isnan(a) and np.isnan(b))
    return a.view(np.uint64) == b.view(np.uint64)


def same_runs(got, want) -> bool:
    (gv, gc), (wv, wc) = got, want
    if len(gv) != len(wv) or not np.array_equal(np.asarray(gc, dtype=np.int64), np.asarray(wc, dtype=np.int64)):
        return False
    return np.array_equal(order_keys(np.asarray(gv, dtype=np.float64)), order_keys(np.asarray(wv, dtype=np.float64)))


def group_docs(key_columns, docs):
    """{group key tuple: the docs of the group, ascending} over the matching docs, in order of first appearance (the reference admits
    groups in docId order)."""
    docs = np.asarray(docs, dtype=np.int64)
    if docs.size == 0:
        return {}
    cols = [np.asarray(c)[docs] for c in key_columns]
    code = np.zeros(docs.size, dtype=np.int64)
    for c in cols:   # one integer per distinct tuple
        values, inverse = np.unique(c, return_inverse=True)
        code = code * len(values) + inverse
    order = np.argsort(code, kind="stable")   # stable: the docs of a group stay ascending
    starts = np.flatnonzero(np.concatenate(([True], code[order][1:] != code[order][:-1])))
    parts = np.split(order, starts[1:])
    parts.sort(key=lambda part: part[0])      # first appearance
    return {tuple(c[part[0]].item() for c in cols): docs[part] for part in parts}


def statistics(n_matches: int, columns_read) -> tuple:
    """(numDocsScanned, numEntriesScannedPostFilter)"""
    return n_matches, n_matches * len(set(columns_read))
