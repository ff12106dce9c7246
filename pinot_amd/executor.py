"""Host-side mirror of the reference's operator / plan-maker interface for the hot path, on top of the C ABI.

Reference classes mirrored (same names, argument meaning and error behaviour; all under pinot-core/src/main/java/org/
apache/pinot/core/):
  plan/maker/PlanMaker.java:37-67, InstancePlanMakerImplV2.java:275-294   → GpuInstancePlanMaker.make_segment_plan_node
  operator/query/GroupByOperator.java:100-140, AggregationOperator.java   → GpuGroupByOperator / GpuAggregationOperator
  operator/blocks/results/GroupByResultsBlock.java, AggregationResultsBlock → GroupByResultsBlock / AggregationResultsBlock
  operator/ExecutionStatistics.java                                        → ExecutionStatistics
  operator/combine/GroupByCombineOperator.java:102-165,191-222 + data/table/IndexedTable.java:90-120
                                                                           → GroupByCombineOperator (host merge)
The Java plug-in is the production host; this module is what the tests and bench.py drive.
`NativeSegment` works over any library exporting the pinot_gpu.h entry points; the product code only ever passes
capi.gpu_api() — the oracle binding lives in tests/.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from fractions import Fraction
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import capi
from .query import CQuery, QueryContext, parse_sql, with_time_arguments
from .segment import HostSegment


@dataclass
class ExecutionStatistics:
    num_docs_scanned: int
    num_entries_scanned_in_filter: int
    num_entries_scanned_post_filter: int
    num_total_docs: int


class NativeSegment:
    """IndexSegment handle: the host segment's buffers registered with (and, for the GPU library, pinned in HBM by) a
    native library.  `destroy()` mirrors IndexSegment#destroy."""

    def __init__(self, api: capi.NativeApi, host: HostSegment, device: Optional[int] = None):
        self.api = api
        self.host = host
        self.handle = C.c_void_p()
        self.device = device
        if device is None:       # the default device (pg_init)
            api.call("segment_create", host.name.encode(), host.total_docs, C.byref(self.handle))
        else:                    # segment -> GPU map of a multi-GPU server process
            api.call("segment_create_on_device", host.name.encode(), host.total_docs, int(device), C.byref(self.handle))
        self._descs = []
        for col in host.columns.values():
            self._register(col)
        for st in getattr(host, "star_trees", []):
            self.add_star_tree(st)

    def _register(self, col):
        d = col.desc()
        self._descs.append(d)
        self.api.call("segment_add_column", self.handle, C.byref(d))
        nv = getattr(col, "null_vector", None)
        if nv is not None:
            self.api.call("segment_set_null_vector", self.handle, col.name.encode(), nv.ctypes.data, nv.nbytes)
        ri = getattr(col, "range_index", None)
        if ri is not None:
            self.api.call("segment_set_range_index", self.handle, col.name.encode(), ri.ctypes.data, ri.nbytes)

    def set_queryable_doc_ids(self, doc_ids):
        """SegmentContext#getQueryableDocIdsSnapshot (upsert validDocIds): ascending docIds, or None to clear."""
        if doc_ids is None:
            self.api.call("segment_set_queryable_doc_ids", self.handle, None, 0)
            return
        from . import formats
        blob = np.frombuffer(formats.serialize_roaring(np.asarray(doc_ids, dtype=np.int64)), dtype=np.uint8)
        self.api.call("segment_set_queryable_doc_ids", self.handle, blob.ctypes.data, blob.nbytes)

    def add_column(self, col, keep_host_buffers: bool = True):
        """Registers one more column (streaming upload of big segments: the GPU library copies the bytes into HBM during
        the call, so the caller may drop the host buffers afterwards with keep_host_buffers=False)."""
        self._register(col)
        self.host.columns[col.name] = col
        if not keep_host_buffers:
            col.forward_index = None
            col.inverted_index = None
            self._descs.pop()

    def add_star_tree(self, star_tree):
        """StarTreeLoaderUtils#loadStarTreeV2: the dimensions must already be registered columns of this segment."""
        d = star_tree.desc()
        self.api.call("segment_add_star_tree", self.handle, C.byref(d))

    @property
    def total_docs(self) -> int:
        return self.host.total_docs

    def device_bytes(self) -> int:
        out = C.c_uint64()
        self.api.call("segment_device_bytes", self.handle, C.byref(out))
        return out.value

    def destroy(self):
        if self.handle:
            self.api.call("segment_destroy", self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    # -- FilterOperator / DocIdSetOperator ------------------------------------------------------------------------
    def filter(self, q, null_handling: bool = False) -> "DocIdSet":
        qc = parse_sql(q) if isinstance(q, str) else q
        cq = CQuery(qc, tuple(self.host.columns))
        h = C.c_void_p()
        if null_handling or (qc.flags & capi.QUERY_FLAG_NULL_HANDLING):   # enableNullHandling=true: three-valued filter
            self.api.call("filter_exec_flags", self.handle, cq.filter_ptr(), capi.QUERY_FLAG_NULL_HANDLING, C.byref(h))
        else:
            self.api.call("filter_exec", self.handle, cq.filter_ptr(), C.byref(h))
        return DocIdSet(self.api, h)

    # -- GroupByOperator / AggregationOperator ---------------------------------------------------------------------
    def execute(self, q, profile: bool = False) -> "ResultsBlock":
        qc = parse_sql(q) if isinstance(q, str) else q
        if profile:
            qc.flags |= capi.QUERY_FLAG_PROFILE
        cached = getattr(qc, "_cquery", None)     # the C structs of a QueryContext are reusable across executions
        cols = tuple(self.host.columns) if qc.selection else ()
        key = (qc.flags, qc.num_groups_limit, qc.limit, qc.min_segment_group_trim_size, cols)
        if cached is None or cached[0] != key:
            cached = (key, CQuery(qc, cols))
            qc._cquery = cached
        cq = cached[1]
        h = C.c_void_p()
        self.api.call("query_exec", self.handle, cq.ptr(), C.byref(h))
        try:
            return ResultsBlock.from_native(self.api, h, qc, self.host)
        finally:
            self.api.call("result_free", h)

    def execute_native(self, q, keep_device_table: bool = True, cancel: "Optional[CancelToken]" = None) -> "NativeResult":
        """Runs the query and keeps the native result handle (and, with `keep_device_table`, its dense accumulator table in HBM)
        so that it can be merged in the library: NativeResult.merge / .all_reduce, then .block()."""
        qc = parse_sql(q) if isinstance(q, str) else q
        flags = qc.flags | (capi.QUERY_FLAG_KEEP_DEVICE_TABLE if keep_device_table else 0)
        cache = getattr(qc, "_cquery_native", None)
        cols = tuple(self.host.columns) if qc.selection else ()
        key = (flags, qc.num_groups_limit, qc.limit, qc.min_segment_group_trim_size, cols)
        if cache is None or cache[0] != key:
            saved = qc.flags
            qc.flags = flags
            cache = (key, CQuery(qc, cols))
            qc.flags = saved
            qc._cquery_native = cache
        h = C.c_void_p()
        self.api.call("query_exec_cancellable", self.handle, cache[1].ptr(), cancel.handle if cancel is not None else None, C.byref(h))
        return NativeResult(self.api, h, qc, self.host)


class CancelToken:
    """pg_cancel_t: the interrupting thread calls request(); the executing thread's query returns PG_ERR_CANCELLED
    (EarlyTerminationException, BaseOperator.java:44-46)."""

    def __init__(self, api: capi.NativeApi):
        self.api = api
        self.handle = C.c_void_p()
        api.call("cancel_create", C.byref(self.handle))

    def request(self):
        self.api.call("cancel_request", self.handle)

    def reset(self):
        self.api.call("cancel_reset", self.handle)

    def destroy(self):
        if self.handle:
            self.api.call("cancel_destroy", self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class Comm:
    """pg_comm_t: an RCCL communicator owned by the library (one per GPU)."""

    def __init__(self, api: capi.NativeApi, handle):
        self.api = api
        self.handle = handle

    @staticmethod
    def unique_id(api: capi.NativeApi) -> bytes:
        buf = C.create_string_buffer(capi.COMM_UNIQUE_ID_BYTES)
        api.call("comm_get_unique_id", buf)
        return buf.raw

    @staticmethod
    def init_rank(api: capi.NativeApi, device: int, world: int, rank: int, unique_id: bytes) -> "Comm":
        assert len(unique_id) == capi.COMM_UNIQUE_ID_BYTES
        h = C.c_void_p()
        api.call("comm_init_rank", device, world, rank, C.create_string_buffer(unique_id, len(unique_id)), C.byref(h))
        return Comm(api, h)

    @staticmethod
    def init_all(api: capi.NativeApi, devices: Sequence[int]) -> "List[Comm]":
        n = len(devices)
        devs = (C.c_int32 * n)(*devices)
        out = (C.c_void_p * n)()
        api.call("comm_init_all", n, devs, out)
        return [Comm(api, C.c_void_p(out[i])) for i in range(n)]

    def world_size(self) -> int:
        n = C.c_int32()
        self.api.call("comm_world_size", self.handle, C.byref(n))
        return n.value

    def destroy(self):
        if self.handle:
            self.api.call("comm_destroy", self.handle)
            self.handle = C.c_void_p()


class NativeResult:
    """A pg_result_t kept alive for merging inside the library (GroupByCombineOperator over segments sharing their key
    space): merge() folds another segment's result of the same query on the same GPU into this one, all_reduce() merges
    across the GPUs of a communicator over RCCL; block() materialises the (merged) intermediate results."""

    def __init__(self, api: capi.NativeApi, handle, qc: QueryContext, host: HostSegment):
        self.api = api
        self.handle = handle
        self.qc = qc
        self.host = host

    def merge(self, other: "NativeResult") -> "NativeResult":
        self.api.call("result_merge", self.handle, other.handle)
        return self

    def all_reduce(self, comm: Comm) -> "NativeResult":
        self.api.call("result_all_reduce", self.handle, comm.handle)
        return self

    def block(self) -> "ResultsBlock":
        return ResultsBlock.from_native(self.api, self.handle, self.qc, self.host)

    def stats(self) -> capi.PgExecStats:
        st = capi.PgExecStats()
        self.api.call("result_stats", self.handle, C.byref(st))
        return st

    def data_table_v4(self) -> bytes:
        """The (merged) intermediate results as DataTableImplV4 bytes (pg_result_data_table_v4)."""
        size = C.c_int64(0)
        self.api.call("result_data_table_v4", self.handle, None, 0, C.byref(size))
        buf = (C.c_uint8 * max(size.value, 1))()
        self.api.call("result_data_table_v4", self.handle, buf, size.value, C.byref(size))
        return bytes(buf[:size.value])

    def free(self):
        if self.handle:
            self.api.call("result_free", self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DocIdSet:
    def __init__(self, api: capi.NativeApi, handle):
        self.api = api
        self.handle = handle

    def cardinality(self) -> int:
        out = C.c_int64()
        self.api.call("docidset_cardinality", self.handle, C.byref(out))
        return out.value

    def words(self) -> np.ndarray:
        n = C.c_int64()
        self.api.call("docidset_num_words", self.handle, C.byref(n))
        out = np.zeros(n.value, dtype=np.uint64)
        self.api.call("docidset_copy_words", self.handle, out.ctypes.data, n.value)
        return out

    def doc_ids(self) -> np.ndarray:
        n = self.cardinality()
        out = np.zeros(n, dtype=np.int32)
        self.api.call("docidset_copy_docids", self.handle, out.ctypes.data, n)
        return out

    def stats(self) -> capi.PgExecStats:
        s = capi.PgExecStats()
        self.api.call("docidset_stats", self.handle, C.byref(s))
        return s

    def free(self):
        if self.handle:
            self.api.call("docidset_free", self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _key_columns(qc: QueryContext, host: HostSegment) -> List[str]:
    """The columns whose values come back as group keys: GROUP BY columns, DISTINCT columns, or a selection's output columns."""
    if qc.selection:
        return qc.extract_expressions(host.columns)
    return qc.distinct or qc.group_by


def _key_repr(v):
    """Group key component as a dict key: floats keep their sign of zero (-0.0 and 0.0 are two groups in the reference's
    Float2Int / Double2Int maps, but equal as Python floats) and NaN compares equal to itself."""
    if isinstance(v, float):
        if v != v:
            return "NaN"
        if v == 0.0:
            return "-0.0" if math.copysign(1.0, v) < 0 else 0.0
    return v


class ResultsBlock:
    """GroupByResultsBlock / AggregationResultsBlock: intermediate results per group key.

    `rows` maps the decoded group key tuple (dictionary values, as GroupKeyGenerator#getGroupKeys yields them) to the
    list of intermediate results, one per aggregation: COUNT → int, SUM/MIN/MAX → float, AVG → (sum, count),
    MINMAXRANGE → (min, max), DISTINCTCOUNT → frozenset of values, DISTINCTCOUNTHLL → bytes of 2^log2m registers.
    The native arrays are kept as numpy arrays (`arrays`, `group_dict_ids`); the Python-object views (`group_keys`,
    `columns`) are built on first use so that the benchmark loop does not pay for boxing."""

    def __init__(self):
        self.query: Optional[QueryContext] = None
        self.group_dict_ids: Optional[np.ndarray] = None   # [n_group_cols, n_groups]
        self.arrays: List[tuple] = []                       # per aggregation: (kind, component arrays...)
        self.stats: Optional[capi.PgExecStats] = None
        self._host: Optional[HostSegment] = None
        self._group_keys: Optional[List[tuple]] = None
        self._columns: Optional[List[list]] = None

    @staticmethod
    def from_native(api: capi.NativeApi, h, qc: QueryContext, host: HostSegment) -> "ResultsBlock":
        rb = ResultsBlock()
        rb.query = qc
        rb._host = host
        n = C.c_int32()
        api.call("result_num_groups", h, C.byref(n))
        ng = n.value
        keys = _key_columns(qc, host)   # SELECT DISTINCT: the tuples, a selection: the rows come back as group keys
        rb.key_columns = keys
        ngb = len(keys)
        ids = np.zeros((ngb, ng), dtype=np.int32)
        rb.group_values = None
        rb.group_value_columns = {}      # group-by column index -> the groups' values (no-dictionary columns)
        for j in range(ngb):
            kt = C.c_int32()
            api.call("result_group_key_type", h, j, C.byref(kt))
            if kt.value == capi.GROUP_KEY_LONG_VALUES:   # a no-dictionary group-by column: the groups' values themselves
                vals = np.zeros(ng, dtype=np.int64)
                api.call("result_group_values_long", h, j, vals.ctypes.data, ng)
                rb.group_value_columns[j] = vals
            elif kt.value == capi.GROUP_KEY_DOUBLE_VALUES:
                vals = np.zeros(ng, dtype=np.float64)
                api.call("result_group_values_double", h, j, vals.ctypes.data, ng)
                rb.group_value_columns[j] = vals
            elif kt.value == capi.GROUP_KEY_BYTES_VALUES:   # a raw STRING / BYTES group-by column: the groups' byte strings
                total = C.c_uint64()
                api.call("result_group_values_bytes_size", h, j, C.byref(total))
                offs = np.zeros(ng + 1, dtype=np.int64)
                blob = np.zeros(max(int(total.value), 1), dtype=np.uint8)
                api.call("result_group_values_bytes", h, j, offs.ctypes.data, ng + 1, blob.ctypes.data, int(total.value))
                raw = blob.tobytes()
                vals = np.empty(ng, dtype=object)
                is_string = host.columns[keys[j]].data_type == "STRING"
                for i in range(ng):
                    v = raw[offs[i]:offs[i + 1]]
                    vals[i] = v.decode("utf-8") if is_string else v
                rb.group_value_columns[j] = vals
            else:
                api.call("result_group_dict_ids", h, j, ids[j].ctypes.data, ng)
        if ngb == 1 and 0 in rb.group_value_columns and rb.group_value_columns[0].dtype == np.int64:
            rb.group_values = rb.group_value_columns[0]
        rb.group_dict_ids = ids
        for a, spec in enumerate(qc.aggregations):
            kind = C.c_int32()
            api.call("result_kind_of", h, a, C.byref(kind))
            k = kind.value
            if k == capi.RESULT_LONG:
                out = np.zeros(ng, dtype=np.int64)
                api.call("result_longs", h, a, 0, out.ctypes.data, ng)
                rb.arrays.append((k, out))
            elif k == capi.RESULT_DOUBLE:
                out = np.zeros(ng, dtype=np.float64)
                api.call("result_doubles", h, a, 0, out.ctypes.data, ng)
                rb.arrays.append((k, out))
            elif k == capi.RESULT_AVG_PAIR:
                s = np.zeros(ng, dtype=np.float64)
                c = np.zeros(ng, dtype=np.int64)
                api.call("result_doubles", h, a, 0, s.ctypes.data, ng)
                api.call("result_longs", h, a, 0, c.ctypes.data, ng)
                rb.arrays.append((k, s, c))
            elif k == capi.RESULT_MINMAX_PAIR:
                lo = np.zeros(ng, dtype=np.float64)
                hi = np.zeros(ng, dtype=np.float64)
                api.call("result_doubles", h, a, 0, lo.ctypes.data, ng)
                api.call("result_doubles", h, a, 1, hi.ctypes.data, ng)
                rb.arrays.append((k, lo, hi))
            elif k == capi.RESULT_DICTID_SET:
                sizes = np.zeros(ng, dtype=np.int32)
                api.call("result_set_sizes", h, a, sizes.ctypes.data, ng)
                total = int(sizes.sum())
                flat = np.zeros(max(total, 1), dtype=np.int32)
                api.call("result_set_dict_ids", h, a, flat.ctypes.data, total)
                rb.arrays.append((k, sizes, flat[:total]))
            elif k == capi.RESULT_VALUE_SET:   # DISTINCTCOUNT over a raw column: the values themselves
                sizes = np.zeros(ng, dtype=np.int32)
                api.call("result_set_sizes", h, a, sizes.ctypes.data, ng)
                total = int(sizes.sum())
                floating = host.columns[spec.column].data_type in ("FLOAT", "DOUBLE")
                flat = np.zeros(max(total, 1), dtype=np.float64 if floating else np.int64)
                api.call("result_set_values_double" if floating else "result_set_values_long", h, a, flat.ctypes.data, total)
                rb.arrays.append((k, sizes, flat[:total]))
            elif k == capi.RESULT_VALUE_COUNTS:   # PERCENTILE: per group the ascending (value, count) runs of its DoubleArrayList
                sizes = np.zeros(ng, dtype=np.int32)
                api.call("result_set_sizes", h, a, sizes.ctypes.data, ng)
                total = int(sizes.sum())
                values = np.zeros(max(total, 1), dtype=np.float64)
                counts = np.zeros(max(total, 1), dtype=np.int64)
                api.call("result_set_values_double", h, a, values.ctypes.data, total)
                api.call("result_set_counts", h, a, counts.ctypes.data, total)
                rb.arrays.append((k, sizes, values[:total], counts[:total]))
            elif k == capi.RESULT_VALUE_COUNT_MAP:   # MODE: per group the map value -> count, keys typed by the column (exact int64, or float64)
                sizes = np.zeros(ng, dtype=np.int32)
                api.call("result_set_sizes", h, a, sizes.ctypes.data, ng)
                total = int(sizes.sum())
                data_type = host.columns[spec.column.split(",")[0].strip()].data_type
                floating = data_type in ("FLOAT", "DOUBLE")
                keys = np.zeros(max(total, 1), dtype=np.float64 if floating else np.int64)
                counts = np.zeros(max(total, 1), dtype=np.int64)
                api.call("result_set_values_double" if floating else "result_set_values_long", h, a, keys.ctypes.data, total)
                api.call("result_set_counts", h, a, counts.ctypes.data, total)
                rb.arrays.append((k, sizes, keys[:total], counts[:total], data_type))
            elif k == capi.RESULT_DOUBLE_ARRAY:   # HISTOGRAM: per group the numBins counts of its DoubleArrayList
                sizes = np.zeros(ng, dtype=np.int32)
                api.call("result_set_sizes", h, a, sizes.ctypes.data, ng)
                total = int(sizes.sum())
                values = np.zeros(max(total, 1), dtype=np.float64)
                api.call("result_set_values_double", h, a, values.ctypes.data, total)
                rb.arrays.append((k, sizes, values[:total]))
            elif k == capi.RESULT_VARIANCE_TUPLE:   # VAR_POP / VAR_SAMP / STDDEV_POP / STDDEV_SAMP: VarianceTuple(count, sum, m2)
                n = np.zeros(ng, dtype=np.int64)
                s = np.zeros(ng, dtype=np.float64)
                m2 = np.zeros(ng, dtype=np.float64)
                api.call("result_longs", h, a, 0, n.ctypes.data, ng)
                api.call("result_doubles", h, a, 0, s.ctypes.data, ng)
                api.call("result_doubles", h, a, 1, m2.ctypes.data, ng)
                rb.arrays.append((k, n, s, m2))
            elif k == capi.RESULT_COVARIANCE_TUPLE:   # COVAR_POP / COVAR_SAMP: CovarianceTuple(sumX, sumY, sumXY, count)
                sums = [np.zeros(ng, dtype=np.float64) for _ in range(3)]
                n = np.zeros(ng, dtype=np.int64)
                for c in range(3):
                    api.call("result_doubles", h, a, c, sums[c].ctypes.data, ng)
                api.call("result_longs", h, a, 0, n.ctypes.data, ng)
                rb.arrays.append((k, sums[0], sums[1], sums[2], n))
            elif k == capi.RESULT_FOURTH_MOMENT:   # SKEWNESS / KURTOSIS: PinotFourthMoment(n, m1, m2, m3, m4)
                n = np.zeros(ng, dtype=np.int64)
                m = [np.zeros(ng, dtype=np.float64) for _ in range(4)]
                api.call("result_longs", h, a, 0, n.ctypes.data, ng)
                for c in range(4):
                    api.call("result_doubles", h, a, c, m[c].ctypes.data, ng)
                rb.arrays.append((k, n, m[0], m[1], m[2], m[3]))
            elif k == capi.RESULT_VALUE_TIME_PAIR:   # FIRSTWITHTIME / LASTWITHTIME: ValueLongPair(value, time), the value in its declared type
                floating = with_time_arguments(spec.column)[2] in ("FLOAT", "DOUBLE")
                t = np.zeros(ng, dtype=np.int64)
                v = np.zeros(ng, dtype=np.float64 if floating else np.int64)
                api.call("result_longs", h, a, 0, t.ctypes.data, ng)
                if floating:
                    api.call("result_doubles", h, a, 0, v.ctypes.data, ng)
                else:
                    api.call("result_longs", h, a, 1, v.ctypes.data, ng)
                rb.arrays.append((k, v, t))
            elif k == capi.RESULT_HLL:
                m = 1 << (spec.log2m or 8)
                regs = np.empty(max(ng * m, 1), dtype=np.uint8)
                api.call("result_hll_registers", h, a, regs.ctypes.data, ng * m)
                rb.arrays.append((k, regs[:ng * m].reshape(ng, m)))
            else:
                raise RuntimeError(f"unknown result kind {k}")
        # enableNullHandling: which results / group keys are NULL (all zero without the flag: not asked for then)
        rb.agg_nulls, rb.key_nulls = {}, {}
        if qc.flags & capi.QUERY_FLAG_NULL_HANDLING:
            for a in range(len(qc.aggregations)):
                f = np.zeros(max(ng, 1), dtype=np.uint8)
                api.call("result_agg_nulls", h, a, f.ctypes.data, ng)
                if f[:ng].any():
                    rb.agg_nulls[a] = f[:ng].astype(bool)
            for j in range(ngb):
                f = np.zeros(max(ng, 1), dtype=np.uint8)
                api.call("result_group_key_nulls", h, j, f.ctypes.data, ng)
                if f[:ng].any():
                    rb.key_nulls[j] = f[:ng].astype(bool)
        st = capi.PgExecStats()
        api.call("result_stats", h, C.byref(st))
        rb.stats = st
        return rb

    @property
    def num_groups(self) -> int:
        return self.group_dict_ids.shape[1] if (self.query.distinct or self.query.group_by or self.query.selection) else 1

    @property
    def selection_rows(self) -> List[tuple]:
        """A selection: the rows in result order (sorted under ORDER BY, else in docId order), one value per output column
        (`key_columns`, extractExpressions order), decoded as distinct_rows are."""
        assert self.query.selection, "not a selection query"
        return self.group_keys

    @property
    def distinct_rows(self) -> List[tuple]:
        """SELECT DISTINCT: the tuples in result order (sorted under ORDER BY, else by first matching docId), decoded — dictionary values,
        raw values, strings; a NaN is "NaN" and -0.0 is "-0.0" so that tuples compare as the reference's typed executors do."""
        assert self.query.distinct, "not a DISTINCT query"
        return self.group_keys

    @property
    def group_keys(self) -> List[tuple]:
        if self._group_keys is None and getattr(self, "group_values", None) is not None:
            kn = getattr(self, "key_nulls", {}).get(0)
            self._group_keys = [(None if (kn is not None and kn[i]) else int(v),) for i, v in enumerate(self.group_values)]
        if self._group_keys is None:
            ids = self.group_dict_ids
            vcols = getattr(self, "group_value_columns", {})
            ng = self.num_groups
            per_col = []
            for j, g in enumerate(getattr(self, "key_columns", None) or self.query.distinct or self.query.group_by):
                if j in vcols:   # raw values; a NaN key is one group: give it a key that compares equal to itself
                    v = vcols[j]
                    per_col.append(list(v) if v.dtype == object else ([int(x) for x in v] if v.dtype == np.int64 else [float(x) for x in v]))
                else:
                    dv = self._host.columns[g].dict_values
                    per_col.append([dv[ids[j, i]] for i in range(ng)])
            kn = getattr(self, "key_nulls", {})
            self._group_keys = [tuple(None if (j in kn and kn[j][i]) else _key_repr(per_col[j][i]) for j in range(len(per_col))) for i in range(ng)]
        return self._group_keys

    @property
    def columns(self) -> List[list]:
        if self._columns is None:
            cols = []
            for spec, arr in zip(self.query.aggregations, self.arrays):
                k = arr[0]
                if k == capi.RESULT_LONG:
                    cols.append([int(v) for v in arr[1]])
                elif k == capi.RESULT_DOUBLE:
                    cols.append([float(v) for v in arr[1]])
                elif k == capi.RESULT_AVG_PAIR:
                    cols.append([(float(x), int(y)) for x, y in zip(arr[1], arr[2])])
                elif k == capi.RESULT_MINMAX_PAIR:
                    cols.append([(float(x), float(y)) for x, y in zip(arr[1], arr[2])])
                elif k == capi.RESULT_DICTID_SET:
                    dv = self._host.columns[spec.column].dict_values
                    col, pos = [], 0
                    for sz in arr[1]:
                        col.append(frozenset(dv[d] for d in arr[2][pos:pos + sz]))
                        pos += sz
                    cols.append(col)
                elif k == capi.RESULT_VALUE_SET:
                    col, pos = [], 0
                    for sz in arr[1]:
                        col.append(frozenset(arr[2][pos:pos + sz].tolist()))
                        pos += sz
                    cols.append(col)
                elif k == capi.RESULT_VARIANCE_TUPLE:   # (count, sum, m2) per group
                    cols.append([(int(n), float(s), float(m2)) for n, s, m2 in zip(arr[1], arr[2], arr[3])])
                elif k == capi.RESULT_COVARIANCE_TUPLE:   # (sumX, sumY, sumXY, count) per group
                    cols.append([(float(sx), float(sy), float(sxy), int(n)) for sx, sy, sxy, n in zip(arr[1], arr[2], arr[3], arr[4])])
                elif k == capi.RESULT_FOURTH_MOMENT:   # (n, m1, m2, m3, m4) per group
                    cols.append([(int(n), float(m1), float(m2), float(m3), float(m4)) for n, m1, m2, m3, m4 in zip(*arr[1:6])])
                elif k == capi.RESULT_VALUE_TIME_PAIR:   # (value, time) per group; a FLOAT / DOUBLE value keeps its bits (NaN payloads, -0.0)
                    cols.append([(v.item(), int(t)) for v, t in zip(arr[1], arr[2])])
                elif k == capi.RESULT_VALUE_COUNT_MAP:   # a ModeMap per group: (type, ((key, count), ...)) ascending by key; empty: ("INT", ())
                    col, pos = [], 0
                    for sz in arr[1]:
                        col.append(mode_map(arr[4], [v.item() for v in arr[2][pos:pos + sz]], [int(c) for c in arr[3][pos:pos + sz]]))
                        pos += sz
                    cols.append(col)
                elif k == capi.RESULT_DOUBLE_ARRAY:   # a tuple of floats per group
                    col, pos = [], 0
                    for sz in arr[1]:
                        col.append(tuple(float(v) for v in arr[2][pos:pos + sz]))
                        pos += sz
                    cols.append(col)
                elif k == capi.RESULT_VALUE_COUNTS:   # (values, counts) per group
                    col, pos = [], 0
                    for sz in arr[1]:
                        col.append((arr[2][pos:pos + sz].copy(), arr[3][pos:pos + sz].copy()))
                        pos += sz
                    cols.append(col)
                else:
                    cols.append([bytes(r) for r in arr[1]])
            for a, flags in getattr(self, "agg_nulls", {}).items():   # enableNullHandling: a NULL result
                cols[a] = [None if flags[i] else v for i, v in enumerate(cols[a])]
            self._columns = cols
        return self._columns

    # -- conveniences ----------------------------------------------------------------------------------------------
    def execution_statistics(self) -> ExecutionStatistics:
        s = self.stats
        return ExecutionStatistics(s.num_docs_scanned, s.num_entries_scanned_in_filter,
                                   s.num_entries_scanned_post_filter, s.num_total_docs)

    def rows(self) -> Dict[tuple, list]:
        return {k: [col[i] for col in self.columns] for i, k in enumerate(self.group_keys)}

    def aggregation_result(self) -> list:
        """AggregationResultsBlock#getResults for a query without GROUP BY."""
        assert not self.query.group_by
        return [col[0] for col in self.columns]


# ----------------------------------------------------------------------------------------------------------------------
# HyperLogLog cardinality (final result extraction; stream-lib HyperLogLog#cardinality)
# ----------------------------------------------------------------------------------------------------------------------
def hll_cardinality(registers: bytes) -> int:
    m = len(registers)
    if m == 16:
        alpha_mm = 0.673 * m * m
    elif m == 32:
        alpha_mm = 0.697 * m * m
    elif m == 64:
        alpha_mm = 0.709 * m * m
    else:
        alpha_mm = (0.7213 / (1 + 1.079 / m)) * m * m
    s = 0.0
    zeros = 0.0
    for v in registers:
        s += 1.0 / (1 << v)
        if v == 0:
            zeros += 1
    est = alpha_mm * (1 / s)
    if est <= 2.5 * m:
        if zeros == 0:   # linearCounting: m * log(m / 0.0) = Infinity, Math.round(Infinity) = Long.MAX_VALUE
            return (1 << 63) - 1
        return int(math.floor(m * math.log(m / zeros) + 0.5))
    return int(math.floor(est + 0.5))


def percentile_expand(runs) -> np.ndarray:
    """The reference's DoubleArrayList behind a PERCENTILE intermediate `(values, counts)`: every matching value, ascending."""
    values, counts = runs
    return np.repeat(np.asarray(values, dtype=np.float64), np.asarray(counts, dtype=np.int64))


def percentile_final(runs, p: float) -> float:
    """PercentileAggregationFunction#extractFinalResult (:155-171) over the runs: sorted[(int)((long) size * p / 100)], the last value for
    p = 100, Double.NEGATIVE_INFINITY over an empty list."""
    values, counts = runs
    n = int(np.sum(counts))
    if n == 0:
        return float("-inf")
    rank = n - 1 if p == 100.0 else int(float(n) * p / 100)
    return float(values[int(np.searchsorted(np.cumsum(counts), rank, side="right"))])


def variance_final(function: str, t) -> float:
    """VarianceAggregationFunction#extractFinalResult over the tuple (count, sum, m2): m2 / count for the population forms, m2 / (count - 1)
    for the sample forms, Math.sqrt of that for STDDEV; Double.NEGATIVE_INFINITY for count 0 and, for the sample forms, count 1."""
    n, _, m2 = t
    sample = function in ("VARSAMP", "STDDEVSAMP")
    if n == 0 or (sample and n == 1):
        return float("-inf")
    v = m2 / (n - 1) if sample else m2 / n
    return math.sqrt(v) if function in ("STDDEVPOP", "STDDEVSAMP") else v


def variance_merge(a, b):
    """VarianceTuple#apply(VarianceTuple): `b` merged into `a` (what the Java side does with the tuples of two segments)."""
    if b[0] == 0:
        return a
    n, s, m2 = a
    avg = 0.0 if n == 0 else s / n
    delta = (b[1] / b[0]) - avg
    return (n + b[0], s + b[1], m2 + (b[2] + delta * delta * b[0] * n / (b[0] + n)))


def covariance_final(function: str, t) -> float:
    """CovarianceAggregationFunction#extractFinalResult over the tuple (sumX, sumY, sumXY, count), in its operation order:
    sumXY / count - (sumX * sumY) / (count * count) for COVAR_POP, sumXY / (count - 1) - (sumX * sumY) / (count * (count - 1)) for
    COVAR_SAMP; Double.NEGATIVE_INFINITY for count 0 and, for COVAR_SAMP, count 1."""
    sx, sy, sxy, n = t
    sample = function == "COVARSAMP"
    if n == 0 or (sample and n == 1):
        return float("-inf")
    with np.errstate(all="ignore"):   # Java double arithmetic: overflow gives an infinity, never an exception
        sx, sy, sxy, c = np.float64(sx), np.float64(sy), np.float64(sxy), np.float64(n)
        if sample:
            return float(sxy / (c - 1) - (sx * sy) / (c * (c - 1)))
        return float(sxy / c - (sx * sy) / (c * c))


def covariance_merge(a, b):
    """CovarianceTuple#apply(CovarianceTuple): `b` added to `a` member by member (what the Java side does with the tuples of two segments)."""
    return (a[0] + b[0], a[1] + b[1], a[2] + b[2], a[3] + b[3])


def skewness_final(t) -> float:
    """FourthMomentAggregationFunction#extractFinalResult for SKEWNESS over the tuple (n, m1, m2, m3, m4) — Commons Math Skewness#getResult:
    NaN for n < 3; with the variance v = m2 / (n - 1), 0.0 for v < 10E-20; else n m3 / ((n - 1)(n - 2) sqrt(v) v)."""
    n, _, m2, m3, _ = t
    if n < 3:
        return float("nan")
    with np.errstate(all="ignore"):   # Java double arithmetic: never an exception
        n0, v = np.float64(n), np.float64(m2) / np.float64(n - 1)
        if v < 10E-20:
            return 0.0
        return float((n0 * np.float64(m3)) / ((n0 - 1) * (n0 - 2) * np.sqrt(v) * v))


def kurtosis_final(t) -> float:
    """... for KURTOSIS — Commons Math Kurtosis#getResult: NaN for n <= 3; 0.0 for a variance v = m2 / (n - 1) below 10E-20; else
    (n (n + 1) m4 - 3 m2 m2 (n - 1)) / ((n - 1)(n - 2)(n - 3) v v)."""
    n, _, m2, _, m4 = t
    if n <= 3:
        return float("nan")
    with np.errstate(all="ignore"):
        n0, m2, m4 = np.float64(n), np.float64(m2), np.float64(m4)
        v = m2 / (n0 - 1)
        if v < 10E-20:
            return 0.0
        return float((n0 * (n0 + 1) * m4 - 3 * m2 * m2 * (n0 - 1)) / ((n0 - 1) * (n0 - 2) * (n0 - 3) * v * v))


def fourth_moment_merge(a, b):
    """PinotFourthMoment#combine: `b` merged into `a` (what the Java side does with the tuples of two segments) — the pairwise update of the
    mean and the central sums, in double; an empty side leaves the other as it is."""
    if b[0] == 0:
        return a
    if a[0] == 0:
        return b
    with np.errstate(all="ignore"):
        an, a1, a2, a3, a4 = a[0], *(np.float64(x) for x in a[1:])
        bn, b1, b2, b3, b4 = b[0], *(np.float64(x) for x in b[1:])
        n = an + bn
        fa, fb, fn = np.float64(an), np.float64(bn), np.float64(n)
        m1 = (fa * a1 + fb * b1) / fn
        d = b1 - a1
        d2 = d * d
        m2 = a2 + b2 + d2 * fa * fb / fn
        d3 = d2 * d
        m3 = a3 + b3 + d3 * fa * fb * np.float64(an - bn) / np.float64(n * n) + 3.0 * d * (fa * b2 - fb * a2) / fn
        d4 = d3 * d
        m4 = (a4 + b4 + d4 * fa * fb * np.float64(an * an - an * bn + bn * bn) / (fn * fn * fn)
              + 6.0 * d2 * (np.float64(an * an) * b2 + np.float64(bn * bn) * a2) / np.float64(n * n) + 4.0 * d * (fa * b3 - fb * a3) / fn)
    return (n, float(m1), float(m2), float(m3), float(m4))


def _double_compare_key(v):
    """Double.compare order for float keys (-0.0 < 0.0, NaN greatest, one NaN); integers as they are"""
    if isinstance(v, float):
        if v != v:
            return (1, 0.0, 0)
        return (0, v, 0 if (v != 0.0 or math.copysign(1.0, v) < 0) else 1)
    return (0, v, 0)


def mode_map(data_type: str, keys, counts):
    """MODE's intermediate as a hashable value: (type, ((key, count), ...)), the entries ascending by key — "INT" / "LONG" keys Python ints,
    "FLOAT" / "DOUBLE" keys floats (a FLOAT widened exactly).  An empty map is ("INT", ()): the reference's Int2LongOpenHashMap, whatever
    the column's type."""
    entries = tuple(sorted(zip(keys, counts), key=lambda e: _double_compare_key(e[0])))
    return (data_type, entries) if entries else ("INT", ())


def mode_merge(a, b):
    """ModeAggregationFunction#merge: an empty map yields the other; else the per-key sum; maps of two key types are refused with the
    reference's text."""
    if not a[1]:
        return b
    if not b[1]:
        return a
    if a[0] != b[0]:
        names = {"INT": "Int2LongOpenHashMap", "LONG": "Long2LongOpenHashMap", "FLOAT": "Float2LongOpenHashMap", "DOUBLE": "Double2LongOpenHashMap"}
        raise ValueError(f"Illegal data type for Intermediate Result of MODE aggregation function: {names[a[0]]}, {names[b[0]]}")
    out = {}
    for k, c in a[1] + b[1]:
        kk = _double_compare_key(k)
        out[kk] = (k, out[kk][1] + c) if kk in out else (k, c)
    return (a[0], tuple(out[kk] for kk in sorted(out)))


def mode_final(m, reducer: str = "MIN") -> float:
    """ModeAggregationFunction#extractFinalResult: the key of greatest count; ties go to the lowest key (MIN), the highest (MAX) — in
    Double.compare order — or to the exact sum of the tied keys as doubles, rounded once, over their number (AVG).  -Infinity for an empty map."""
    if reducer not in capi.MODE_REDUCERS:
        raise ValueError("No enum constant org.apache.pinot.core.query.aggregation.function.ModeAggregationFunction.MultiModeReducerType." + reducer)
    if not m[1]:
        return float("-inf")
    top = max(c for _, c in m[1])
    tied = [float(k) for k, c in m[1] if c == top]   # ascending by key
    if reducer == "MIN":
        return tied[0]
    if reducer == "MAX":
        return tied[-1]
    if any(t != t for t in tied) or (float("inf") in tied and float("-inf") in tied):
        return float("nan")
    if float("inf") in tied or float("-inf") in tied:
        return float("inf") if float("inf") in tied else float("-inf")
    try:
        total = math.fsum(tied)   # the exact sum, rounded once
    except OverflowError:
        total = float("inf") if sum(Fraction(t) for t in tied) > 0 else float("-inf")
    return total / len(tied)


def mode_reducer_of(column: str) -> str:
    """the reducer of a MODE's canonical argument list: "x" -> MIN, "x,'AVG'" -> AVG"""
    _, comma, rest = column.partition(",")
    return rest.strip().strip("'") if comma else "MIN"


def histogram_merge(a, b):
    """HistogramAggregationFunction#merge (DoubleVectorOpUtils#vectorAdd): the element-wise sum of two count arrays, what the Java side does
    with the arrays of two segments; arrays of unequal lengths are refused, as vectorAdd's checkState refuses them."""
    if len(a) != len(b):
        raise ValueError(f"The two operand arrays are not of the same size! provided {len(a)}, {len(b)}")
    return tuple(float(x) + float(y) for x, y in zip(a, b))


def with_time_merge(function: str, a, b):
    """FirstWithTimeAggregationFunction#merge / LastWithTimeAggregationFunction#merge over two (value, time) pairs, what the Java side does
    with the pairs of two segments: LAST keeps `a` where a.time >= b.time, FIRST where a.time <= b.time — the first argument wins a tie."""
    if function == "LASTWITHTIME":
        return a if a[1] >= b[1] else b
    return a if a[1] <= b[1] else b


def hll_merge(a: bytes, b: bytes) -> bytes:
    return bytes(max(x, y) for x, y in zip(a, b))


# ----------------------------------------------------------------------------------------------------------------------
# GroupByCombineOperator + IndexedTable: merge per-segment intermediate results keyed by *values*
# (dictionaries are per segment; GroupByCombineOperator.java:132-147 decodes before upserting).
# ----------------------------------------------------------------------------------------------------------------------
def merge_intermediate(function: str, a, b):
    """AggregationFunction#merge for the functions on the path (the *MV forms merge like their single-value forms)."""
    function = capi.MV_TO_SV_FUNCTION.get(function, function)
    if function in ("COUNT", "SUM"):
        return a + b
    if function == "MIN":
        return b if b < a else a
    if function == "MAX":
        return b if b > a else a
    if function == "AVG":
        return (a[0] + b[0], a[1] + b[1])
    if function == "MINMAXRANGE":
        return (min(a[0], b[0]), max(a[1], b[1]))
    if function == "DISTINCTCOUNT":
        return a | b
    if function == "DISTINCTCOUNTHLL":
        return hll_merge(a, b)
    if function in capi.VARIANCE_FUNCTIONS:
        return variance_merge(a, b)
    if function in capi.COVARIANCE_FUNCTIONS:
        return covariance_merge(a, b)
    if function in capi.FOURTH_MOMENT_FUNCTIONS:
        return fourth_moment_merge(a, b)
    if function in capi.WITH_TIME_FUNCTIONS:
        return with_time_merge(function, a, b)
    if function in capi.HISTOGRAM_FUNCTIONS:
        return histogram_merge(a, b)
    if function in capi.MODE_FUNCTIONS:
        return mode_merge(a, b)
    raise ValueError(function)


def extract_final(function: str, v, column: "Optional[str]" = None):
    """AggregationFunction#extractFinalResult (`column`: the aggregation's argument list, which carries a MODE's reducer)."""
    function = capi.MV_TO_SV_FUNCTION.get(function, function)
    if function == "AVG":
        return v[0] / v[1] if v[1] else float("-inf")
    if function == "MINMAXRANGE":
        return v[1] - v[0]
    if function == "DISTINCTCOUNT":
        return len(v)
    if function == "DISTINCTCOUNTHLL":
        return hll_cardinality(v)
    if function in capi.VARIANCE_FUNCTIONS:
        return variance_final(function, v)
    if function in capi.COVARIANCE_FUNCTIONS:
        return covariance_final(function, v)
    if function in capi.FOURTH_MOMENT_FUNCTIONS:
        return skewness_final(v) if function == "SKEWNESS" else kurtosis_final(v)
    if function in capi.WITH_TIME_FUNCTIONS:   # the pair's value
        return v[0]
    if function in capi.MODE_FUNCTIONS:   # a map: its mode under the reducer; a final double (PG_QUERY_FLAG_FINAL_MODE) as it is
        return mode_final(v, mode_reducer_of(column or "")) if isinstance(v, tuple) else v
    if function in capi.HISTOGRAM_FUNCTIONS:   # the array itself (DOUBLE_ARRAY)
        return tuple(float(x) for x in v)
    return v


class GroupByCombineOperator:
    """Host-side merge of per-segment (per-GPU) results: IndexedTable#upsert semantics (key → record, merge per
    aggregation function).  The RCCL variant for identical key spaces lives in pinot_amd.distributed."""

    def __init__(self, blocks: Sequence[ResultsBlock]):
        self.blocks = list(blocks)

    def merge(self) -> Dict[tuple, list]:
        table: Dict[tuple, list] = {}
        fns = [a.function for a in self.blocks[0].query.aggregations]
        for b in self.blocks:
            for key, vals in b.rows().items():
                cur = table.get(key)
                if cur is None:
                    table[key] = list(vals)
                else:
                    table[key] = [merge_intermediate(f, x, y) for f, x, y in zip(fns, cur, vals)]
        return table

    def final(self) -> Dict[tuple, list]:
        aggs = self.blocks[0].query.aggregations
        return {k: [extract_final(a.function, v, a.column) for a, v in zip(aggs, vals)] for k, vals in self.merge().items()}


class GpuInstancePlanMaker:
    """PlanMaker for the accelerated path.  `make_segment_plan_node(segment, query)` returns a callable plan node whose
    run() yields the operator result, or raises NativeError(PG_ERR_UNSUPPORTED) so the caller can fall back to the
    default plan — the contract the Java GpuInstancePlanMaker follows."""

    def __init__(self):
        self.api = capi.gpu_api()

    def load_segment(self, host: HostSegment) -> NativeSegment:
        return NativeSegment(self.api, host)

    def make_segment_plan_node(self, segment: NativeSegment, query):
        qc = parse_sql(query) if isinstance(query, str) else query
        cq = CQuery(qc, tuple(segment.host.columns))
        self.api.call("query_supported", segment.handle, cq.ptr())
        return _SegmentPlanNode(segment, qc)


class _SegmentPlanNode:
    def __init__(self, segment: NativeSegment, qc: QueryContext):
        self.segment = segment
        self.qc = qc

    def run(self) -> ResultsBlock:
        return self.segment.execute(self.qc)
