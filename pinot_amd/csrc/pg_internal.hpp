// Host-side internals of libpinot_gpu.so (below the C ABI in include/pinot_gpu.h).
#pragma once
#include <hip/hip_runtime_api.h>

#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/pinot_gpu.h"
#include "pg_device.h"
#include "pg_side_query.h"

namespace pg {

// ---- errors ------------------------------------------------------------------------------------------------------------
struct Error : std::runtime_error {
  int32_t status;
  Error(int32_t s, const std::string& m) : std::runtime_error(m), status(s) {}
};
[[noreturn]] void fail(int32_t status, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
void set_last_error(const std::string& msg);
const std::string& last_error();

#define PG_HIP(expr)                                                                                   \
  do {                                                                                                 \
    hipError_t _e = (expr);                                                                            \
    if (_e != hipSuccess)                                                                              \
      ::pg::fail(_e == hipErrorOutOfMemory ? PG_ERR_OUT_OF_MEMORY : PG_ERR_DEVICE, "HIP error %s at %s:%d: %s", \
                 hipGetErrorName(_e), __FILE__, __LINE__, #expr);                                      \
  } while (0)

// ---- device memory -------------------------------------------------------------------------------------------------------
// Allocated on the device that is current at alloc() time (every entry point first makes the segment's device current) and
// freed on that same device whatever is current then.
struct DeviceBuffer {
  void* ptr = nullptr;
  size_t size = 0;
  int device = -1;
  DeviceBuffer() = default;
  explicit DeviceBuffer(size_t n, bool zero = false) { alloc(n, zero); }
  DeviceBuffer(const DeviceBuffer&) = delete;
  DeviceBuffer& operator=(const DeviceBuffer&) = delete;
  DeviceBuffer(DeviceBuffer&& o) noexcept : ptr(o.ptr), size(o.size), device(o.device) { o.ptr = nullptr; o.size = 0; }
  DeviceBuffer& operator=(DeviceBuffer&& o) noexcept {
    if (this != &o) { release(); ptr = o.ptr; size = o.size; device = o.device; o.ptr = nullptr; o.size = 0; }
    return *this;
  }
  ~DeviceBuffer() { release(); }
  void alloc(size_t n, bool zero = false);
  void release();
  void upload(const void* src, size_t n, size_t dst_off = 0);
  template <typename T> T* as() const { return reinterpret_cast<T*>(ptr); }
};
template <typename T>
DeviceBuffer upload_vector(const std::vector<T>& v) {
  DeviceBuffer b(v.empty() ? sizeof(T) : v.size() * sizeof(T));
  if (!v.empty()) b.upload(v.data(), v.size() * sizeof(T));
  return b;
}

// ---- segment ----------------------------------------------------------------------------------------------------------------
struct Column {
  std::string name;
  int32_t data_type = 0;
  int32_t fwd_encoding = 0;
  bool has_dictionary = false;
  int32_t cardinality = 0;
  int32_t bits = 0;
  bool is_sorted = false;
  int32_t dict_bytes_per_value = 0;
  // host copies needed by the planner
  std::vector<uint8_t> dict_host;               // big-endian dictionary bytes (binary search, as the reference does)
  std::vector<int32_t> sorted_start, sorted_end; // SortedIndexReaderImpl pairs
  // device
  int32_t col_kind = PG_COL_FIXED_BIT;          // layout the kernels see
  int32_t val_type = PG_V_I32;
  DeviceBuffer fwd_dev;                         // doc 0 at offset 0, padded to whole tiles
  DeviceBuffer dict_dev;                        // native-endian values
  // inverted index (BitmapInvertedIndexReader): containers re-laid out 16-byte aligned
  bool has_inverted = false;
  std::vector<PgContainer> descs_host;
  std::vector<uint32_t> posting_begin;          // cardinality + 1 offsets into descs_host
  std::vector<int64_t> posting_card;            // docs per dictId (exact: planning estimates filter selectivity from it)
  DeviceBuffer containers_dev, descs_dev;
  // bit-sliced range index (BitSlicedRangeIndexReader over a RoaringBitmap RangeBitmap): one container per (2^16-row chunk, slice)
  bool has_range_index = false;
  int32_t ri_slices = 0, ri_chunks = 0;
  int64_t ri_min = 0;                            // stored value = value - ri_min (raw INT / LONG), dictId, or FPOrdering ordinal
  uint64_t ri_bytes = 0;
  DeviceBuffer ri_containers_dev, ri_descs_dev;
  uint64_t fwd_bytes_logical = 0;               // bytes of the forward index proper (for algorithmic byte accounting)
  // value statistics behind exact SUMs (fixed-point scale, digit count), computed once at registration
  int32_t fx_exp = 0;                           // FLOAT / DOUBLE: every finite |value| < 2^fx_exp (a multiple of 16)
  bool has_nonfinite = false;                   // NaN / +-Inf among the values: SUM falls back to IEEE double accumulation
  uint64_t max_abs_int = 0;                     // LONG: largest |value|
  bool has_int_range = false;                   // raw INT / LONG: smallest and largest value (tuple packing of the partition pipeline)
  int64_t int_min = 0, int_max = 0;
  // narrow image of a single-value raw INT column whose range needs <= 24 bits (pg_segment.cpp, narrow_image): value - int_min in img_bits
  // (8 / 16 / 24) bits, byte planes per wave tile, beside fwd_dev; built on the device at first use by pg_fast_i32range_s / _st, under the
  // segment's lock.  img_state: 0 not tried, 1 built, 2 not to be had (not eligible, or no memory: the plans keep the raw layout)
  DeviceBuffer img_dev;
  int32_t img_bits = 0;
  int32_t img_state = 0;
  bool dict_affine = false;                     // INT / LONG dictionary whose values are base + step x dictId (ids, dense enumerations)
  int64_t dict_base = 0, dict_step = 0;
  uint64_t dict_hash = 0;                       // FNV-1a of the dictionary bytes: tables merge element-wise only over equal dictionaries
  std::map<int, DeviceBuffer> hll_luts;         // per log2m: (register index | rank << 16) of every dictionary value
  // virtual dictionary of a raw group-by column (pg_vdict.hip): a Column of bit-packed ids whose `vdict_keys` are the distinct values
  // (order-preserving 64-bit keys, ascending); built at first use, under the segment's lock
  std::unique_ptr<Column> vdict;
  std::vector<uint64_t> vdict_keys;
  int vdict_kind = -1;                          // 0 INT, 1 LONG, 2 FLOAT, 3 DOUBLE (set on the id column)
  uint64_t vdict_hash = 0;
  int32_t hll_log2m = 0;                        // PG_COL_HLL_REGS: log2m of the serialized HyperLogLogs
  // multi-value dictionary column (FixedBitMVForwardIndexReader): fwd_dev holds the dictIds of all docs back to back (the bit stream
  // of the index's raw-data section), mv_offsets_dev the first entry of every doc (numDocs + 1 ints: the row-start bitmap expanded
  // once at registration, instead of the reader's chunk-offset + bitmap walk per doc)
  // raw STRING / BYTES column (VarByteChunkSVForwardIndexReader): fwd_dev = the values back to back (chunk headers dropped at
  // registration), vb_offsets_dev = int64 [numDocs + 1]
  DeviceBuffer vb_offsets_dev;
  uint64_t vb_total_bytes = 0;
  // ... and, on its virtual dictionary (vdict_kind 4): the distinct values back to back in id order + offsets (cardinality + 1)
  std::vector<uint8_t> vdict_bytes;
  std::vector<int64_t> vdict_bytes_off;
  bool is_mv = false;
  // raw (no-dictionary) multi-value column (FixedByteChunkMVForwardIndexReader): the values are turned into a dictionary-encoded
  // multi-value column ONCE at registration — sorted distinct values + bit-packed ids in the FixedBitMV layout — kept in `vdict`
  // (complete at registration, unlike a single-value column's lazily built one); the planner resolves the column to it for filters,
  // group keys and aggregation sources, and hands the group keys back as values.  has_dictionary stays false on THIS column: the
  // dictionary-only operators (NonScanBasedAggregationOperator) do not apply to a raw column.
  bool raw_mv = false;
  Column* public_col = nullptr;                 // on the internal twin: the column the segment knows by name (statistics count it once)
  int32_t total_entries = 0;                    // ColumnMetadata#getTotalNumberOfEntries
  int32_t max_entries_per_doc = 0;              // ColumnMetadata#getMaxNumberOfMultiValues
  DeviceBuffer mv_offsets_dev;
  std::vector<int32_t> mv_offsets_host;         // the same offsets for the host-side statistics automaton (pg_filter_stats.cpp)
  // a DERIVED key column (pg_exprkey.cpp): GROUP BY / DISTINCT over an arithmetic expression.  DOUBLE, no dictionary, no forward index of its
  // own (fwd_dev stays empty: nothing may read it) — only `vdict`, built from pg_expr_keys' output; `name` is the expression's text.  Non-empty
  // exactly on such a column: the distinct operand columns, which statistics count in its place.
  std::vector<Column*> expr_operands;
};

struct CompiledPlan;
struct StarTree;

struct Segment {
  std::string name;
  int device = 0;                               // HIP device ordinal whose HBM holds the segment (segment -> GPU map)
  int32_t total_docs = 0;
  int32_t n_tiles = 0;
  std::map<std::string, std::unique_ptr<Column>> columns;
  std::shared_ptr<int> alive = std::make_shared<int>(1);   // results keep a weak reference: their schema points into the columns' host dictionaries
  uint64_t device_bytes = 0;
  std::mutex mu;
  std::unordered_map<std::string, std::shared_ptr<CompiledPlan>> plan_cache;
  std::vector<std::unique_ptr<StarTree>> star_trees;   // IndexSegment#getStarTrees
  // doc-id bitmaps handed over as portable RoaringBitmaps, kept as one-posting inverted indexes (the kernels' posting leaf):
  std::map<std::string, std::shared_ptr<Column>> null_vectors;   // NullValueVectorReader#getNullBitmap per column
  std::shared_ptr<Column> queryable_doc_ids;                     // SegmentContext#getQueryableDocIdsSnapshot
  // per expression text of an aggregation (pg_exec_expr.hip): the bounds pass's answer over ALL docs, filled under `mu`
  // (the pass itself runs outside it); at most 256 entries, emptied when full
  struct ExprBounds {
    int32_t exp = 0;             // every finite |value| < 2^exp
    bool has_nonfinite = false;  // a NaN / Inf occurs (division by zero, overflow): such a query stays with the Java plan
  };
  std::map<std::string, ExprBounds> expr_bounds;
  // per expression text of a GROUP BY / DISTINCT key (pg_exprkey.cpp): its derived column.  Shared-owned — plans hold Column*, so a plan
  // compiled against a column that was evicted since keeps it alive (CompiledPlan::pinned).  At most PG_MAX_DERIVED_KEYS per segment, the
  // one used longest ago goes first; read and filled under `mu`, the full-segment passes that build a column run outside it.
  struct DerivedKey {
    std::shared_ptr<Column> col;
    uint64_t last_used = 0;
    uint64_t bytes = 0;          // its share of device_bytes
  };
  std::map<std::string, DerivedKey> derived_keys;
  uint64_t derived_clock = 0;
  Column* find(const char* name);
  Segment();
  ~Segment();
};

// StarTreeV2 (pinot-segment-local/.../startree/v2/store/StarTreeLoaderUtils.java:53-128): the tree (host), and the star-tree
// docs as a doc space of their own — dimension columns (fixed-bit dictIds of the parent's dictionaries) and one column per
// function-column pair, pinned in HBM like any other column.
struct StarTreePair {
  int32_t function = 0;      // pg_agg_function
  std::string column;        // "*" for COUNT
  Column* col = nullptr;     // column of `space` named AggregationFunctionColumnPair#toColumnName
  Column* col_b = nullptr;   // AVG / MINMAXRANGE pairs (BYTES: AvgPair / MinMaxRangePair) are split in two raw columns: col = sum / min, col_b = count / max
};
struct StarTree {
  Segment space;
  std::vector<std::string> dims;
  std::vector<StarTreePair> pairs;
  std::vector<int32_t> nodes;   // 7 ints per node (OffHeapStarTreeNode), native endian
  int32_t n_nodes = 0;
  int pair_index(int32_t function, const char* column) const;
};

void segment_add_column(Segment& seg, const pg_column_desc& d);
void ensure_virtual_dictionary(Segment& seg, Column& c);            // pg_vdict.hip
// ... and the virtual dictionary of a key column that is an expression (pg_vdict.hip): pg_expr_keys over all docs, then the steps a stored
// raw DOUBLE column takes.  seg.mu is NOT needed (it reads registered columns only); `id_bytes`: the HBM the bit-packed ids keep.
std::unique_ptr<Column> expression_virtual_dictionary(Segment& seg, const std::string& text, const PgExprArgs& args, uint64_t* id_bytes);
// ... and of one that is a time-bucket transform: pg_time_keys over all docs, then the steps a stored raw LONG column takes
std::unique_ptr<Column> time_virtual_dictionary(Segment& seg, const std::string& text, const PgTimeKeyArgs& args, uint64_t* id_bytes);
int64_t vdict_value_of_key(uint64_t key, int kind, double* as_double);   // the value behind an order-preserving key (FLOAT / DOUBLE: IEEE double bits)
double limbs_to_double(const int64_t* limbs, int n_limbs, int q);   // sum_j limbs[j] * 2^(32 j + q), correctly rounded (pg_plan.cpp)
void segment_add_star_tree(Segment& seg, const pg_star_tree_desc& d);
// ZSTANDARD / GZIP chunks: host decode at registration (pg_host_codecs.cpp)
bool host_codec(int compression);
void host_decompress_fixed_byte_chunks(int compression, const uint8_t* file, const std::vector<uint64_t>& offs, uint32_t chunk_bytes,
                                       uint64_t total_bytes, uint8_t* dst_device, const char* column);
// one var-byte chunk of any supported ChunkCompressionType -> its bytes (at most `capacity`); PG_ERR_UNSUPPORTED / INVALID_ARGUMENT otherwise
std::vector<uint8_t> host_decompress_chunk(int compression, const uint8_t* src, uint64_t n, uint64_t capacity, const char* column);
void decompress_fixed_byte_chunks(int compression, const uint8_t* file, const std::vector<uint64_t>& offs, uint32_t chunk_bytes,
                                  uint64_t total_bytes, uint8_t* dst, const char* column);
void segment_set_null_vector(Segment& seg, const char* column, const void* roaring, uint64_t size);
void segment_set_range_index(Segment& seg, const char* column, const void* bytes, uint64_t size);
void segment_set_queryable_doc_ids(Segment& seg, const void* roaring, uint64_t size);

// ---- predicate evaluation (host): PredicateEvaluatorProvider & factories ---------------------------------------------------
struct PredEval {
  int32_t pred_type = 0;
  bool dictionary_based = false;
  bool always_true = false, always_false = false;
  bool exclusive = false;
  // dictionary based
  bool is_range = false;
  int32_t start_dict_id = 0, end_dict_id = 0;   // [start, end)
  std::vector<uint8_t> match;                   // per dictId
  std::vector<int32_t> matching, non_matching;  // ascending
  // raw based
  int32_t data_type = 0;
  int64_t lo_i = 0, hi_i = 0;
  double lo_d = 0, hi_d = 0;
  std::vector<int64_t> set_i;
  std::vector<double> set_d;
};
PredEval make_pred_eval(const pg_filter_node& p, const Column& col);

// ---- host-side doc-id bitmaps (pg_filter_stats.cpp: numEntriesScannedInFilter of leapfrogged filter shapes) ---------------------
struct HostBits {
  std::vector<uint64_t> w;   // ceil(n_docs / 64) + 1 words, bits beyond n_docs clear
  int64_t n_docs = 0;
  int64_t next_set(int64_t from) const;   // first set bit >= from, -1 when none
  int64_t cardinality() const;
  void resize_for(int64_t docs);
  void add_range(int64_t lo, int64_t hi_inclusive);
};
struct FilterOp;
using StatLeafBits = std::unordered_map<const FilterOp*, HostBits>;
// max_next >= 0: the count at the point where the consumer stopped after that many next() calls (a selection's LIMIT), not drained
int64_t emulate_entries_scanned_in_filter(const FilterOp& root, const StatLeafBits& leaves, int32_t n_docs, int64_t max_next = -1);
// The same count without the bitmaps leaving HBM, for the shapes whose automaton decomposes into tiles (pg_filter_stats_tiles.h): an AND whose
// children are scans, index-based leaves and flat ORs of both, under any nest of drained ORs / NOTs.  `filter_stats_on_device`: does the plan's
// tree have such a shape; `entries_scanned_on_device`: the count, given every Scan / Inverted / RangeIdx leaf's match bitmap on the device
// (`arena`: scratch the call may grow; it synchronizes `stream` once, for the 8-byte answer).
using StatLeafWords = std::unordered_map<const FilterOp*, const uint64_t*>;
bool filter_stats_on_device(const FilterOp& root, int32_t n_docs);
int64_t entries_scanned_on_device(const FilterOp& root, const StatLeafWords& leaves, int32_t n_docs, DeviceBuffer& arena, void* hip_stream);

// ---- compiled plan ------------------------------------------------------------------------------------------------------------
// Expr: ExpressionFilterOperator — a predicate over an arithmetic expression (pg_expr.h); its doc set is computed when the plan is compiled
enum class OpKind { Empty, MatchAll, Scan, Inverted, Sorted, And, Or, Not, Bitmap, RangeIdx, Expr };

struct FilterOp {
  OpKind kind = OpKind::Empty;
  PredEval eval;
  Column* col = nullptr;
  std::shared_ptr<Column> bitmap_col;        // Inverted over a docId bitmap of the segment (null vector, queryableDocIds): keeps it alive
  std::vector<std::unique_ptr<FilterOp>> children;
  std::vector<int32_t> range_lo, range_hi;   // Bitmap (BitmapBasedFilterOperator): ascending disjoint inclusive docId ranges
  // Expr: the leaf's doc set as match words in HBM (the layout PG_F_PUSH_WORDS reads: one dword per 32 docs, whole wave tiles), computed once
  // by pg_expr_pred and kept with the plan through its operator tree (CompiledPlan::root_op); its distinct operand columns
  std::shared_ptr<DeviceBuffer> expr_words;
  std::vector<Column*> expr_cols;
};
using OpPtr = std::unique_ptr<FilterOp>;
OpPtr make_filter_op(OpKind k);
OpPtr and_operator(std::vector<OpPtr> ops);
OpPtr or_operator(std::vector<OpPtr> ops);
OpPtr not_operator(OpPtr child);
OpPtr leaf_operator(PredEval ev, Column* col, int32_t predicate_type);
// StarTreeUtils#createStarTreeBasedProjectOperator + StarTreeFilterOperator: the filter over the star-tree docs when the
// query is fit for the star-tree, nullptr otherwise
OpPtr star_tree_filter(Segment& seg, StarTree& st, const pg_filter_node* filter, const pg_query& q);

enum class ResultKind { Long, Double, AvgPair, MinMaxPair };

static const int32_t kCountFromStats = -2;   // AggOut::op_a/op_b, CompiledPlan::exist_op: the match count, not a table op

struct AggOut {          // how one requested aggregation maps onto accumulator ops
  int32_t function;
  int32_t op_a = -1, op_b = -1;   // indices into ops (AVG: sum,count; MINMAXRANGE: min,max; COUNT: count op)
  bool is_float = false;
  int32_t sum_limbs = 0;           // SUM / AVG: > 0: the sum is the fixed-point number sum_j ops[op_a + j] * 2^(32 j + fx_q), rounded once
  int32_t fx_q = 0;
  bool star_count = false;         // COUNT over a star-tree: op_a is the SUM of count__* (CountAggregationFunction.java:99-106)
  int32_t aux = -1;                // DISTINCTCOUNT / DISTINCTCOUNTHLL: index into PgQueryPlan::aux
  int32_t log2m = 0;
  Column* aux_col = nullptr;
};

struct CompiledPlan {
  PgQueryPlan dev{};                 // template; per-execution pointers are patched in
  std::vector<DeviceBuffer> keep;    // device allocations referenced by dev
  std::vector<std::shared_ptr<Column>> pinned;   // doc-id bitmaps (null vectors, queryableDocIds snapshot) the program reads
  int32_t n_stat_slots = 1;
  // candidates of the scan leaf per 1000 docs as the last execution counted them (-1: never run) — pg_fast_i32range_s streams every column
  // whole, pg_fast_i32range_p skips the quads without candidates: which of the two runs follows what the plan's filter lets through
  mutable std::atomic<int> observed_candidate_permille{-1}, observed_match_permille{-1};
  mutable std::atomic<uint64_t> last_used{0};   // the segment's plan cache evicts the plans used longest ago (pg_exec.hip, get_plan)
  int64_t full_scan_entries = 0;     // entries contributed by unmasked scans whose count is known (numDocs each)
  bool stats_exact = true;           // the kernels' own counters give numEntriesScannedInFilter (flat AND shapes, drained ORs)
  mutable std::atomic<int> stats_on_device{-1};   // !stats_exact: can the tile automaton count it on the device (filter_stats_on_device; -1: not judged yet)
  // otherwise: the physical filter tree and one filter-only plan per Scan / Inverted leaf — their match bitmaps feed the iterator
  // automaton of pg_filter_stats.cpp, which reproduces the reference's count exactly
  std::unique_ptr<FilterOp> root_op;
  std::vector<std::pair<const FilterOp*, std::shared_ptr<CompiledPlan>>> stat_leaves;
  int32_t fast_scan_bits = 0;        // bits per value of the single scan leaf's column (pg_dict_count_* is chosen by it)
  bool always_empty = false;
  bool match_all = false;            // the filter is MatchAllFilterOperator: no filter pass in front of the partition pipeline
  int32_t n_projected_columns = 0;
  int64_t algorithmic_bytes = 0;
  // pg_fast_i32range_s / _st: the raw INT scan column and the value column where their ranges allow a narrow image (Column::img_dev), else null;
  // the executor asks for the images when it launches that kernel (narrow_image) and falls back to the raw layout column by column
  Column* spec_scan_col = nullptr;
  Column* spec_val_col = nullptr;
  // aggregation
  std::vector<AggOut> aggs;
  std::vector<Column*> group_cols;
  std::vector<int32_t> group_cards;
  size_t lds_bytes = 0;
  int32_t num_groups_limit = 0;
  // segment-level group trim (GroupByOperator.java:120-133): the ORDER BY expressions and trimSize = max(5 x limit, minSegmentGroupTrimSize);
  // 0: no trim.  Applied at result assembly (pg_exec.hip trim_groups), on the device first where the table allows (device_trim).
  std::vector<pg_order_by> order_by;
  int32_t trim_size = 0;
  // result assembly, dense key spaces in which EVERY group exists (a star-tree's pre-aggregated docs, low-cardinality group-bys): the groups'
  // dictIds per group-by column are a function of the plan alone — decoded once, copied afterwards (12 800 groups x 4 columns were ~20 us of the
  // star-tree route's 55 us of assembly).  Filled under full_keys_once by the first result that needs them.
  mutable std::once_flag full_keys_once;
  mutable std::vector<std::vector<int32_t>> full_keys;
  int32_t exist_op = 0;              // accumulator whose value tells whether a group was touched
  bool raw_group = false;            // the single group-by column is a raw INT / LONG column: keys are values (hash group-by)
  std::vector<Column*> group_vdict;  // per group-by column: its virtual dictionary (raw column grouped through ids), or null
  int32_t first_doc_op = -1;         // MIN(docId) per group, present when the key space exceeds numGroupsLimit
  int32_t fast_filter = -2;          // -2: interpreter kernel; -1: index-only filter; >= 0: ScanKind of the one scan leaf
  bool fast_agg = true;              // aggregation fits the fast kernels (or there is none)
  bool aux_in_lds = false;           // DISTINCTCOUNT / HLL states live in the workgroups' LDS (merged by pg_reduce_aux_kernel)
  bool digit_ops = false;            // some SUM runs on digit accumulators (PgAccValueKind): the *d kernels
  bool wide_agg = false;             // LDS-table aggregation over wide group columns / 64-bit sources: the *_w kernels
  DeviceBuffer ops_dev;
  std::vector<size_t> aux_bytes;     // bytes of each auxiliary region (256-byte multiples)
  int32_t star_tree_index = -1;      // the star-tree whose doc space the plan runs on
  int32_t space_docs = 0;            // docs of that doc space (the segment's own when no star-tree is used)
  // what pg_result_merge / pg_result_all_reduce check beyond the layout: the dictionaries behind dictId-indexed state (group-by
  // columns, DISTINCTCOUNT sets, dictionary-fed HyperLogLogs) must be equal, and the summed accumulators must still hold the sum
  std::vector<uint64_t> dict_hashes;
  uint64_t sum_max_abs = 0;          // largest |value| an int64 SUM accumulator adds per doc (0: none)
  bool has_digit_sums = false;       // 32-bit digits summed in int64 accumulators: safe below 2^31 docs in total
  bool non_scan_based = false;       // NonScanBasedAggregationOperator: answered from dictionaries on the host
};

void hll_registers_of_dictionary(Column& c, int log2m, uint8_t* regs);
double dictionary_value_as_double(const Column& c, int32_t dict_id);
// Expression leaves of a filter (a pg_filter_node whose column spells an expression): expr_leaf_specs checks and resolves them under seg.mu
// (every refusal of the leaf comes from here), expr_leaf_run is the pass over all docs that produces a leaf's match words — get_plan runs it
// WITHOUT the segment's lock, as the bounds pass of expressions inside aggregations does, and hands the words to compile_plan.
#define PG_MAX_EXPR_LEAVES 4   // per filter: each costs numDocs / 8 bytes of HBM per cached plan
struct ExprLeafSpec {
  const pg_filter_node* node = nullptr;
  PgExprArgs args;     // expression 0: the program; srcs: the operand columns
  PgExprPred pred;     // kind, bounds (set / out: filled by the pass)
  std::vector<uint64_t> set_bits;   // IN / NOT_IN: Double.doubleToLongBits of the values
  std::vector<Column*> cols;
  std::shared_ptr<DeviceBuffer> words;   // after expr_leaf_run
};
bool filter_has_expression(const pg_filter_node* filter);
Column* expr_operand_column(Segment& seg, const std::string& name, bool null_handling);   // an expression's operand, checked (seg.mu held)
void expr_fill_src(PgValueSrc& S, const Column& c);
// The operand columns of an aggregation's expression, checked, in the program's order.  A program that holds a CASE (pg_expr.h) is resolved
// against their types: a literal compared with a STRING column becomes its dictId, a FLOAT-typed CASE narrows its INT / LONG literals, and
// what the program cannot restate is refused.  seg.mu held.
struct ExprProgram;
std::vector<Column*> expr_resolve_operands(Segment& seg, ExprProgram& prog, bool null_handling);
std::vector<ExprLeafSpec> expr_leaf_specs(Segment& seg, const pg_filter_node* filter, int32_t flags);   // seg.mu held
void expr_leaf_run(Segment& seg, ExprLeafSpec& leaf);                                                    // seg.mu not needed
// `expr_leaves`: the filter's expression leaves with their words (a filter that holds one and finds no words is PG_ERR_INTERNAL)
std::shared_ptr<CompiledPlan> compile_plan(Segment& seg, const pg_filter_node* filter, const pg_query* query, int32_t flags = 0,
                                           const std::vector<ExprLeafSpec>* expr_leaves = nullptr);   // flags: of a filter-only plan (query == nullptr)
// ---- arithmetic expressions as GROUP BY / DISTINCT keys (pg_exprkey.cpp) -------------------------------------------------------
#define PG_MAX_DERIVED_KEYS 16   // derived key columns kept per segment
#define PG_MAX_EXPR_KEYS 4       // expression keys of one query, arithmetic and time-bucket ones together
// Every entry point that plans a query opens one over it before anything else (execute_query, pg_query_supported): it checks the query's
// expression keys under seg.mu (every refusal of such a key comes from here), builds the derived columns the segment does not hold WITHOUT
// the lock, inserts them under it again, and keeps the query's columns alive and findable for the calling thread while it lives.
class ExprKeyScope {
 public:
  ExprKeyScope(Segment& seg, const pg_query& q);
  ~ExprKeyScope();
  ExprKeyScope(const ExprKeyScope&) = delete;
  ExprKeyScope& operator=(const ExprKeyScope&) = delete;
 private:
  size_t mark_;
};
// THE resolution of a group-by / DISTINCT text (seg.mu held): the derived column of an expression (`*keep` then shares its ownership: a plan
// or shape that stores the pointer stores `keep` with it), else seg.find(text) — nullptr when the segment has no such column.
Column* group_key_column(Segment& seg, const char* text, std::shared_ptr<Column>* keep);
// the columns statistics count for a resolved key column: the operands of a derived column, else the column itself
inline const std::vector<Column*> key_columns_read(Column* c) { return c->expr_operands.empty() ? std::vector<Column*>{c} : c->expr_operands; }
// SELECT DISTINCT (PG_QUERY_FLAG_DISTINCT): the checked query and its key space (pg_plan.cpp); execute_distinct runs it (pg_exec.hip)
struct DistinctShape {
  std::vector<Column*> cols;       // per DISTINCT column: the column of fixed-bit ids (its own dictIds, or its virtual dictionary's ids)
  std::vector<Column*> vdicts;     // per DISTINCT column: the virtual dictionary of a raw column, or null
  std::vector<uint64_t> mult;      // weight of the column's digit in the key (order-by columns most significant, in ORDER BY order)
  std::vector<int32_t> desc;       // the digit is cardinality - 1 - id
  uint64_t key_space = 1;          // product of the cardinalities (<= 2^32)
  bool dict_only = false;          // DictionaryBasedDistinctOperator: no filter, one dictionary-encoded column
  bool ordered = false;            // ORDER BY present
  std::vector<std::shared_ptr<Column>> keep;   // the derived columns among `vdicts`' owners (expression keys)
  int n_read = -1;                 // with an expression key: the distinct columns the keys name, operands included (-1: one per DISTINCT column)
};
DistinctShape distinct_shape(Segment& seg, const pg_query& q);
// selection queries (PG_QUERY_FLAG_SELECTION): the checked output columns and ORDER BY (pg_plan.cpp); execute_selection runs them (pg_exec.hip)
struct SelectionShape {
  std::vector<Column*> cols;                 // per output column (extractExpressions order)
  std::vector<std::pair<int, bool>> order;   // the distinct ORDER BY columns: (output column, ascending), most significant first
  int key_bits = 0;                          // width of the order-space key (<= 64)
  int n_distinct = 0;                        // distinct output columns (ProjectOperator#getNumColumnsProjected)
};
SelectionShape selection_shape(Segment& seg, const pg_query& q);
std::vector<std::pair<const FilterOp*, std::shared_ptr<CompiledPlan>>> stat_leaf_plans(Segment& seg, const CompiledPlan& P);
std::string query_signature(const pg_filter_node* filter, const pg_query* query, int32_t flags = 0);

// ---- results --------------------------------------------------------------------------------------------------------------------
// Page-locked host blocks for result copies that a result may keep (pooled: hipHostMalloc costs more than a query)
struct PinnedBlock {
  void* ptr = nullptr;
  size_t size = 0;
  ~PinnedBlock();   // back to the pool
};
std::shared_ptr<PinnedBlock> acquire_pinned(size_t bytes);
struct AggResult {
  int32_t kind = PG_RESULT_DOUBLE;
  std::vector<double> d[4];   // the third plane: PG_RESULT_COVARIANCE_TUPLE and PG_RESULT_FOURTH_MOMENT, the fourth: PG_RESULT_FOURTH_MOMENT only
  std::vector<int64_t> l[2];
  std::vector<int32_t> set_sizes, set_ids;   // PG_RESULT_DICTID_SET: per group sizes, concatenated ascending dictIds
  int32_t set_value_kind = -1;               // PG_RESULT_VALUE_SET (a raw column through its virtual dictionary): 0 INT, 1 LONG (values in l[0]), 2 FLOAT, 3 DOUBLE (in d[0]; l[0] the IEEE bits), parallel to set_ids
  std::vector<uint8_t> hll;                  // PG_RESULT_HLL: num_groups * 2^log2m registers, or — big states —
  // the registers stay where the device wrote them: a page-locked block shared with the result (copying 3.3 MB of freshly DMA'd,
  // cache-cold bytes costs more than the kernel that produced them); group i's registers = hll_regs + hll_gids[i] * hll_stride
  std::shared_ptr<struct PinnedBlock> hll_block;
  const uint8_t* hll_regs = nullptr;
  int64_t hll_stride = 0;
  std::vector<int64_t> hll_gids;
  int32_t log2m = 0;
  // PG_RESULT_VARIANCE_TUPLE (VAR_POP / VAR_SAMP / STDDEV_POP / STDDEV_SAMP): l[0] = count, d[0] = sum, d[1] = m2
  // PG_RESULT_COVARIANCE_TUPLE (COVAR_POP / COVAR_SAMP): d[0] = sumX, d[1] = sumY, d[2] = sumXY, l[0] = count
  // PG_RESULT_FOURTH_MOMENT (SKEWNESS / KURTOSIS): l[0] = n, d[0] .. d[3] = m1 .. m4
  // PG_RESULT_DOUBLE_ARRAY (HISTOGRAM): set_sizes = numBins for every group, d[0] = the groups' counts back to back (group-major)
  // PG_RESULT_VALUE_TIME_PAIR (FIRSTWITHTIME / LASTWITHTIME): l[0] = time; l[1] = the value in its declared type — an INT / LONG value, or the
  // raw IEEE bits of a FLOAT (32, zero-extended) / DOUBLE —, d[0] = a FLOAT / DOUBLE value (the FLOAT widened exactly); `value_type` the
  // declared type (pg_data_type: the data table's object type and the width of its value)
  int32_t value_type = -1;
  // PG_RESULT_VALUE_COUNTS (PERCENTILE): set_sizes = runs per group, d[0] = the runs' values (ascending under Double.compare within a group),
  // l[0] = their counts; `param` is the aggregation's p (also kept on a final PG_RESULT_DOUBLE: the data table names the column by it)
  double param = 0;
  // PG_RESULT_VALUE_COUNT_MAP (MODE): set_sizes = entries per group, ascending by key; l[0] = the counts; `set_value_kind` the column's stored
  // type (0 INT, 1 LONG: the keys exactly in l[1]; 2 FLOAT, 3 DOUBLE: the keys in d[0], a FLOAT widened exactly)
};
// What pg_result_merge / pg_result_all_reduce need to merge two results of the same query and to re-assemble the groups:
// the dense accumulator table [n_ops][G] + the statistics counters + the DISTINCTCOUNT / HLL regions, left in HBM.
// The key space of a table merged BY VALUE across segments whose group-by dictionaries differ (pg_comm.cpp, union_key_space): per group-by
// column the sorted union of the ranks' dictionaries — kept as a virtual dictionary (Column::vdict_kind / vdict_keys / vdict_bytes), so the
// assembly hands the groups' VALUES over as it does for raw group-by columns — and the dense layout over the unions' cardinalities
// (column 0 least significant, as in the plan's own key space).
struct UnionKeys {
  std::vector<std::unique_ptr<Column>> dicts;
  std::vector<int32_t> cards;
  std::vector<int64_t> mults;
  int64_t n_groups = 1;
};
struct DeviceTable {
  std::shared_ptr<CompiledPlan> plan;
  std::unique_ptr<UnionKeys> keys;   // set once the table has been re-keyed by pg_result_all_reduce (null: the plan's own key space)
  int device = 0;
  int32_t n_group_by = 0, n_aggregations = 0;
  int64_t n_out = 0;            // n_ops * G int64 slots, followed by PG_MAX_STATS statistics counters
  size_t aux_total = 0;         // bytes of the merged auxiliary regions (replica 0 .. n_rep-1 of every op)
  DeviceBuffer table, aux;
  int64_t full_scan_entries = 0;   // summed over the merged segments
  int64_t num_total_docs = 0;
  int64_t tail_host[2] = {0, 0};   // source of the asynchronous copy of the two above behind the statistics counters
  // overflow guards of the summed accumulators, carried by the TABLE (a merged table folds segments with different value ranges:
  // the plan of its first segment no longer bounds what it holds): largest |value| an int64 SUM adds per doc over every segment
  // folded in so far, and whether 32-bit digits are summed in int64 accumulators
  uint64_t sum_max_abs = 0;
  bool has_digit_sums = false;
};
// What a data table needs to know about a result column (pg_datatable.cpp): the name, the column's stored type and its dictionary on
// the host (a pointer into the segment's Column: the segment outlives its results)
struct ResultColumn {
  std::string name;                 // group-by column / the aggregation's argument ("*" for COUNT)
  int32_t data_type = 0;            // pg_data_type of the column
  int32_t function = -1;            // pg_agg_function (aggregations)
  const uint8_t* dict = nullptr;    // big-endian dictionary values, dict_width bytes each
  int32_t dict_width = 0;
};
// Result::merged_elsewhere, one bit per side path
enum MergedElsewhere : uint32_t {
  MERGED_PERCENTILE = 1u << 0, MERGED_EXPRESSION = 1u << 1, MERGED_VARIANCE = 1u << 2, MERGED_FOURTH_MOMENT = 1u << 3, MERGED_COVARIANCE = 1u << 4,
  MERGED_WITH_TIME = 1u << 5, MERGED_HISTOGRAM = 1u << 6, MERGED_MODE = 1u << 7,
};
struct Result {
  std::vector<ResultColumn> schema_keys, schema_aggs;
  std::weak_ptr<int> schema_segment;   // the segment whose dictionaries the schema points into (pg_result_data_table_v4 refuses once it is destroyed)
  bool schema_null_handling = false;   // enableNullHandling: COUNT(col) keeps its argument in the column name (CountAggregationFunction.java:64-66)
  std::unique_ptr<DeviceTable> dev;    // PG_QUERY_FLAG_KEEP_DEVICE_TABLE
  int32_t num_groups = 0;
  std::vector<std::vector<int32_t>> group_dict_ids;
  // no-dictionary group-by columns: per column the key type (PG_GROUP_KEY_*) and, for value keys, the groups' values (LONG values,
  // or the IEEE bits of DOUBLE values); group_dict_ids[col] stays empty for them
  std::vector<int32_t> group_key_type;
  std::vector<std::vector<int64_t>> group_values;
  std::vector<std::vector<uint8_t>> group_bytes;        // PG_GROUP_KEY_BYTES_VALUES: the groups' values back to back,
  std::vector<std::vector<int64_t>> group_bytes_off;    //   offsets (num_groups + 1)
  std::vector<AggResult> aggs;
  // PG_QUERY_FLAG_NULL_HANDLING: per aggregation / per group-by column, 1 where the group's result / key is NULL (empty vector: none is)
  std::vector<std::vector<uint8_t>> agg_nulls, key_nulls;
  bool null_handling = false;   // the query ran with PG_QUERY_FLAG_NULL_HANDLING (its data table carries the columns' null bitmaps)
  bool distinct = false;        // PG_QUERY_FLAG_DISTINCT: the groups are the distinct tuples, no aggregation (never merged in the library)
  bool selection = false;       // PG_QUERY_FLAG_SELECTION: the groups are the selected rows (never merged in the library)
  // MERGED_* bits: the side aggregations the query carried.  Their results merge on the Java side, never in the library (pg_api.cpp words
  // the refusals): a PERCENTILE's lists by value; an aggregation over an expression because the scale of its sums differs per segment; the
  // variance, SKEWNESS / KURTOSIS and covariance tuples by VarianceTuple#apply, PinotFourthMoment#combine and CovarianceTuple#apply; the
  // FIRSTWITHTIME / LASTWITHTIME pairs with the functions' own merge; the HISTOGRAM arrays by DoubleVectorOpUtils#vectorAdd; a MODE's maps by
  // value (the per-key sum of ModeAggregationFunction#merge)
  uint32_t merged_elsewhere = 0;
  pg_exec_stats stats{};
};
struct DocIdSet {
  int device = 0;
  int32_t num_docs = 0;
  int64_t cardinality = 0;
  DeviceBuffer words;          // tile padded
  std::vector<uint32_t> tile_counts;
  pg_exec_stats stats{};
};

// cancellation token (pg_cancel_*): set by any thread, polled by the executing one
struct CancelToken { std::atomic<int> requested{0}; };

// execution (pg_exec.hip)
void device_init(int ordinal);          // pg_init: validates + selects the default device
int default_device();                   // the device pg_segment_create pins on (0 unless pg_init chose another)
void use_device(int ordinal);           // makes `ordinal` current on the calling thread, initialising it on first use
int device_cus(int ordinal);            // its compute units (after use_device(ordinal))
double now_ms();                        // the host clock of host_ms_plan / host_ms_total
std::unique_ptr<Result> execute_query(Segment& seg, const pg_query& q, const CancelToken* cancel);         // pg_nullaware.cpp: query-level null handling above ...
// internal query flag (never set by callers: pg_query_exec masks it): the query is a part of a null-partitioned one — its filter is evaluated in
// three-valued logic even where the reference's FastFilteredCountOperator would not (a lone COUNT(*) over an index-only filter)
constexpr int32_t kQueryFlagNullPartition = 0x40000000;
std::unique_ptr<Result> execute_distinct(Segment& seg, const pg_query& q, const CancelToken* cancel);   // PG_QUERY_FLAG_DISTINCT (pg_exec.hip)
std::unique_ptr<Result> execute_selection(Segment& seg, const pg_query& q, const CancelToken* cancel);  // PG_QUERY_FLAG_SELECTION (pg_exec.hip)
// ---- side passes: aggregations answered by a pass of their own and joined to the ordinary plan by group key -------------------------------
// The frame they share (pg_exec_sidepass.hip; `who` names the path in messages — "PERCENTILE" / "expression" / "variance" / "covariance" / "fourth-moment" / "HISTOGRAM" / "FIRSTWITHTIME / LASTWITHTIME" —,
// `subject` is how a refusal names its aggregation: "PERCENTILE" / "an aggregation over an expression" / "a variance aggregation" /
// "FIRSTWITHTIME / LASTWITHTIME").
bool column_has_nulls(Segment& seg, const std::string& name);   // seg.mu held
Column* id_column(Segment& seg, Column& c, const char* what, const char* who);   // seg.mu held
std::vector<uint32_t> group_ids_of(const Result& r, int j, const Column& col, const Column& ids, int32_t n_rows, const char* who);
void wait_stream(hipStream_t stream, const CancelToken* cancel);   // polls the token while the stream drains (no spin limiter)
void side_query_check(const pg_query& q, const char* subject);     // the query's aggregation and group-by lists, before the path plans them
struct SideGroups {
  std::vector<Column*> group_cols, group_ids;   // the group-by columns and their fixed-bit ids
  std::vector<uint64_t> mult;                   // weight of the group column's digit (column 0 least significant)
  uint64_t G = 1;
  std::vector<std::shared_ptr<Column>> keep;    // the derived columns among group_cols (expression keys)
};
SideGroups side_groups(Segment& seg, const pg_query& q, const char* subject, const char* who, std::set<std::string>& read);   // seg.mu held; adds the columns' names to `read`
// the ordinary part's result, the filter's match words and the admitted groups' rows (rows[i]: the mixed-radix key of group i)
struct SidePass {
  std::unique_ptr<Result> res;
  std::unique_ptr<DocIdSet> ds;   // null: no filter and no upsert snapshot, every doc matches
  int64_t M = 0;                  // matching docs
  int32_t n_rows = 0;
  std::vector<uint32_t> rows;
  int64_t n_words = 0;            // ceil(total_docs / 64)
  hipStream_t stream = nullptr;
  int cus = 1;
};
SidePass side_pass_begin(Segment& seg, const pg_query& q, const SideBaseQuery& B, const SideGroups& G, const char* who, const CancelToken* cancel);
int64_t side_scan_fill(PgGroupScan& scan, const Segment& seg, const SidePass& S, const SideGroups& G);   // returns the group columns' bits per doc
// PG_QUERY_FLAG_PROFILE: a pass between two events of its own (without the flag there are none and stop_ms() is 0)
class ProfileTimer {
 public:
  explicit ProfileTimer(int32_t query_flags);
  ~ProfileTimer();
  ProfileTimer(const ProfileTimer&) = delete;
  ProfileTimer& operator=(const ProfileTimer&) = delete;
  void start(hipStream_t stream);
  float stop_ms();   // waits for the stream under the flag
 private:
  hipEvent_t ev_[2] = {nullptr, nullptr};
  hipStream_t stream_ = nullptr;
};
struct SidePassStats {
  const char* kernel;
  int64_t pass_bytes;     // the pass's algorithmic bytes
  int n_columns_read;     // distinct columns the query projects (ProjectOperator#getNumColumnsProjected)
  float pass_ms;
  double t0, t_plan;      // now_ms() at the start of the query and after its planning
};
// the ordinary part's columns and null vectors moved to their places in `out` (through B.base_index), `out` made the result's aggregations,
// every statistic of the query written, the schema filled
std::unique_ptr<Result> side_pass_finish(Segment& seg, const pg_query& q, const SideBaseQuery& B, SidePass& S, std::vector<AggResult>& out, const SidePassStats& P);
// ---- the slot-table paths (expressions, the variance family, COVAR_POP / COVAR_SAMP, SKEWNESS / KURTOSIS, HISTOGRAM, FIRSTWITHTIME / LASTWITHTIME): a table [G][slots] of 64-bit slots, filled over
// the match words by one of three tiers (side_tier, pg_side_query.h; the kernels' half is pg_side_scan.h) and gathered for the admitted rows
int side_pass_grid(int tier, int cus, int64_t n_words, int64_t lds_wgs_per_cu = 1);   // workgroups of a tier's pass: persistent ones in the LDS tier
int side_flat_grid(int cus, int64_t items);                                           // ... of a kernel with one thread per item (256 per workgroup)
int64_t value_src_bits(const Column& c);                                              // bits a kernel reads per doc of a value column
// S.rows uploaded, launch(rows on the device, out on the device) run, `got` copied back from `out`, the stream drained (also without rows)
void side_gather_rows(const SidePass& S, std::vector<int64_t>& got, const CancelToken* cancel, const std::function<void(const uint32_t*, int64_t*)>& launch);
// the algorithmic bytes of `passes` passes over `doc_bits` bits per doc and the match words, plus `extra`
int64_t side_pass_bytes(const Segment& seg, const SidePass& S, int passes, int64_t doc_bits, int64_t extra = 0);
// The admission of an aggregation's argument column (seg.mu held): found, single-value, numeric, without nulls under null handling and — with
// `layout_role` — readable by the kernels: fixed-bit dictIds with a dictionary on the device, or raw values.  `fn` names the function, `role` and
// `layout_role` the column ("column", "time column", "argument column") and `mv_note` ends the multi-value refusal, as the paths' messages differ.
Column* side_argument_column(Segment& seg, const char* name, const char* fn, const char* role, const char* layout_role, const char* mv_note, bool null_handling);
// ... of a column whose values are summed digit by digit (the variance family, covariance, SKEWNESS / KURTOSIS): an argument column the
// kernels read, without a NaN or an infinity — the sums have no digits for them
Column* side_value_column(Segment& seg, const char* name, const char* fn, bool null_handling);
// The columns an aggregation of ANOTHER path reads, added to `read` (a pass counts every column the query projects): a plain column name,
// the column arguments of a FIRSTWITHTIME / LASTWITHTIME / COVAR argument list, or the first argument of a HISTOGRAM's or a MODE's.  COUNT(*) and a malformed list add nothing — the list's
// own path refuses it.
void side_columns_read(const pg_agg_spec& s, std::set<std::string>& read);
const char* agg_function_text(int32_t fn);   // "VAR_POP", "FIRSTWITHTIME", ...: the functions the side paths name in messages
// The table of a slot-table path as its plan decides it (seg.mu held): the group-by columns (side_groups, which adds them to `read`; `read`
// then holds every column the query projects), the table's slots and where it lives (side_tier).  A table of more than `hbm_max_bytes`
// bytes is refused: "<noun>: .. groups x .. slots need a table of .. bytes, more than <knob> (..)".
struct SideTable {
  SideGroups groups;
  int32_t slots = 0;            // of one group's row
  uint64_t n_slots = 0;         // groups.G * slots
  int tier = TIER_REG;
  int n_columns_read = 0;       // distinct columns the query projects (ProjectOperator#getNumColumnsProjected)
};
SideTable side_table_plan(Segment& seg, const pg_query& q, const char* subject, const char* who, std::set<std::string>& read, int32_t slots, uint64_t lds_max_slots,
                          int bytes_per_slot, int64_t hbm_max_bytes, const char* noun, const char* knob);
// The pass of a path that keeps a table [G][slots] of int64 sums (expressions, the variance family, covariance, SKEWNESS / KURTOSIS, HISTOGRAM), from
// the query's first clock reading to its result.  A path's execute_* constructs one, plans, and then
//   begin       runs the ordinary part and the filter (side_pass_begin), allocates the table and fills the head of the kernel arguments;
//   accumulate  initialises the table, launches the path's kernels over the match words and gathers the admitted groups' rows, all between
//               a ProfileTimer's events, and checks the doc counts of a path with a count slot;
//   finish      joins the path's tuples to the ordinary part and writes the statistics (side_pass_finish).
class SumTablePass {
 public:
  SumTablePass(Segment& seg, const pg_query& q, const char* who, const CancelToken* cancel);   // the query's start: before the path plans
  // `A` zeroed; its scan, slots, n_groups, n_slots and table filled.  Returns the group columns' bits per doc; `T` outlives the pass.
  template <typename Args>
  int64_t begin(const SideTable& T, Args& A) {
    begin_table(T);
    memset(&A, 0, sizeof(A));
    A.slots = T.slots;
    A.n_groups = T.groups.G;
    A.n_slots = T.n_slots;
    A.table = table_.as<int64_t>();
    return side_scan_fill(A.scan, seg_, S_, T.groups);
  }
  // launch(tier, grid, stream): the accumulation kernel of the table's tier (not called when no doc matches); `lds_wgs_per_cu`: the LDS
  // tier's persistent workgroups per CU; `count_slot`: the slot of the group's doc count, -1 without one; init(grid, stream): sets the
  // table's initial values with one thread per slot — none: the table is zeroed by a memset.
  using Launch = std::function<void(int, int, hipStream_t)>;
  using Init = std::function<void(int, hipStream_t)>;
  void accumulate(const Launch& launch, int64_t lds_wgs_per_cu, int32_t count_slot, const Init& init = nullptr);
  int32_t n_rows() const { return S_.n_rows; }
  const int64_t* row(int32_t i) const { return &got_[(size_t)i * (size_t)T_->slots]; }   // the gathered row of admitted group i
  // `kernel`: the name the statistics report; `doc_bits`: the bits the pass read per doc; `merged`: the path's MERGED_* bit
  std::unique_ptr<Result> finish(std::vector<AggResult>& out, const char* kernel, int64_t doc_bits, uint32_t merged);
 private:
  void begin_table(const SideTable& T);
  Segment& seg_;
  const pg_query& q_;
  const char* who_;
  const CancelToken* cancel_;
  double t0_, t_plan_ = 0;
  const SideTable* T_ = nullptr;
  SideBaseQuery B_;
  SidePass S_;
  DeviceBuffer table_;
  std::vector<int64_t> got_;
  float pass_ms_ = 0;
};
// one tuple column for all the aggregations that share it (`aggs`: their indexes in `out`, at least one)
void side_share_result(std::vector<AggResult>& out, const std::vector<int>& aggs, AggResult&& r);
// ---- the side paths: one entry per family in kSidePaths (pg_exec_sidepass.hip), in nesting order — the only statement of that order.  A new
// family declares its three functions below and adds its entry; pg_query_supported (side_check) and pg_query_exec (execute_query) follow the table.
struct SidePath {
  bool (*is_side)(const pg_agg_spec&);            // is this aggregation answered by the path?
  void (*plan_check)(Segment&, const pg_query&);  // plans the path's aggregations and group-by columns and drops the plan: its refusals
  std::unique_ptr<Result> (*execute)(Segment&, const pg_query&, const CancelToken*);
  int32_t base_clears;                            // PG_QUERY_FLAG_* bits its ordinary part must not see
};
const SidePath* side_path_of(const pg_query& q);     // the outermost path with an aggregation in `q`; null: none, or a DISTINCT / selection query
void side_check(Segment& seg, const pg_query& q);    // every nested path's plan_check, then the checks and the cached plan of the innermost ordinary part
void side_base_query(const pg_query& q, SideBaseQuery& out);   // `q` without the aggregations of its outermost path (pg_side_query.h), failing through fail()
// exact PERCENTILE and MODE (pg_exec_percentile.hip): the ordinary part and one counting pass per distinct column; is_percentile_agg is the
// counting path's test, PERCENTILE or MODE
bool is_percentile_agg(const pg_agg_spec& s);
void percentile_plan_check(Segment& seg, const pg_query& q);
std::unique_ptr<Result> execute_percentile(Segment& seg, const pg_query& q, const CancelToken* cancel);
// ... its sort tier's runs (pg_kernels_percentile.hip): the matching docs' keys written compacted, sorted over their significant bits and
// run-length encoded on `stream`; returns after the stream drained (the number of runs is read back)
struct PctlSortRuns {
  DeviceBuffer keys, cum;       // [n_runs] distinct keys ascending, inclusive prefix sums of their counts
  DeviceBuffer counts;          // [n_runs] uint32
  int64_t n_runs = 0;
};
size_t pctl_sort_bytes(int64_t n_matches);   // bytes of the work area (keys in and out, runs, rocprim's temporaries)
void pctl_sort_build(const PgPctlArgs& A, int64_t n_matches, int key_bits, hipStream_t stream, PctlSortRuns& out);
// aggregations over an arithmetic expression (pg_exec_expr.hip): SUM / MIN / MAX / AVG / MINMAXRANGE whose pg_agg_spec.column is an expression
// text (pg_expr.h).  A bounds pass per (segment, expression), one accumulation pass for all expressions of the query.  Its plan_check answers
// the bounds from the segment's cache when it is filled, else the shape is let through.
bool is_expression_agg(const pg_agg_spec& s);
void expression_plan_check(Segment& seg, const pg_query& q);
std::unique_ptr<Result> execute_expression(Segment& seg, const pg_query& q, const CancelToken* cancel);
// VAR_POP / VAR_SAMP / STDDEV_POP / STDDEV_SAMP (pg_exec_var.hip): one accumulation pass of exact power sums (pg_moments.h) for all of them
bool is_variance_agg(const pg_agg_spec& s);
void variance_plan_check(Segment& seg, const pg_query& q);
std::unique_ptr<Result> execute_variance(Segment& seg, const pg_query& q, const CancelToken* cancel);
// FIRSTWITHTIME / LASTWITHTIME (pg_exec_withtime.hip): one arg-max pass (two in wide mode, pg_with_time.h) for all of them and a gather of the
// winners' values
bool is_with_time_agg(const pg_agg_spec& s);
void with_time_plan_check(Segment& seg, const pg_query& q);
std::unique_ptr<Result> execute_with_time(Segment& seg, const pg_query& q, const CancelToken* cancel);
// COVAR_POP / COVAR_SAMP (pg_exec_covar.hip): one fused accumulation pass of the exact sums of x, y and the rounded products (pg_covar.h)
// for all of them
bool is_covariance_agg(const pg_agg_spec& s);
void covariance_plan_check(Segment& seg, const pg_query& q);
std::unique_ptr<Result> execute_covariance(Segment& seg, const pg_query& q, const CancelToken* cancel);
// SKEWNESS / KURTOSIS (pg_exec_moment.hip): one accumulation pass of the exact power sums up to x^4 (pg_moment4.h) for all of them
bool is_moment_agg(const pg_agg_spec& s);
void moment_plan_check(Segment& seg, const pg_query& q);
std::unique_ptr<Result> execute_moment(Segment& seg, const pg_query& q, const CancelToken* cancel);
// HISTOGRAM (pg_exec_hist.hip): one counting pass of the bins (pg_histogram.h) for all of them
bool is_histogram_agg(const pg_agg_spec& s);
void histogram_plan_check(Segment& seg, const pg_query& q);
std::unique_ptr<Result> execute_histogram(Segment& seg, const pg_query& q, const CancelToken* cancel);
std::unique_ptr<Result> execute_query_plain(Segment& seg, const pg_query& q, const CancelToken* cancel);   // ... the executor proper (pg_exec.hip)
void fill_result_schema(Segment& seg, const pg_query& q, Result& r);
int64_t hll_cardinality(const uint8_t* regs, int log2m);   // HyperLogLog#cardinality of one register row (pg_exec.hip)
void result_merge(Result& dst, Result& src);
std::vector<uint8_t> result_data_table_v4(const Result& r);   // pg_datatable.cpp
void check_null_handling(Segment& seg, const pg_query& q);     // pg_nullaware.cpp: what PG_QUERY_FLAG_NULL_HANDLING leaves to the Java plan
// RCCL (pg_comm.cpp)
struct Comm;
void comm_unique_id(void* out128);
Comm* comm_init_rank(int device, int world, int rank, const void* id128);
void comm_init_all(int n, const int32_t* devices, Comm** out);
int comm_world(const Comm& c);
void comm_destroy(Comm* c);
void result_all_reduce(Result& r, Comm& c);
// shared by result_merge / result_all_reduce (pg_exec.hip): rebuild the host view of a result from its device table
void result_reassemble(Result& r);
int64_t table_signature(const DeviceTable& T);
void check_merge_bounds(uint64_t sum_max_abs, bool has_digit_sums, int64_t total_docs);
void device_table_tail_store(DeviceTable& T, hipStream_t stream);
void merge_sets_on_stream(uint32_t* dst, const uint32_t* gathered, int64_t n_words, int n_src, hipStream_t stream);
bool merge_rekey_by_value(DeviceTable& A, DeviceTable& B, hipStream_t stream);   // pg_comm.cpp: two tables of one device into the union of their group-by dictionaries
void remap_table_on_stream(const int64_t* src, int64_t* dst, int64_t G, int64_t G2, int n_ops, int n_cols, const int32_t* maps, const int64_t* geo,
                           const PgAccOp* ops, hipStream_t stream);
hipStream_t thread_stream(int device);
std::unique_ptr<DocIdSet> execute_filter(Segment& seg, const pg_filter_node* filter, int32_t flags = 0);   // flags: PG_QUERY_FLAG_NULL_HANDLING
std::shared_ptr<CompiledPlan> get_plan(Segment& seg, const pg_filter_node* filter, const pg_query* q, int32_t flags = 0);   // cached, under seg.mu
void docidset_copy_docids(DocIdSet& s, int32_t* out, int64_t cap);


// ---- measurement / test / tuning knobs ------------------------------------------------------------------------------------------------
// Every PG_* environment variable the library honours, read ONCE (at pg_init, or on first use) into this struct — round 4 had 44 getenv
// calls in the planner and the executor, several of them per plan or per query.  pg_options_reload() re-reads the environment: the A/B
// measurements (tools/) and the tests that compare two kernels inside one process call it after changing a variable; it must not run
// concurrently with queries.  Flags are "variable present"; integers keep `unset` (-1) when absent.
struct Knobs {
  // planner (pg_plan.cpp)
  bool no_oct = false, oct_no_affine = false, oct_byte_regs = false, oct_any_cardinality = false, no_oct_prune = false, oct_dword_regs = false;
  bool no_p2 = false, p2_no_fast_a = false, no_p2_oct = false, no_radix = false, no_radix_aux = false, no_part = false, no_radix_packed = false;
  bool no_pipe_general = false, no_pipe_wide = false, no_pipe_wide_double = false, mv_no_windows = false;
  int specd_wgs_per_cu = 1;   // PG_SPECD_WGS_PER_CU: workgroups of the pg_fast_dictrange_s family per CU (where their LDS fits)
  bool specw = false;   // PG_SPECW: the shared-stage frame (pg_fast_dictrange_w, pg_kernels_specw.hip) where it fits — a measurement variant, slower than pg_fast_dictrange_s
  bool p2_no_pack = false;   // PG_P2_NO_PACK: no shared COUNT + SUM atomic in the partition pipeline's aggregation pass
  bool no_mvg = false;   // PG_NO_MVG: GROUP BY one multi-value column through pg_mv_query_l (the interpreter's frame), not pg_mv_group_*
  bool specd_no_dma = false;   // PG_SPECD_NO_DMA: the register-staged kernels also where the LDS-DMA kernels (pg_fast_dictrange_s_*_dma) fit
  bool no_specd = false, specd_no_affine = false;   // PG_NO_SPECD: no pg_fast_dictrange_s family; PG_SPECD_NO_AFFINE: arithmetic dictionaries are gathered like any other
  int64_t oct_min_docs = -1;
  bool no_oct_count_kernel = false;                // PG_NO_OCT_COUNT_KERNEL: those plans run pg_oct_l (two load buffers) instead of pg_oct_c (four)
  bool no_oct_count = false;                       // PG_NO_OCT_COUNT: COUNT(*)-only group-bys stay on the quad-layout kernels
  int64_t oct_count_min_docs = (int64_t)1 << 22;   // PG_OCT_COUNT_MIN_DOCS
  int part_min = -1;
  // executor (pg_exec.hip)
  bool force_interpreter = false, no_scan_pipe = false, no_pipe = false, no_dense_fused = false, no_part_grid_clamp = false, no_spin_wait = false;
  bool trace_oct = false, no_tile_split = false, no_oct_exec = false, no_p2_simple = false, no_dense_count = false, no_direct_result = false, trace_host = false, no_limit_prefix = false, no_device_trim = false, no_fused_finish = false;
  bool no_narrow_image = false;   // PG_NO_NARROW_IMAGE: pg_fast_i32range_s / _st stream the raw columns also where a narrow image could be had
  bool wave_specialised = false, no_wave_specialised = false;   // PG_WAVE_SPECIALISED: pg_fast_i32range_s whatever the filter lets through; PG_NO_WAVE_SPECIALISED: never
  int wave_specialised_min_permille = 150;                     // PG_WAVE_SPECIALISED_MIN_PERMILLE: ... by default from this candidate rate on (profiles/r05_wave_specialised.txt)
  int max_inflight = 16;   // PG_MAX_INFLIGHT: queries between submission and result per device (<= 0: unbounded)
  int scan_wgs_per_cu = 1, pipe_wgs_per_cu = 1, wgs_per_cu = 1, p2_wgs_per_cu = 4, dense_count_wgs = 1, tile_split_max = -1, hash_first_buckets = -1;
  int64_t exact_stats_max_docs = (int64_t)1 << 22;
  int64_t exact_stats_device_max_docs = (int64_t)1 << 27;   // PG_EXACT_STATS_DEVICE_MAX_DOCS: ... and where the device counts it (pg_filter_stats_tiles.h: ~1 ms per 10^8 docs)
  bool filter_stats_host = false;   // PG_FILTER_STATS_HOST: the iterator automaton always walks on the host (pg_filter_stats.cpp), also for shapes the device counts
  int64_t select_sort_max_bytes = (int64_t)8 << 30;   // PG_SELECT_SORT_MAX_BYTES: work area of a selection's sort tier (larger ones are refused)
  // PERCENTILE (pg_exec_percentile.hip): counter tables of up to pctl_lds_max_keys 32-bit counters live in the workgroups' LDS (default and
  // ceiling PG_PCTL_LDS_KEYS = 32 768: 128 KiB, one persistent workgroup per CU), up to pctl_hbm_max_bytes in HBM (default 256 MiB: 2^26
  // counters); beyond that the sort tier runs.  Tests lower both to cross the boundaries on small segments.
  int64_t pctl_lds_max_keys = 32768;          // PG_PCTL_LDS_MAX_KEYS
  int64_t pctl_hbm_max_bytes = (int64_t)256 << 20;   // PG_PCTL_HBM_MAX_BYTES
  int64_t mode_split_ids = 1024;              // PG_MODE_SPLIT_IDS: fewest ids of a row worth a wavefront of their own in pg_mode_select (few wide rows are cut into such shares; flat from 64 to 4 096 in tools/prof_mode.py's sweep)
  int64_t pctl_sort_max_bytes = (int64_t)8 << 30;    // PG_PCTL_SORT_MAX_BYTES: work area of the sort tier (larger ones are refused by pg_query_exec, which alone knows the matches)
  // expressions inside aggregations (pg_exec_expr.hip): tables of up to expr_lds_max_slots 64-bit slots (groups x slots per group) live in the
  // workgroups' LDS (default and ceiling PG_EXPR_LDS_SLOTS = 16 384: 128 KiB), up to expr_hbm_max_bytes in HBM; beyond that the query is refused.
  int64_t expr_lds_max_slots = 16384;                // PG_EXPR_LDS_MAX_SLOTS
  int64_t expr_hbm_max_bytes = (int64_t)256 << 20;   // PG_EXPR_HBM_MAX_BYTES
  int64_t var_hbm_max_bytes = (int64_t)256 << 20;    // PG_VAR_HBM_MAX_BYTES: the slot table of the variance aggregations (pg_exec_var.hip) beyond its LDS tier; larger ones are refused
  int64_t moment_hbm_max_bytes = (int64_t)256 << 20; // PG_MOMENT_HBM_MAX_BYTES: the slot table of the SKEWNESS / KURTOSIS aggregations (pg_exec_moment.hip) beyond its LDS tier; larger ones are refused
  int64_t hist_hbm_max_bytes = (int64_t)256 << 20;   // PG_HIST_HBM_MAX_BYTES: the count table of the HISTOGRAM aggregations (pg_exec_hist.hip) beyond its LDS tier; larger ones are refused
  int64_t hist_combine_rounds = -1;                  // PG_HIST_COMBINE_ROUNDS: distinct bins per 64-doc word pg_hist_one combines inside the wavefront (unset: the constant of pg_device.h; a measurement, tools/prof_histogram.py)
  int64_t covar_hbm_max_bytes = (int64_t)256 << 20;  // PG_COVAR_HBM_MAX_BYTES: the slot table of the covariance aggregations (pg_exec_covar.hip) beyond its LDS tier; larger ones are refused
  int64_t wt_hbm_max_bytes = (int64_t)256 << 20;     // PG_WT_HBM_MAX_BYTES: the planes of FIRSTWITHTIME / LASTWITHTIME (pg_exec_withtime.hip) beyond their LDS tier; larger ones are refused
  int64_t limit_prefix_min_docs = (int64_t)1 << 20;   // PG_LIMIT_PREFIX_MIN_DOCS: smallest doc prefix of the numGroupsLimit admission pass (tests lower it)
  std::string oct_passes;      // PG_OCT_PASSES: cumulative fractions, e.g. "0.02,0.08,0.3,1"
  // pg_comm.cpp
  std::string rccl_library;    // PG_RCCL_LIBRARY: the collective library to bind instead of the system's RCCL
};
const Knobs& knobs();
void knobs_reload();
// The narrow image of `c` (see Column::img_dev), built on the first call; false: the column has none (then it never will).  Takes seg.mu.
bool narrow_image_eligible(const Column& c);
bool narrow_image(Segment& seg, Column& c);
inline int64_t narrow_image_tile_bytes(int bits) { return (int64_t)(PG_WAVE_DOCS / 8) * bits; }
}  // namespace pg
