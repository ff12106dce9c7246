// The frame of the side passes: aggregations answered by a pass of their own and joined to the ordinary plan by group key (exact PERCENTILE:
// and MODE: pg_exec_percentile.hip; aggregations over an expression: pg_exec_expr.hip; the variance family: pg_exec_var.hip; COVAR_POP / COVAR_SAMP: pg_exec_covar.hip; SKEWNESS / KURTOSIS: pg_exec_moment.hip; HISTOGRAM: pg_exec_hist.hip; FIRSTWITHTIME / LASTWITHTIME: pg_exec_withtime.hip).
// The paths are the entries of kSidePaths below, in nesting order; side_path_of, side_check and execute_query (pg_nullaware.cpp) follow that list.  A path plans its aggregations and its group-by
// columns (side_groups, side_argument_column; side_columns_read for what the other paths' aggregations read), splits the query
// (side_base_query), and then
//   1. side_pass_begin runs the ordinary part through execute_query — it decides the groups, the numGroupsLimit admission and the other
//      aggregations' results —, runs the filter again for its match words (the filter kernels and cached filter plan of the DISTINCT path; none
//      without a filter and without an upsert snapshot) and maps the admitted groups to rows of the path's table;
//   2. the path runs its own kernels over the match words (side_scan_fill: the head of their arguments) between a ProfileTimer's events;
//   3. side_pass_finish joins the columns and writes the statistics.
// The paths with a table [G][slots] of 64-bit slots share more: the end of their plans (side_table_plan: the groups, where the table lives
// — side_tier — and the refusal of a table over the path's knob), the pass's grid (side_pass_grid), the gather of the admitted rows
// (side_gather_rows) and the pass's bytes (side_pass_bytes, value_src_bits).
// The five of them whose slots are int64 sums (expressions, the variance family, covariance, SKEWNESS / KURTOSIS, HISTOGRAM) share the whole sequence:
// SumTablePass, at the end of this file, runs steps 1 to 3 with the table's allocation and initialisation, the launch, the gather through
// pg_expr_gather and the doc-count checks.  Such a path supplies its plan, its kernel arguments, a launch callable, the LDS tier's
// workgroups per CU, the kernel name to report, an initialiser where zero is not the identity, and the reading of the gathered rows into its
// tuples.  PERCENTILE (counting passes and a sort tier) and FIRSTWITHTIME / LASTWITHTIME (two planes, up to two ordered passes, a gather
// of its own) call the pieces directly.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <unordered_map>

#include "pg_internal.hpp"
#include "pg_expr.h"
#include "pg_histogram.h"

void pg_expr_launch_gather(const int64_t* table, const uint32_t* rows, int32_t n_rows, int32_t slots, uint64_t n_groups, int64_t* out, int grid, hipStream_t stream);

namespace pg {

bool column_has_nulls(Segment& seg, const std::string& name) {   // seg.mu held
  auto it = seg.null_vectors.find(name);
  return it != seg.null_vectors.end() && it->second && !it->second->posting_card.empty() && it->second->posting_card[0] > 0;
}

// the column of fixed-bit, value-ordered ids behind `c`: its own dictIds, or its virtual dictionary's (seg.mu held)
Column* id_column(Segment& seg, Column& c, const char* what, const char* who) {
  Column* id = &c;
  if (!c.has_dictionary) {
    if (c.col_kind != PG_COL_RAW32 && c.col_kind != PG_COL_RAW64 && c.col_kind != PG_COL_VAR_BYTES)
      fail(PG_ERR_UNSUPPORTED, "%s: %s column %s (layout %d)", who, what, c.name.c_str(), c.col_kind);
    ensure_virtual_dictionary(seg, c);
    id = c.vdict.get();
  }
  if (id->cardinality < 1 || id->bits < 1 || id->bits > 31)
    fail(PG_ERR_UNSUPPORTED, "%s: %s column %s has %d values in %d bits", who, what, c.name.c_str(), id->cardinality, id->bits);
  return id;
}

void wait_stream(hipStream_t stream, const CancelToken* cancel) {
  if (cancel) {
    for (;;) {
      const hipError_t e = hipStreamQuery(stream);
      if (e == hipSuccess) return;
      if (e != hipErrorNotReady) PG_HIP(e);
      if (cancel->requested.load(std::memory_order_acquire)) {
        (void)hipStreamSynchronize(stream);   // let what was launched finish
        fail(PG_ERR_CANCELLED, "query cancelled (EarlyTerminationException)");
      }
    }
  }
  PG_HIP(hipStreamSynchronize(stream));
}

// the id of every admitted group's key in group-by column j of a side pass
std::vector<uint32_t> group_ids_of(const Result& r, int j, const Column& col, const Column& ids, int32_t n_rows, const char* who) {
  std::vector<uint32_t> out((size_t)n_rows);
  const int32_t kt = r.group_key_type.empty() ? PG_GROUP_KEY_DICT_IDS : r.group_key_type[(size_t)j];
  if (kt == PG_GROUP_KEY_DICT_IDS) {
    if (!col.has_dictionary) fail(PG_ERR_INTERNAL, "%s: dictIds for the raw group-by column %s", who, col.name.c_str());
    for (int32_t i = 0; i < n_rows; i++) out[(size_t)i] = (uint32_t)r.group_dict_ids[(size_t)j][(size_t)i];
    return out;
  }
  if (col.has_dictionary) fail(PG_ERR_INTERNAL, "%s: values for the dictionary group-by column %s", who, col.name.c_str());
  const size_t card = (size_t)ids.cardinality;
  if (kt == PG_GROUP_KEY_BYTES_VALUES) {
    std::unordered_map<std::string, uint32_t> by_value;
    for (size_t v = 0; v < card; v++)
      by_value.emplace(std::string(reinterpret_cast<const char*>(ids.vdict_bytes.data()) + ids.vdict_bytes_off[v], (size_t)(ids.vdict_bytes_off[v + 1] - ids.vdict_bytes_off[v])), (uint32_t)v);
    const auto& off = r.group_bytes_off[(size_t)j];
    for (int32_t i = 0; i < n_rows; i++) {
      auto it = by_value.find(std::string(reinterpret_cast<const char*>(r.group_bytes[(size_t)j].data()) + off[(size_t)i], (size_t)(off[(size_t)i + 1] - off[(size_t)i])));
      if (it == by_value.end()) fail(PG_ERR_INTERNAL, "%s: a group key of %s is not in its virtual dictionary", who, col.name.c_str());
      out[(size_t)i] = it->second;
    }
    return out;
  }
  std::unordered_map<int64_t, uint32_t> by_value;   // LONG values, or the IEEE bits of DOUBLE values: what the ordinary part hands back
  by_value.reserve(card * 2);
  for (size_t v = 0; v < card; v++) by_value.emplace(vdict_value_of_key(ids.vdict_keys[v], ids.vdict_kind, nullptr), (uint32_t)v);
  for (int32_t i = 0; i < n_rows; i++) {
    auto it = by_value.find(r.group_values[(size_t)j][(size_t)i]);
    if (it == by_value.end()) fail(PG_ERR_INTERNAL, "%s: a group key of %s is not in its virtual dictionary", who, col.name.c_str());
    out[(size_t)i] = it->second;
  }
  return out;
}

void side_query_check(const pg_query& q, const char* subject) {
  if (q.n_aggregations <= 0 || !q.aggregations) fail(PG_ERR_INVALID_ARGUMENT, "query has no aggregation");
  if (q.n_group_by < 0 || (q.n_group_by > 0 && !q.group_by_columns)) fail(PG_ERR_INVALID_ARGUMENT, "group_by_columns is null");
  if (q.n_group_by > PG_MAX_GROUP_COLS) fail(PG_ERR_UNSUPPORTED, "%s with more than %d group-by columns", subject, PG_MAX_GROUP_COLS);
}

SideGroups side_groups(Segment& seg, const pg_query& q, const char* subject, const char* who, std::set<std::string>& read) {
  const bool null_handling = (q.flags & PG_QUERY_FLAG_NULL_HANDLING) != 0;
  SideGroups S;
  for (int j = 0; j < q.n_group_by; j++) {
    const char* name = q.group_by_columns[j];
    std::shared_ptr<Column> derived;
    Column* c = group_key_column(seg, name, &derived);   // an expression key: its derived DOUBLE column, grouped through its virtual dictionary
    if (!c) fail(PG_ERR_NOT_FOUND, "column not found: %s", name ? name : "(null)");
    if (derived) S.keep.push_back(derived);
    if (c->is_mv || c->raw_mv) fail(PG_ERR_UNSUPPORTED, "%s next to the multi-value group-by column %s", subject, c->name.c_str());
    if (null_handling && column_has_nulls(seg, c->name)) fail(PG_ERR_UNSUPPORTED, "enableNullHandling: %s grouped by %s, which holds nulls", subject, c->name.c_str());
    for (Column* r : key_columns_read(c)) read.insert(r->name);   // (an expression key counts its operands)
    Column* id = id_column(seg, *c, "group-by", who);
    S.group_cols.push_back(c);
    S.group_ids.push_back(id);
    S.mult.push_back(S.G);
    S.G *= (uint64_t)id->cardinality;
    if (S.G > ((uint64_t)1 << 32)) fail(PG_ERR_UNSUPPORTED, "%s: group key space over 2^32 (the product of the group-by columns' cardinalities)", subject);
  }
  return S;
}

// ---- the side paths in nesting order: the outermost first.  A query that carries several kinds is answered by the first one here; its ordinary
// part comes back through execute_query and meets the next.
// the ordinary part may hold a PERCENTILE, which reads PG_QUERY_FLAG_FINAL_PERCENTILE; it does not keep its table (the result is not merged in the library)
constexpr int32_t kSideBaseClears = PG_QUERY_FLAG_KEEP_DEVICE_TABLE;
// the counting path's ordinary part holds neither a PERCENTILE nor a MODE: it neither keeps its table (the result is not merged in the library) nor reads the final-form flags
constexpr int32_t kPercentileBaseClears = PG_QUERY_FLAG_FINAL_PERCENTILE | PG_QUERY_FLAG_FINAL_MODE | PG_QUERY_FLAG_KEEP_DEVICE_TABLE;
const SidePath kSidePaths[] = {
    // aggregations over expressions: before the PERCENTILE, so that the expression pass is the outer one of a query that carries both — its
    // statistics count the operand columns, and its ordinary part (PERCENTILEs included) comes back through execute_query
    {is_expression_agg, expression_plan_check, execute_expression, kSideBaseClears},
    // inside the expression pass, outside the variance's and the PERCENTILE's: its statistics count its two argument columns
    {is_with_time_agg, with_time_plan_check, execute_with_time, kSideBaseClears},
    // inside the FIRSTWITHTIME / LASTWITHTIME pass (which counts its argument columns, side_columns_read), outside the variance's
    {is_covariance_agg, covariance_plan_check, execute_covariance, kSideBaseClears},
    // inside the covariance pass, outside the variance's: SKEWNESS / KURTOSIS next to VAR_POP and PERCENTILE leave those to the passes below
    {is_moment_agg, moment_plan_check, execute_moment, kSideBaseClears},
    // inside the SKEWNESS / KURTOSIS pass, outside the variance's: its ordinary part (COUNT(*) when nothing else remains) names the groups
    {is_histogram_agg, histogram_plan_check, execute_histogram, kSideBaseClears},
    // inside the expression pass, outside the PERCENTILE's: its ordinary part comes back through execute_query
    {is_variance_agg, variance_plan_check, execute_variance, kSideBaseClears},
    // the counting path, PERCENTILE or MODE (is_percentile_agg), innermost: its ordinary part comes back through execute_query; nulls in its
    // columns are refused (percentile_plan_check).  MODE has no entry of its own: its intermediate is the table the PERCENTILE's counting
    // pass builds, so MODE(x) next to PERCENTILE(x, p) shares one pass, and next to a HISTOGRAM, a variance or an expression it nests as a PERCENTILE does
    {is_percentile_agg, percentile_plan_check, execute_percentile, kPercentileBaseClears},
};

const SidePath* side_path_of(const pg_query& q) {
  if (q.flags & (PG_QUERY_FLAG_DISTINCT | PG_QUERY_FLAG_SELECTION)) return nullptr;
  if (!q.aggregations) return nullptr;
  for (const SidePath& path : kSidePaths)
    for (int a = 0; a < q.n_aggregations; a++) if (path.is_side(q.aggregations[a])) return &path;
  return nullptr;
}

void side_base_query(const pg_query& q, SideBaseQuery& out) {
  const SidePath* path = side_path_of(q);
  if (!path) fail(PG_ERR_INTERNAL, "a side pass over a query without a side aggregation");
  std::string error;
  const int32_t st = side_base_query(q, path->is_side, path->base_clears, out, error);
  if (st != PG_OK) fail(st, "%s", error.c_str());
}

void side_check(Segment& seg, const pg_query& q) {
  const SidePath* path = side_path_of(q);
  if (!path) {   // the ordinary part: what its plan refuses; compiled and cached for the execution that follows
    check_null_handling(seg, q);
    (void)get_plan(seg, q.filter, &q);
    return;
  }
  path->plan_check(seg, q);
  SideBaseQuery B;   // ... and what the ordinary part refuses
  side_base_query(q, B);
  side_check(seg, B.q);
}

// ---- what the slot-table paths share ---------------------------------------------------------------------------------------------------------
int side_flat_grid(int cus, int64_t items) { return (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)cus * 8, (items + 255) / 256)); }

int side_pass_grid(int tier, int cus, int64_t n_words, int64_t lds_wgs_per_cu) {
  const int64_t words_per_wg = tier == TIER_LDS ? 32 : 16;
  return (int)std::max<int64_t>(1, std::min<int64_t>(tier == TIER_LDS ? cus * lds_wgs_per_cu : (int64_t)cus * 8, (n_words + words_per_wg - 1) / words_per_wg));
}

int64_t value_src_bits(const Column& c) { return c.col_kind == PG_COL_FIXED_BIT ? c.bits : (c.col_kind == PG_COL_RAW32 ? 32 : 64); }

void side_gather_rows(const SidePass& S, std::vector<int64_t>& got, const CancelToken* cancel, const std::function<void(const uint32_t*, int64_t*)>& launch) {
  if (S.n_rows > 0) {
    DeviceBuffer d_rows((size_t)S.n_rows * 4), d_out(got.size() * 8);
    PG_HIP(hipMemcpyAsync(d_rows.ptr, S.rows.data(), (size_t)S.n_rows * 4, hipMemcpyHostToDevice, S.stream));
    launch(d_rows.as<uint32_t>(), d_out.as<int64_t>());
    PG_HIP(hipGetLastError());
    PG_HIP(hipMemcpyAsync(got.data(), d_out.ptr, got.size() * 8, hipMemcpyDeviceToHost, S.stream));
    wait_stream(S.stream, cancel);   // d_rows and d_out go out of scope
  } else {
    wait_stream(S.stream, cancel);
  }
}

int64_t side_pass_bytes(const Segment& seg, const SidePass& S, int passes, int64_t doc_bits, int64_t extra) {
  return passes * (((int64_t)seg.total_docs * doc_bits + 7) / 8 + (S.ds ? S.n_words * 8 : 0)) + extra;
}

Column* side_argument_column(Segment& seg, const char* name, const char* fn, const char* role, const char* layout_role, const char* mv_note, bool null_handling) {
  Column* c = seg.find(name);
  if (!c) fail(PG_ERR_NOT_FOUND, "column not found: %s", name);
  if (c->is_mv || c->raw_mv) fail(PG_ERR_UNSUPPORTED, "%s over the multi-value %s %s%s", fn, role, c->name.c_str(), mv_note);
  if (c->data_type > PG_TYPE_DOUBLE) fail(PG_ERR_UNSUPPORTED, "%s over the %s %s %s", fn, c->data_type == PG_TYPE_STRING ? "STRING" : "BYTES", role, c->name.c_str());
  if (null_handling && column_has_nulls(seg, c->name)) fail(PG_ERR_UNSUPPORTED, "enableNullHandling: %s over %s, which holds nulls", fn, c->name.c_str());
  if (!layout_role) return c;
  const bool dict_ok = c->has_dictionary && c->col_kind == PG_COL_FIXED_BIT && c->bits >= 1 && c->bits <= 31 && c->cardinality >= 1 && c->dict_dev.ptr;
  const bool raw_ok = !c->has_dictionary && (c->col_kind == PG_COL_RAW32 || c->col_kind == PG_COL_RAW64);
  if (!dict_ok && !raw_ok) fail(PG_ERR_UNSUPPORTED, "%s: %s %s (layout %d, %d bits)", fn, layout_role, c->name.c_str(), c->col_kind, c->bits);
  return c;
}

Column* side_value_column(Segment& seg, const char* name, const char* fn, bool null_handling) {
  Column* c = side_argument_column(seg, name, fn, "column", "argument column", "", null_handling);
  // the registration pass (pg_segment.cpp) knows every FLOAT / DOUBLE column's non-finite values
  if ((c->val_type == PG_V_F32 || c->val_type == PG_V_F64) && c->has_nonfinite)
    fail(PG_ERR_UNSUPPORTED, "%s over %s, which holds a NaN or an infinity: the Java plan answers such a query", fn, c->name.c_str());
  return c;
}

void side_columns_read(const pg_agg_spec& s, std::set<std::string>& read) {
  if (!s.column) return;
  if (is_histogram_agg(s)) {   // x, then the bins
    HistSpec spec;
    std::string error;
    if (hist_parse_arguments(s.column, spec, error) == PG_OK && !expr_is_expression(spec.column.c_str())) read.insert(spec.column);
    return;
  }
  if (s.function == PG_AGG_MODE) {   // x, then the reducer
    ModeSpec spec;
    std::string error;
    if (mode_parse_arguments(s.column, spec, error) == PG_OK && !expr_is_expression(spec.column.c_str()) && spec.column != "*") read.insert(spec.column);
    return;
  }
  const bool with_time = is_with_time_agg(s);
  if (!with_time && !is_covariance_agg(s)) {
    if (strcmp(s.column, "*") != 0) read.insert(s.column);
    return;
  }
  std::vector<ExprArgument> args;   // x, t, 'TYPE' or x, y: the first two are columns
  std::string error;
  if (expr_split_arguments(s.column, args, error) != PG_OK || args.size() != (with_time ? 3u : 2u)) return;
  for (int k = 0; k < 2; k++) if (!args[(size_t)k].quoted) read.insert(args[(size_t)k].text);
}

SideTable side_table_plan(Segment& seg, const pg_query& q, const char* subject, const char* who, std::set<std::string>& read, int32_t slots, uint64_t lds_max_slots,
                          int bytes_per_slot, int64_t hbm_max_bytes, const char* noun, const char* knob) {
  SideTable T;
  T.groups = side_groups(seg, q, subject, who, read);
  T.n_columns_read = (int)read.size();
  T.slots = slots;
  T.n_slots = T.groups.G * (uint64_t)slots;   // G <= 2^32 and a path's row has fewer than 2^7 slots
  const uint64_t bytes = T.n_slots * (uint64_t)bytes_per_slot;
  T.tier = side_tier(q.n_group_by, T.n_slots, lds_max_slots, bytes, hbm_max_bytes);
  if (T.tier == TIER_REFUSED)
    fail(PG_ERR_UNSUPPORTED, "%s: %llu groups x %d slots need a table of %llu bytes, more than %s (%lld)", noun, (unsigned long long)T.groups.G, slots,
         (unsigned long long)bytes, knob, (long long)hbm_max_bytes);
  return T;
}

const char* agg_function_text(int32_t fn) {
  switch (fn) {
    case PG_AGG_COUNT: return "COUNT";
    case PG_AGG_DISTINCTCOUNT: return "DISTINCTCOUNT";
    case PG_AGG_DISTINCTCOUNTHLL: return "DISTINCTCOUNTHLL";
    case PG_AGG_PERCENTILE: return "PERCENTILE";
    case PG_AGG_COUNTMV: return "COUNTMV";
    case PG_AGG_SUMMV: return "SUMMV";
    case PG_AGG_MINMV: return "MINMV";
    case PG_AGG_MAXMV: return "MAXMV";
    case PG_AGG_AVGMV: return "AVGMV";
    case PG_AGG_MINMAXRANGEMV: return "MINMAXRANGEMV";
    case PG_AGG_DISTINCTCOUNTMV: return "DISTINCTCOUNTMV";
    case PG_AGG_DISTINCTCOUNTHLLMV: return "DISTINCTCOUNTHLLMV";
    case PG_AGG_VARPOP: return "VAR_POP";
    case PG_AGG_VARSAMP: return "VAR_SAMP";
    case PG_AGG_STDDEVPOP: return "STDDEV_POP";
    case PG_AGG_STDDEVSAMP: return "STDDEV_SAMP";
    case PG_AGG_COVARPOP: return "COVAR_POP";
    case PG_AGG_COVARSAMP: return "COVAR_SAMP";
    case PG_AGG_SKEWNESS: return "SKEWNESS";
    case PG_AGG_KURTOSIS: return "KURTOSIS";
    case PG_AGG_HISTOGRAM: return "HISTOGRAM";
    case PG_AGG_MODE: return "MODE";
    case PG_AGG_FIRSTWITHTIME: return "FIRSTWITHTIME";
    case PG_AGG_LASTWITHTIME: return "LASTWITHTIME";
    default: return "this aggregation function";
  }
}

SidePass side_pass_begin(Segment& seg, const pg_query& q, const SideBaseQuery& B, const SideGroups& G, const char* who, const CancelToken* cancel) {
  SidePass S;
  S.res = execute_query(seg, B.q, cancel);
  use_device(seg.device);
  S.stream = thread_stream(seg.device);
  S.cus = device_cus(seg.device);
  S.n_rows = q.n_group_by > 0 ? S.res->num_groups : 1;
  S.n_words = ((int64_t)seg.total_docs + 63) / 64;
  // ---- the filter's match words (none without a filter and without an upsert snapshot) ---------------------------------------------------
  bool snapshot = false;
  {
    std::lock_guard<std::mutex> lock(seg.mu);
    snapshot = seg.queryable_doc_ids != nullptr;
  }
  S.M = seg.total_docs;
  if (q.filter || snapshot) {
    S.ds = execute_filter(seg, q.filter, q.flags & PG_QUERY_FLAG_NULL_HANDLING);
    S.M = S.ds->cardinality;
  }
  if (cancel && cancel->requested.load(std::memory_order_acquire)) fail(PG_ERR_CANCELLED, "query cancelled (EarlyTerminationException)");
  // ---- the admitted groups' keys -------------------------------------------------------------------------------------------------------------
  S.rows.assign((size_t)S.n_rows, 0);
  for (int j = 0; j < q.n_group_by; j++) {
    const std::vector<uint32_t> ids = group_ids_of(*S.res, j, *G.group_cols[(size_t)j], *G.group_ids[(size_t)j], S.n_rows, who);
    for (int32_t i = 0; i < S.n_rows; i++) {
      if (ids[(size_t)i] >= (uint32_t)G.group_ids[(size_t)j]->cardinality) fail(PG_ERR_INTERNAL, "%s: group key id %u of %s out of range", who, ids[(size_t)i], G.group_cols[(size_t)j]->name.c_str());
      S.rows[(size_t)i] += (uint32_t)(ids[(size_t)i] * G.mult[(size_t)j]);
    }
  }
  return S;
}

int64_t side_scan_fill(PgGroupScan& scan, const Segment& seg, const SidePass& S, const SideGroups& G) {
  scan.match = S.ds ? S.ds->words.as<uint64_t>() : nullptr;
  scan.n_words = S.n_words;
  scan.n_docs = seg.total_docs;
  scan.n_gcols = (int32_t)G.group_ids.size();
  int64_t bits = 0;
  for (size_t j = 0; j < G.group_ids.size(); j++) {
    scan.gcols[j].data = G.group_ids[j]->fwd_dev.as<uint8_t>();
    scan.gcols[j].bits = G.group_ids[j]->bits;
    scan.gcols[j].card = G.group_ids[j]->cardinality;
    scan.gcols[j].mult = G.mult[j];
    bits += G.group_ids[j]->bits;
  }
  return bits;
}

ProfileTimer::ProfileTimer(int32_t query_flags) {
  if (query_flags & PG_QUERY_FLAG_PROFILE) {
    PG_HIP(hipEventCreate(&ev_[0]));
    PG_HIP(hipEventCreate(&ev_[1]));
  }
}
ProfileTimer::~ProfileTimer() {
  for (hipEvent_t e : ev_) if (e) (void)hipEventDestroy(e);
}
void ProfileTimer::start(hipStream_t stream) {
  stream_ = stream;
  if (ev_[0]) PG_HIP(hipEventRecord(ev_[0], stream));
}
float ProfileTimer::stop_ms() {
  float ms = 0;
  if (ev_[0]) {
    PG_HIP(hipEventRecord(ev_[1], stream_));
    PG_HIP(hipEventSynchronize(ev_[1]));
    PG_HIP(hipEventElapsedTime(&ms, ev_[0], ev_[1]));
  }
  return ms;
}

std::unique_ptr<Result> side_pass_finish(Segment& seg, const pg_query& q, const SideBaseQuery& B, SidePass& S, std::vector<AggResult>& out, const SidePassStats& P) {
  std::unique_ptr<Result> res = std::move(S.res);
  std::vector<std::vector<uint8_t>> nulls;
  if (!res->agg_nulls.empty()) nulls.assign((size_t)q.n_aggregations, {});
  for (int a = 0; a < q.n_aggregations; a++) {
    const int bi = B.base_index[(size_t)a];
    if (bi < 0) continue;
    out[(size_t)a] = std::move(res->aggs[(size_t)bi]);
    if (!nulls.empty() && (size_t)bi < res->agg_nulls.size()) nulls[(size_t)a] = std::move(res->agg_nulls[(size_t)bi]);
  }
  res->aggs = std::move(out);
  res->agg_nulls = std::move(nulls);
  res->dev.reset();
  // the ordinary part's statistics become the query's: its device times and bytes are added to (a PERCENTILE inside an expression query has
  // added its own already), the counters the Java side reports are the whole query's
  pg_exec_stats& st = res->stats;
  st.num_docs_scanned = S.M;
  st.num_entries_scanned_post_filter = S.M * P.n_columns_read;
  if (S.ds) {
    st.num_entries_scanned_in_filter = S.ds->stats.num_entries_scanned_in_filter;
    st.stats_exact = S.ds->stats.stats_exact;
    st.filter_stats_path = S.ds->stats.filter_stats_path;
    st.device_ms_filter += S.ds->stats.device_ms_filter;
  } else {
    st.num_entries_scanned_in_filter = 0;
    st.stats_exact = 1;
  }
  st.device_ms_aggregate += P.pass_ms;
  st.device_ms_total += P.pass_ms + (S.ds ? S.ds->stats.device_ms_filter : 0.0f);
  st.num_total_docs = seg.total_docs;
  st.star_tree_index = -1;
  st.algorithmic_bytes += P.pass_bytes;
  snprintf(st.kernel, sizeof(st.kernel), "%s", P.kernel);
  fill_result_schema(seg, q, *res);
  res->null_handling = (q.flags & PG_QUERY_FLAG_NULL_HANDLING) != 0;
  st.host_ms_plan += (float)(P.t_plan - P.t0);
  st.host_ms_total = (float)(now_ms() - P.t0);
  return res;
}

// ---- the pass of the sum-table paths ---------------------------------------------------------------------------------------------------------
SumTablePass::SumTablePass(Segment& seg, const pg_query& q, const char* who, const CancelToken* cancel) : seg_(seg), q_(q), who_(who), cancel_(cancel), t0_(now_ms()) {
  use_device(seg.device);
}

void SumTablePass::begin_table(const SideTable& T) {
  t_plan_ = now_ms();
  T_ = &T;
  side_base_query(q_, B_);
  S_ = side_pass_begin(seg_, q_, B_, T.groups, who_, cancel_);
  table_.alloc((size_t)T.n_slots * 8);
}

void SumTablePass::accumulate(const Launch& launch, int64_t lds_wgs_per_cu, int32_t count_slot, const Init& init) {
  const SideTable& T = *T_;
  hipStream_t stream = S_.stream;
  // PG_QUERY_FLAG_PROFILE: the pass (initialisation, accumulation, gather and its copy) between two events of its own
  ProfileTimer timer(q_.flags);
  timer.start(stream);
  if (init) {
    init(side_flat_grid(S_.cus, (int64_t)T.n_slots), stream);
    PG_HIP(hipGetLastError());
  } else {
    PG_HIP(hipMemsetAsync(table_.ptr, 0, (size_t)T.n_slots * 8, stream));
  }
  if (S_.M > 0 && S_.n_words > 0) {
    launch(T.tier, side_pass_grid(T.tier, S_.cus, S_.n_words, lds_wgs_per_cu), stream);
    PG_HIP(hipGetLastError());
  }
  got_.assign((size_t)S_.n_rows * (size_t)T.slots, 0);
  side_gather_rows(S_, got_, cancel_, [&](const uint32_t* rows, int64_t* out) {
    pg_expr_launch_gather(table_.as<int64_t>(), rows, S_.n_rows, T.slots, T.groups.G, out, side_flat_grid(S_.cus, (int64_t)got_.size()), stream);
  });
  pass_ms_ = timer.stop_ms();
  if (count_slot < 0) return;
  if (q_.n_group_by == 0 && row(0)[count_slot] != S_.M)
    fail(PG_ERR_INTERNAL, "%s: %lld docs counted for %lld matching docs", who_, (long long)row(0)[count_slot], (long long)S_.M);
  for (int32_t i = 0; i < S_.n_rows; i++) {
    const int64_t n = row(i)[count_slot];
    if (n < 0 || n > S_.M) fail(PG_ERR_INTERNAL, "%s: %lld docs counted in a group of %lld matching docs", who_, (long long)n, (long long)S_.M);
  }
}

std::unique_ptr<Result> SumTablePass::finish(std::vector<AggResult>& out, const char* kernel, int64_t doc_bits, uint32_t merged) {
  std::unique_ptr<Result> res = side_pass_finish(seg_, q_, B_, S_, out, {kernel, side_pass_bytes(seg_, S_, 1, doc_bits), T_->n_columns_read, pass_ms_, t0_, t_plan_});
  res->merged_elsewhere |= merged;
  return res;
}

void side_share_result(std::vector<AggResult>& out, const std::vector<int>& aggs, AggResult&& r) {
  for (size_t k = 0; k + 1 < aggs.size(); k++) out[(size_t)aggs[k]] = r;
  out[(size_t)aggs.back()] = std::move(r);
}

}  // namespace pg
