// The frame of the side passes: aggregations answered by a pass of their own and joined to the ordinary plan by group key (exact PERCENTILE:
// pg_exec_percentile.hip; aggregations over an expression: pg_exec_expr.hip; the variance family: pg_exec_var.hip; FIRSTWITHTIME / LASTWITHTIME: pg_exec_withtime.hip).  A path plans its aggregations and its group-by
// columns (side_groups), splits the query (side_base_query), and then
//   1. side_pass_begin runs the ordinary part through execute_query — it decides the groups, the numGroupsLimit admission and the other
//      aggregations' results —, runs the filter again for its match words (the filter kernels and cached filter plan of the DISTINCT path; none
//      without a filter and without an upsert snapshot) and maps the admitted groups to rows of the path's table;
//   2. the path runs its own kernels over the match words (side_scan_fill: the head of their arguments) between a ProfileTimer's events;
//   3. side_pass_finish joins the columns and writes the statistics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <unordered_map>

#include "pg_internal.hpp"

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

void side_base_query(const pg_query& q, bool (*is_side)(const pg_agg_spec&), int32_t clear_flags, SideBaseQuery& out) {
  std::string error;
  const int32_t st = side_base_query(q, is_side, clear_flags, out, error);
  if (st != PG_OK) fail(st, "%s", error.c_str());
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

}  // namespace pg
