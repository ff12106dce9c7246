// Queries with an exact PERCENTILE aggregation (PG_AGG_PERCENTILE): a side pass joined to the ordinary plan by group key, in the frame of
// pg_exec_sidepass.hip (which runs step 1 and the filter, maps the admitted groups to rows and joins the result).
//   1. The ordinary part — the query without its PERCENTILEs (COUNT(*) if nothing else remains) — runs through execute_query unchanged: it
//      decides the groups, the numGroupsLimit admission and the other aggregations' results.
//   2. One counting pass per distinct percentile COLUMN (p50 / p95 / p99 of one column share it) over the filter's match words into a dense
//      table of 32-bit counters [G][C]: pg_pctl_lds up to Knobs::pctl_lds_max_keys counters, pg_pctl_hbm up to Knobs::pctl_hbm_max_bytes;
//      beyond that the sort tier (pg_pctl_sort: the matching docs' 64-bit keys written compacted, a radix sort over their significant bits, a
//      run-length encode), refused when its work area would exceed Knobs::pctl_sort_max_bytes.
//   3. Rank selection on the device over the rows of the admitted groups (pg_pctl_select; pg_pctl_sort_select over the sort tier's runs); the
//      intermediate form is the rows' non-zero (value, count) runs (pg_pctl_runs / pg_pctl_sort_runs), the final form
//      (PG_QUERY_FLAG_FINAL_PERCENTILE) one double per group and aggregation.
// MODE (PG_AGG_MODE) joins this path: its intermediate, a map value -> count per group, is what the counting pass builds.  MODE(x) next to
// PERCENTILE(x, p) shares the column's pass; after it the rank selection runs only for a column with PERCENTILEs and the mode selection
// (pg_mode_select / pg_mode_finish, pg_mode_sort_select: the partial of pg_mode.h per row) for one with MODEs; either delivers the rows' n and
// non-zero counters.  The intermediate form (PG_RESULT_VALUE_COUNT_MAP) is the same runs with their keys decoded to exact longs or doubles;
// the final form (PG_QUERY_FLAG_FINAL_MODE) is computed on the host from the partial — the lowest / highest tied id, or for AVG the exact sum
// of the tied values, whose ids a threshold launch of pg_pctl_runs / pg_pctl_sort_runs compacts when more than two tie.
// The kernels are those of pg_kernels_percentile.hip and pg_kernels_mode.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <set>
#include <string>

#include "pg_internal.hpp"
#include "pg_expr.h"

void pg_pctl_launch_count(const PgPctlArgs* args, int lds, int grid, hipStream_t stream);
void pg_pctl_launch_select(const PgPctlSelectArgs* args, int grid, hipStream_t stream);
void pg_pctl_launch_runs(const uint32_t* table, const uint32_t* rows, int32_t n_rows, uint32_t card, const int64_t* offsets, const uint32_t* min_counts,
                         uint32_t* out_ids, uint32_t* out_counts, int grid, hipStream_t stream);
void pg_mode_launch_select(const PgModeSelectArgs* args, int grid, hipStream_t stream);
void pg_mode_launch_finish(const PgModeRow* parts, int32_t n_rows, uint32_t shares, PgModeRow* out, int grid, hipStream_t stream);
void pg_mode_launch_sort_select(const PgModeSortSelectArgs* args, int grid, hipStream_t stream);

void pg_pctl_launch_sort_select(const PgPctlSortSelectArgs* args, hipStream_t stream);
void pg_pctl_launch_sort_runs(const uint64_t* run_keys, const uint32_t* run_counts, const uint32_t* rows, const int64_t* first_run, int32_t n_rows,
                              uint32_t card, const int64_t* offsets, const uint32_t* min_counts, const uint32_t* n_runs, uint32_t* out_ids, uint32_t* out_counts,
                              int grid, hipStream_t stream);

namespace pg {

namespace {

struct PctlColumn {
  Column* col = nullptr;    // the column the segment knows by name
  Column* ids = nullptr;    // its fixed-bit ids
  std::vector<int> aggs;    // the PERCENTILE aggregations over it (indexes into the query's)
  std::vector<int> modes;   // the MODE aggregations over it ...
  std::vector<int32_t> reducers;   // ... and their pg_mode_reducer
  const char* fn() const { return aggs.empty() ? "MODE" : "PERCENTILE"; }   // how a message names the column's aggregation
  bool lds = false, sort = false;
  uint64_t n_keys = 0;
};
struct PctlPlan {
  SideGroups groups;
  std::vector<PctlColumn> cols;
  const char* who = "PERCENTILE";   // the path in messages: "MODE" for a query whose counting aggregations are all MODEs
  int n_columns_read = 0;       // distinct columns the query projects (ProjectOperator#getNumColumnsProjected)
};

PctlPlan pctl_plan(Segment& seg, const pg_query& q) {
  bool any_percentile = false;
  for (int a = 0; q.aggregations && a < q.n_aggregations; a++) any_percentile |= q.aggregations[a].function == PG_AGG_PERCENTILE;
  const char* kWho = any_percentile ? "PERCENTILE" : "MODE";
  side_query_check(q, kWho);
  const bool null_handling = (q.flags & PG_QUERY_FLAG_NULL_HANDLING) != 0;
  PctlPlan P;
  P.who = kWho;
  std::set<std::string> read;
  std::lock_guard<std::mutex> lock(seg.mu);   // virtual dictionaries are built under the segment's lock
  for (int a = 0; a < q.n_aggregations; a++) {
    const pg_agg_spec& s = q.aggregations[a];
    auto column_of = [&](Column* c) -> PctlColumn& {   // PERCENTILEs and MODEs of one column share its pass
      size_t k = 0;
      while (k < P.cols.size() && P.cols[k].col != c) k++;
      if (k == P.cols.size()) {
        PctlColumn pc;
        pc.col = c;
        P.cols.push_back(pc);
      }
      return P.cols[k];
    };
    if (s.function == PG_AGG_MODE) {   // "x" or "x,'MAX'": the column alone is read; no agg_params entry
      ModeSpec ms;
      std::string error;
      const int32_t st = mode_parse_arguments(s.column, ms, error);
      if (st != PG_OK) fail(st, "%s", error.c_str());
      if (ms.column == "*") fail(PG_ERR_INVALID_ARGUMENT, "MODE needs a column");
      if (expr_is_expression(ms.column.c_str())) fail(PG_ERR_UNSUPPORTED, "MODE over an expression (%s): the Java plan answers", ms.column.c_str());
      Column* c = side_argument_column(seg, ms.column.c_str(), "MODE", "column", nullptr, " (the Java plan answers)", null_handling);
      read.insert(ms.column);
      PctlColumn& pc = column_of(c);
      pc.modes.push_back(a);
      pc.reducers.push_back(ms.reducer);
      continue;
    }
    if (s.column && strcmp(s.column, "*") != 0) read.insert(s.column);
    if (s.function != PG_AGG_PERCENTILE) continue;
    if (!q.agg_params) fail(PG_ERR_INVALID_ARGUMENT, "PERCENTILE without agg_params");
    const double p = q.agg_params[a];
    if (!(p >= 0.0 && p <= 100.0)) fail(PG_ERR_INVALID_ARGUMENT, "PERCENTILE(%s, %g): the percentile must be in [0, 100]", s.column ? s.column : "*", p);
    if (!s.column || strcmp(s.column, "*") == 0) fail(PG_ERR_INVALID_ARGUMENT, "PERCENTILE needs a column");
    // (no layout check: the pass counts ids — the column's dictIds, or its virtual dictionary's, id_column below)
    Column* c = side_argument_column(seg, s.column, kWho, "column", nullptr, " (PERCENTILEMV stays with the Java plan)", null_handling);
    column_of(c).aggs.push_back(a);
  }
  P.groups = side_groups(seg, q, kWho, kWho, read);   // (a refusal names the path: MODE in a query without a PERCENTILE)
  P.n_columns_read = (int)read.size();
  const Knobs& K = knobs();
  for (PctlColumn& pc : P.cols) {
    pc.ids = id_column(seg, *pc.col, "aggregated", kWho);
    const uint64_t C = (uint64_t)pc.ids->cardinality;
    pc.n_keys = P.groups.G * C;   // < 2^63
    pc.sort = pc.n_keys >= 0xFFFFFFFFull || pc.n_keys * 4 > (uint64_t)K.pctl_hbm_max_bytes;   // no dense table: the sort tier
    pc.lds = !pc.sort && pc.n_keys <= (uint64_t)std::min<int64_t>(K.pctl_lds_max_keys, PG_PCTL_LDS_KEYS);
  }
  return P;
}

// MODE's keys are typed by the column's stored type: an INT / LONG key exactly in *l, a FLOAT (widened exactly) / DOUBLE key in *d
int key_kind(const Column& col) { return col.data_type == PG_TYPE_INT ? 0 : col.data_type == PG_TYPE_LONG ? 1 : col.data_type == PG_TYPE_FLOAT ? 2 : 3; }
void key_of_id(const Column& col, const Column& ids, int32_t id, int64_t* l, double* d) {
  if (!col.has_dictionary) {
    *l = vdict_value_of_key(ids.vdict_keys[(size_t)id], ids.vdict_kind, d);
    return;
  }
  const uint8_t* p = col.dict_host.data() + (size_t)id * (col.data_type == PG_TYPE_INT || col.data_type == PG_TYPE_FLOAT ? 4 : 8);
  uint64_t u = 0;
  for (int b = 0; b < (col.data_type == PG_TYPE_INT || col.data_type == PG_TYPE_FLOAT ? 4 : 8); b++) u = (u << 8) | p[b];   // big-endian
  switch (col.data_type) {
    case PG_TYPE_INT: *l = (int64_t)(int32_t)(uint32_t)u; *d = (double)*l; break;
    case PG_TYPE_LONG: *l = (int64_t)u; *d = (double)*l; break;
    case PG_TYPE_FLOAT: { const uint32_t w = (uint32_t)u; float f; memcpy(&f, &w, 4); *d = (double)f; memcpy(l, d, 8); break; }
    default: memcpy(d, &u, 8); *l = (int64_t)u; break;
  }
}

double value_of_id(const Column& col, const Column& ids, int32_t id) {   // Dictionary#getDoubleValue / the raw value as getDoubleValuesSV gives it
  if (col.has_dictionary) return dictionary_value_as_double(col, id);
  double d = 0;
  (void)vdict_value_of_key(ids.vdict_keys[(size_t)id], ids.vdict_kind, &d);
  return d;
}

}  // namespace

// the counting path's test: PERCENTILE or MODE
bool is_percentile_agg(const pg_agg_spec& s) { return s.function == PG_AGG_PERCENTILE || s.function == PG_AGG_MODE; }
void percentile_plan_check(Segment& seg, const pg_query& q) { (void)pctl_plan(seg, q); }

std::unique_ptr<Result> execute_percentile(Segment& seg, const pg_query& q, const CancelToken* cancel) {
  const double t0 = now_ms();
  use_device(seg.device);
  const PctlPlan P = pctl_plan(seg, q);
  const double t_plan = now_ms();
  const bool final_values = (q.flags & PG_QUERY_FLAG_FINAL_PERCENTILE) != 0;   // each flag governs its own function only
  const bool final_modes = (q.flags & PG_QUERY_FLAG_FINAL_MODE) != 0;
  SideBaseQuery B;
  side_base_query(q, B);
  SidePass S = side_pass_begin(seg, q, B, P.groups, P.who, cancel);
  const int32_t n_rows = S.n_rows;
  const int64_t M = S.M, n_words = S.n_words;
  const int cus = S.cus;
  hipStream_t stream = S.stream;
  DeviceBuffer d_rows((size_t)std::max(n_rows, 1) * 4);
  if (n_rows > 0) PG_HIP(hipMemcpyAsync(d_rows.ptr, S.rows.data(), (size_t)n_rows * 4, hipMemcpyHostToDevice, stream));
  std::vector<AggResult> out((size_t)q.n_aggregations);
  const char* kernel = "";
  int64_t pass_bytes = 0;
  int32_t passes = 0;
  // PG_QUERY_FLAG_PROFILE: the counting passes and what follows them (selection, runs, ties and their copies) between two events of their own
  ProfileTimer timer(q.flags);
  timer.start(stream);
  for (const PctlColumn& pc : P.cols) {
    // ---- the counting pass ---------------------------------------------------------------------------------------------------------------
    const uint32_t C = (uint32_t)pc.ids->cardinality;
    const int kind = key_kind(*pc.col);
    DeviceBuffer table;
    if (!pc.sort) {
      table.alloc((size_t)pc.n_keys * 4);
      PG_HIP(hipMemsetAsync(table.ptr, 0, (size_t)pc.n_keys * 4, stream));
    }
    PgPctlArgs A;
    memset(&A, 0, sizeof(A));
    const int64_t id_bits = pc.ids->bits + side_scan_fill(A.scan, seg, S, P.groups);
    A.vcol.data = pc.ids->fwd_dev.as<uint8_t>();
    A.vcol.bits = pc.ids->bits;
    A.vcol.card = pc.ids->cardinality;
    A.vcol.mult = 1;
    A.card = C;
    A.n_keys = pc.sort ? 0u : (uint32_t)pc.n_keys;
    A.table = table.as<uint32_t>();
    PctlSortRuns runs_dev;
    if (pc.sort) {
      const size_t need = pctl_sort_bytes(M);
      if ((int64_t)need > knobs().pctl_sort_max_bytes)
        fail(PG_ERR_UNSUPPORTED, "%s(%s): sorting the keys of %lld matching docs needs a work area of %llu bytes, more than PG_PCTL_SORT_MAX_BYTES (%lld)",
             pc.fn(), pc.col->name.c_str(), (long long)M, (unsigned long long)need, (long long)knobs().pctl_sort_max_bytes);
      int key_bits = 1;
      while (key_bits < 64 && ((pc.n_keys - 1) >> key_bits) != 0) key_bits++;
      pctl_sort_build(A, M, key_bits, stream, runs_dev);
    } else if (M > 0 && n_words > 0) {
      const int64_t words_per_wg = pc.lds ? 64 : 16;
      const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(pc.lds ? cus : cus * 8, (n_words + words_per_wg - 1) / words_per_wg));
      pg_pctl_launch_count(&A, pc.lds ? 1 : 0, grid, stream);
      PG_HIP(hipGetLastError());
    }
    kernel = pc.sort ? "pg_pctl_sort" : pc.lds ? "pg_pctl_lds" : "pg_pctl_hbm";
    passes++;
    pass_bytes += ((int64_t)seg.total_docs * id_bits + 7) / 8 + (S.ds ? n_words * 8 : 0);
    if (n_rows == 0) {
      for (int a : pc.aggs) { out[(size_t)a].kind = final_values ? PG_RESULT_DOUBLE : PG_RESULT_VALUE_COUNTS; out[(size_t)a].param = q.agg_params[a]; }
      for (int a : pc.modes) { out[(size_t)a].kind = final_modes ? PG_RESULT_DOUBLE : PG_RESULT_VALUE_COUNT_MAP; out[(size_t)a].set_value_kind = kind; }
      wait_stream(stream, cancel);
      continue;
    }
    // ---- rank selection over the admitted groups' rows (a column with PERCENTILEs) ----------------------------------------------------------
    const int n_p = (int)pc.aggs.size();
    DeviceBuffer d_totals((size_t)n_rows * 8), d_nnz((size_t)n_rows * 4), d_sel((size_t)n_rows * PG_PCTL_MAX_P * 4), d_first((size_t)n_rows * 8);
    std::vector<int64_t> totals((size_t)n_rows);
    std::vector<uint32_t> nnz((size_t)n_rows);
    std::vector<std::vector<int32_t>> sel;   // per chunk of PG_PCTL_MAX_P percentiles: [n_rows][n]
    const int sel_grid = (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)cus * 8, ((int64_t)n_rows + 3) / 4));
    for (int k0 = 0; k0 < n_p; k0 += PG_PCTL_MAX_P) {
      const int n = std::min(PG_PCTL_MAX_P, n_p - k0);
      if (pc.sort) {
        PgPctlSortSelectArgs S;
        memset(&S, 0, sizeof(S));
        S.run_keys = runs_dev.keys.as<uint64_t>();
        S.run_cum = runs_dev.cum.as<uint64_t>();
        S.n_runs = runs_dev.n_runs;
        S.rows = d_rows.as<uint32_t>();
        S.n_rows = n_rows;
        S.card = C;
        S.n_p = n;
        for (int k = 0; k < n; k++) S.p[k] = q.agg_params[pc.aggs[(size_t)(k0 + k)]];
        S.totals = d_totals.as<int64_t>();
        S.nnz = d_nnz.as<uint32_t>();
        S.first_run = d_first.as<int64_t>();
        S.sel = d_sel.as<int32_t>();
        pg_pctl_launch_sort_select(&S, stream);
      } else {
        PgPctlSelectArgs S;
        memset(&S, 0, sizeof(S));
        S.table = table.as<uint32_t>();
        S.rows = d_rows.as<uint32_t>();
        S.n_rows = n_rows;
        S.card = C;
        S.n_p = n;
        for (int k = 0; k < n; k++) S.p[k] = q.agg_params[pc.aggs[(size_t)(k0 + k)]];
        S.totals = d_totals.as<int64_t>();
        S.nnz = d_nnz.as<uint32_t>();
        S.sel = d_sel.as<int32_t>();
        pg_pctl_launch_select(&S, sel_grid, stream);
      }
      PG_HIP(hipGetLastError());
      sel.emplace_back((size_t)n_rows * (size_t)n);
      PG_HIP(hipMemcpyAsync(sel.back().data(), d_sel.ptr, sel.back().size() * 4, hipMemcpyDeviceToHost, stream));
      if (k0 + PG_PCTL_MAX_P < n_p) wait_stream(stream, cancel);   // d_sel is reused by the next chunk
    }
    if (n_p > 0) {
      PG_HIP(hipMemcpyAsync(totals.data(), d_totals.ptr, (size_t)n_rows * 8, hipMemcpyDeviceToHost, stream));
      PG_HIP(hipMemcpyAsync(nnz.data(), d_nnz.ptr, (size_t)n_rows * 4, hipMemcpyDeviceToHost, stream));
    }
    // ---- the mode selection (a column with MODEs): the rows' partials, and their n and non-zero counters whichever selection ran ----------------
    std::vector<PgModeRow> mode_rows;
    DeviceBuffer d_mode, d_parts;
    if (!pc.modes.empty()) {
      mode_rows.resize((size_t)n_rows);
      d_mode.alloc((size_t)n_rows * sizeof(PgModeRow));
      if (pc.sort) {
        PgModeSortSelectArgs MS;
        memset(&MS, 0, sizeof(MS));
        MS.run_keys = runs_dev.keys.as<uint64_t>();
        MS.run_counts = runs_dev.counts.as<uint32_t>();
        MS.n_runs = runs_dev.n_runs;
        MS.rows = d_rows.as<uint32_t>();
        MS.n_rows = n_rows;
        MS.card = C;
        MS.out = d_mode.as<PgModeRow>();
        MS.first_run = d_first.as<int64_t>();
        pg_mode_launch_sort_select(&MS, sel_grid, stream);
      } else {
        // Few wide rows are spread over wavefronts: below two wavefronts per SIMD (8 per CU) a row is cut into shares of at least
        // Knobs::mode_split_ids ids, and pg_mode_finish combines them.  With many rows one wavefront walks its row alone.
        const int64_t want = (int64_t)cus * 8;
        const int64_t split = std::max<int64_t>(64, knobs().mode_split_ids);
        int64_t shares = 1;
        if (n_rows < want) shares = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(((int64_t)C + split - 1) / split, (want + n_rows - 1) / n_rows), PG_MODE_MAX_SHARES));
        const int64_t per = (((int64_t)C + shares - 1) / shares + 63) / 64 * 64;
        PgModeSelectArgs MS;
        memset(&MS, 0, sizeof(MS));
        MS.table = table.as<uint32_t>();
        MS.rows = d_rows.as<uint32_t>();
        MS.n_rows = n_rows;
        MS.card = C;
        MS.shares = (uint32_t)shares;
        MS.share_ids = (uint32_t)std::min<int64_t>(per, 0xFFFFFFC0ll);
        if (shares > 1) d_parts.alloc((size_t)n_rows * (size_t)shares * sizeof(PgModeRow));
        MS.out = shares > 1 ? d_parts.as<PgModeRow>() : d_mode.as<PgModeRow>();
        const int64_t items = (int64_t)n_rows * shares;
        pg_mode_launch_select(&MS, (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)cus * 8, (items + 3) / 4)), stream);
        if (shares > 1) {
          PG_HIP(hipGetLastError());
          pg_mode_launch_finish(d_parts.as<PgModeRow>(), n_rows, (uint32_t)shares, d_mode.as<PgModeRow>(), sel_grid, stream);
        }
      }
      PG_HIP(hipGetLastError());
      PG_HIP(hipMemcpyAsync(mode_rows.data(), d_mode.ptr, (size_t)n_rows * sizeof(PgModeRow), hipMemcpyDeviceToHost, stream));
    }
    wait_stream(stream, cancel);
    if (n_p == 0)
      for (int32_t i = 0; i < n_rows; i++) { totals[(size_t)i] = (int64_t)mode_rows[(size_t)i].n; nnz[(size_t)i] = mode_rows[(size_t)i].nnz; }
    if (q.n_group_by == 0 && totals[0] != M)
      fail(PG_ERR_INTERNAL, "%s(%s): %lld values counted for %lld matching docs", pc.fn(), pc.col->name.c_str(), (long long)totals[0], (long long)M);
    for (const PgModeRow& r : mode_rows)
      if (r.p.n_tied > r.nnz || (r.p.n_tied > 0 && (r.p.lo > r.p.hi || r.p.hi >= C)) || (r.p.n_tied == 0) != (r.nnz == 0))
        fail(PG_ERR_INTERNAL, "MODE(%s): %u ids tied between %u and %u of %u, %u counted", pc.col->name.c_str(), r.p.n_tied, r.p.lo, r.p.hi, C, r.nnz);
    if (final_values) {
      for (int k = 0; k < n_p; k++) {
        AggResult& r = out[(size_t)pc.aggs[(size_t)k]];
        r.kind = PG_RESULT_DOUBLE;
        r.param = q.agg_params[pc.aggs[(size_t)k]];
        r.d[0].resize((size_t)n_rows);
        const std::vector<int32_t>& s = sel[(size_t)(k / PG_PCTL_MAX_P)];
        const int n = std::min(PG_PCTL_MAX_P, n_p - k / PG_PCTL_MAX_P * PG_PCTL_MAX_P);
        for (int32_t i = 0; i < n_rows; i++) {
          const int32_t id = s[(size_t)i * (size_t)n + (size_t)(k % PG_PCTL_MAX_P)];
          if (id >= (int32_t)C) fail(PG_ERR_INTERNAL, "PERCENTILE(%s): selected id %d of %u", pc.col->name.c_str(), id, C);
          r.d[0][(size_t)i] = id < 0 ? -std::numeric_limits<double>::infinity() : value_of_id(*pc.col, *pc.ids, id);
        }
      }
    }
    // Compacted (id, count) runs of the rows: the non-zero ones (threshold 1: the intermediate forms), or those reaching a row's threshold
    auto compact = [&](const std::vector<int64_t>& off, const std::vector<uint32_t>* least, std::vector<uint32_t>& run_ids, std::vector<uint32_t>& run_counts) {
      const int64_t n_runs = off[(size_t)n_rows];
      run_ids.assign((size_t)n_runs, 0u);
      run_counts.assign((size_t)n_runs, 0u);
      if (n_runs == 0) return;
      DeviceBuffer d_off(off.size() * 8), d_ids((size_t)n_runs * 4), d_counts((size_t)n_runs * 4), d_least, d_in_row;
      PG_HIP(hipMemcpyAsync(d_off.ptr, off.data(), off.size() * 8, hipMemcpyHostToDevice, stream));
      if (least) {
        d_least.alloc((size_t)n_rows * 4);
        PG_HIP(hipMemcpyAsync(d_least.ptr, least->data(), (size_t)n_rows * 4, hipMemcpyHostToDevice, stream));
        if (pc.sort) {
          d_in_row.alloc((size_t)n_rows * 4);
          PG_HIP(hipMemcpyAsync(d_in_row.ptr, nnz.data(), (size_t)n_rows * 4, hipMemcpyHostToDevice, stream));
        }
      }
      if (pc.sort)
        pg_pctl_launch_sort_runs(runs_dev.keys.as<uint64_t>(), runs_dev.counts.as<uint32_t>(), d_rows.as<uint32_t>(), d_first.as<int64_t>(), n_rows, C, d_off.as<int64_t>(),
                                 least ? d_least.as<uint32_t>() : nullptr, least ? d_in_row.as<uint32_t>() : nullptr, d_ids.as<uint32_t>(), d_counts.as<uint32_t>(), sel_grid, stream);
      else
        pg_pctl_launch_runs(table.as<uint32_t>(), d_rows.as<uint32_t>(), n_rows, C, d_off.as<int64_t>(), least ? d_least.as<uint32_t>() : nullptr, d_ids.as<uint32_t>(),
                            d_counts.as<uint32_t>(), sel_grid, stream);
      PG_HIP(hipGetLastError());
      PG_HIP(hipMemcpyAsync(run_ids.data(), d_ids.ptr, (size_t)n_runs * 4, hipMemcpyDeviceToHost, stream));
      PG_HIP(hipMemcpyAsync(run_counts.data(), d_counts.ptr, (size_t)n_runs * 4, hipMemcpyDeviceToHost, stream));
      wait_stream(stream, cancel);
      for (int64_t e = 0; e < n_runs; e++)
        if (run_ids[(size_t)e] >= C || run_counts[(size_t)e] == 0) fail(PG_ERR_INTERNAL, "%s(%s): run id %u of %u, count %u", pc.fn(), pc.col->name.c_str(), run_ids[(size_t)e], C, run_counts[(size_t)e]);
    };
    // ---- MODE's final values, from the partials ------------------------------------------------------------------------------------------------
    if (final_modes && !pc.modes.empty()) {
      const bool any_avg = std::find(pc.reducers.begin(), pc.reducers.end(), (int32_t)PG_MODE_AVG) != pc.reducers.end();
      std::vector<int64_t> tie_off((size_t)n_rows + 1, 0);   // AVG over more than two ties needs every tied id; up to two are lo and hi
      std::vector<uint32_t> least((size_t)n_rows, 1u), tie_ids, tie_counts;
      if (any_avg) {
        for (int32_t i = 0; i < n_rows; i++) {
          const pg_mode_partial& p = mode_rows[(size_t)i].p;
          tie_off[(size_t)i + 1] = tie_off[(size_t)i] + (p.n_tied > 2 ? p.n_tied : 0u);
          least[(size_t)i] = std::max(1u, p.max_count);
        }
        compact(tie_off, &least, tie_ids, tie_counts);
      }
      std::vector<double> avg;
      if (any_avg) {
        avg.resize((size_t)n_rows);
        std::vector<double> tied;
        for (int32_t i = 0; i < n_rows; i++) {
          const pg_mode_partial& p = mode_rows[(size_t)i].p;
          if (p.n_tied == 0) { avg[(size_t)i] = -std::numeric_limits<double>::infinity(); continue; }
          tied.clear();
          if (p.n_tied <= 2) {
            tied.push_back(value_of_id(*pc.col, *pc.ids, (int32_t)p.lo));
            if (p.n_tied == 2) tied.push_back(value_of_id(*pc.col, *pc.ids, (int32_t)p.hi));
          } else {
            for (int64_t e = tie_off[(size_t)i]; e < tie_off[(size_t)i + 1]; e++) {
              if (tie_counts[(size_t)e] != p.max_count) fail(PG_ERR_INTERNAL, "MODE(%s): a tied id counted %u, the greatest count is %u", pc.col->name.c_str(), tie_counts[(size_t)e], p.max_count);
              tied.push_back(value_of_id(*pc.col, *pc.ids, (int32_t)tie_ids[(size_t)e]));
            }
          }
          avg[(size_t)i] = mode_exact_sum(tied.data(), tied.size()) / (double)p.n_tied;   // the exact sum rounded once, then one division
        }
      }
      for (size_t k = 0; k < pc.modes.size(); k++) {
        AggResult& r = out[(size_t)pc.modes[k]];
        r.kind = PG_RESULT_DOUBLE;
        if (pc.reducers[k] == PG_MODE_AVG) { r.d[0] = avg; continue; }
        r.d[0].resize((size_t)n_rows);
        for (int32_t i = 0; i < n_rows; i++) {
          const pg_mode_partial& p = mode_rows[(size_t)i].p;
          r.d[0][(size_t)i] = p.n_tied == 0 ? -std::numeric_limits<double>::infinity() : value_of_id(*pc.col, *pc.ids, (int32_t)(pc.reducers[k] == PG_MODE_MAX ? p.hi : p.lo));
        }
      }
    }
    const bool pctl_runs = !final_values && n_p > 0, mode_runs = !final_modes && !pc.modes.empty();
    if (!pctl_runs && !mode_runs) continue;
    // ---- the rows' non-zero runs -------------------------------------------------------------------------------------------------------------
    std::vector<int64_t> off((size_t)n_rows + 1, 0);
    for (int32_t i = 0; i < n_rows; i++) off[(size_t)i + 1] = off[(size_t)i] + nnz[(size_t)i];
    const int64_t n_runs = off[(size_t)n_rows];
    std::vector<uint32_t> run_ids, run_counts;
    compact(off, nullptr, run_ids, run_counts);
    if (pctl_runs) {
      AggResult runs;
      runs.kind = PG_RESULT_VALUE_COUNTS;
      runs.set_sizes.assign(nnz.begin(), nnz.end());
      runs.d[0].resize((size_t)n_runs);
      runs.l[0].resize((size_t)n_runs);
      for (int64_t e = 0; e < n_runs; e++) {
        runs.d[0][(size_t)e] = value_of_id(*pc.col, *pc.ids, (int32_t)run_ids[(size_t)e]);
        runs.l[0][(size_t)e] = run_counts[(size_t)e];
      }
      for (int a : pc.aggs) {
        out[(size_t)a] = runs;
        out[(size_t)a].param = q.agg_params[a];
      }
    }
    if (mode_runs) {   // the map value -> count, ascending by key (the id order); keys exact in the column's stored type
      AggResult map;
      map.kind = PG_RESULT_VALUE_COUNT_MAP;
      map.set_value_kind = kind;
      map.set_sizes.assign(nnz.begin(), nnz.end());
      map.l[0].resize((size_t)n_runs);
      map.l[1].resize((size_t)n_runs);
      map.d[0].resize((size_t)n_runs);
      for (int64_t e = 0; e < n_runs; e++) {
        key_of_id(*pc.col, *pc.ids, (int32_t)run_ids[(size_t)e], &map.l[1][(size_t)e], &map.d[0][(size_t)e]);
        map.l[0][(size_t)e] = run_counts[(size_t)e];
      }
      for (int a : pc.modes) out[(size_t)a] = map;
    }
  }
  const float pass_ms = timer.stop_ms();
  std::unique_ptr<Result> res = side_pass_finish(seg, q, B, S, out, {kernel, pass_bytes, P.n_columns_read, pass_ms, t0, t_plan});
  for (const PctlColumn& pc : P.cols) res->merged_elsewhere |= (pc.aggs.empty() ? 0u : MERGED_PERCENTILE) | (pc.modes.empty() ? 0u : MERGED_MODE);
  res->stats.percentile_passes = passes;
  return res;
}

}  // namespace pg
