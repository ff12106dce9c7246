// Queries with a VAR_POP / VAR_SAMP / STDDEV_POP / STDDEV_SAMP aggregation (PG_AGG_VARPOP .. PG_AGG_STDDEVSAMP): a side pass joined to the
// ordinary plan by group key, in the frame of pg_exec_sidepass.hip (which runs step 1 and the filter, maps the admitted groups to rows and
// joins the result, step 4).
//   1. The ordinary part — the query without its variance aggregations (COUNT(*) if nothing else remains) — runs through execute_query
//      unchanged, never on a star-tree: it decides the groups, the numGroupsLimit admission and the other aggregations' results (a PERCENTILE
//      among them takes its own side pass from there).  An ORDER BY that names a variance aggregation leaves the segment untrimmed.
//   2. One accumulation pass for ALL variance aggregations of the query over the filter's match words into a table [G][slots] of int64: slot 0
//      the doc count, then per distinct argument column (at most PG_VAR_MAX_COLS; VAR_POP(x), STDDEV_SAMP(x) share one) the exact power sums of
//      pg_moments.h.  pg_var_reg without GROUP BY, pg_var_lds up to PG_VAR_LDS_SLOTS slots, pg_var_hbm up to Knobs::var_hbm_max_bytes;
//      beyond that the query is refused.
//   3. The rows of the admitted groups are gathered on the device (pg_expr_gather); the host forms sum and m2, each rounded once.
//   4. The tuples are joined to the ordinary part on the host.
// The kernels are those of pg_kernels_var.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <set>
#include <string>

#include "pg_internal.hpp"
#include "pg_fixed_point.h"
#include "pg_moments.h"

void pg_var_launch_pass(const PgVarArgs* args, int tier, int grid, hipStream_t stream);
void pg_expr_launch_gather(const int64_t* table, const uint32_t* rows, int32_t n_rows, int32_t slots, uint64_t n_groups, int64_t* out, int grid, hipStream_t stream);

namespace pg {
namespace {

const char* kWho = "variance";
const char* kSubject = "a variance aggregation";
const char* const kTierKernel[3] = {"pg_var_reg", "pg_var_lds", "pg_var_hbm"};

bool is_variance_function(int32_t fn) { return fn >= PG_AGG_VARPOP && fn <= PG_AGG_STDDEVSAMP; }

struct VarColumn {
  Column* col = nullptr;
  std::vector<int> aggs;    // the variance aggregations over it (indexes into the query's)
  bool is_int = false;      // the integer path
  int exp = 0;              // double path: every finite |value| < 2^exp
  int32_t first_slot = 0;
};
struct VarPlan {
  SideGroups groups;
  std::vector<VarColumn> cols;
  int32_t slots = 1;            // slot 0: the doc count
  uint64_t n_slots = 0;
  int tier = TIER_REG;
  int n_columns_read = 0;       // distinct columns the query projects (ProjectOperator#getNumColumnsProjected)
};

VarPlan var_plan(Segment& seg, const pg_query& q) {
  side_query_check(q, kSubject);
  const bool null_handling = (q.flags & PG_QUERY_FLAG_NULL_HANDLING) != 0;
  VarPlan P;
  std::set<std::string> read;
  std::lock_guard<std::mutex> lock(seg.mu);   // virtual dictionaries are built under the segment's lock
  for (int a = 0; a < q.n_aggregations; a++) {
    const pg_agg_spec& s = q.aggregations[a];
    if (s.column && strcmp(s.column, "*") != 0) read.insert(s.column);
    if (!is_variance_agg(s)) continue;
    const char* fn = agg_function_text(s.function);
    if (!s.column || strcmp(s.column, "*") == 0) fail(PG_ERR_INVALID_ARGUMENT, "%s needs a column", fn);
    Column* c = side_argument_column(seg, s.column, fn, "column", "argument column", "", null_handling);
    // the registration pass (pg_segment.cpp) knows every FLOAT / DOUBLE column's non-finite values: the power sums have no digits for them
    if ((c->val_type == PG_V_F32 || c->val_type == PG_V_F64) && c->has_nonfinite)
      fail(PG_ERR_UNSUPPORTED, "%s over %s, which holds a NaN or an infinity: the Java plan answers such a query", fn, c->name.c_str());
    size_t k = 0;
    while (k < P.cols.size() && P.cols[k].col != c) k++;
    if (k == P.cols.size()) {
      if (k >= PG_VAR_MAX_COLS) fail(PG_ERR_UNSUPPORTED, "variance aggregations over more than %d distinct columns in one query", PG_VAR_MAX_COLS);
      VarColumn vc;
      vc.col = c;
      vc.is_int = c->val_type == PG_V_I32;
      vc.exp = c->val_type == PG_V_I64 ? PG_VAR_LONG_EXP : c->fx_exp;
      vc.first_slot = P.slots;
      P.slots += vc.is_int ? PG_VAR_INT_SLOTS : PG_VAR_DBL_SLOTS;
      P.cols.push_back(vc);
    }
    P.cols[k].aggs.push_back(a);
  }
  P.groups = side_groups(seg, q, kSubject, kWho, read);
  P.n_columns_read = (int)read.size();
  P.n_slots = P.groups.G * (uint64_t)P.slots;   // < 2^38
  const Knobs& K = knobs();
  P.tier = side_tier(q.n_group_by, P.n_slots, PG_VAR_LDS_SLOTS, P.n_slots * 8, K.var_hbm_max_bytes);
  if (P.tier == TIER_REFUSED)
    fail(PG_ERR_UNSUPPORTED, "variance aggregations: %llu groups x %d slots need a table of %llu bytes, more than PG_VAR_HBM_MAX_BYTES (%lld)",
         (unsigned long long)P.groups.G, P.slots, (unsigned long long)(P.n_slots * 8), (long long)K.var_hbm_max_bytes);
  return P;
}

}  // namespace

bool is_variance_agg(const pg_agg_spec& s) { return is_variance_function(s.function); }
void variance_plan_check(Segment& seg, const pg_query& q) { (void)var_plan(seg, q); }

std::unique_ptr<Result> execute_variance(Segment& seg, const pg_query& q, const CancelToken* cancel) {
  const double t0 = now_ms();
  use_device(seg.device);
  const VarPlan P = var_plan(seg, q);
  const double t_plan = now_ms();
  SideBaseQuery B;
  side_base_query(q, B);
  SidePass S = side_pass_begin(seg, q, B, P.groups, kWho, cancel);
  const int32_t n_rows = S.n_rows;
  const int64_t M = S.M, n_words = S.n_words;
  const int cus = S.cus;
  hipStream_t stream = S.stream;
  // ---- the accumulation pass -------------------------------------------------------------------------------------------------------------------
  PgVarArgs A;
  memset(&A, 0, sizeof(A));
  int64_t doc_bits = side_scan_fill(A.scan, seg, S, P.groups);
  A.n_cols = (int32_t)P.cols.size();
  A.slots = P.slots;
  A.n_groups = P.groups.G;
  A.n_slots = P.n_slots;
  for (size_t i = 0; i < P.cols.size(); i++) {
    const VarColumn& vc = P.cols[i];
    PgVarCol& C = A.cols[i];
    expr_fill_src(C.src, *vc.col);
    C.is_int = vc.is_int ? 1 : 0;
    C.first_slot = vc.first_slot;
    C.q1 = pg_var_q1(vc.exp);
    C.q2 = pg_var_q2(vc.exp);
    doc_bits += value_src_bits(*vc.col);
  }
  DeviceBuffer table((size_t)P.n_slots * 8);
  A.table = table.as<int64_t>();
  // PG_QUERY_FLAG_PROFILE: the pass (initialisation, accumulation, gather and its copy) between two events of its own
  ProfileTimer timer(q.flags);
  timer.start(stream);
  PG_HIP(hipMemsetAsync(table.ptr, 0, (size_t)P.n_slots * 8, stream));
  if (M > 0 && n_words > 0) {
    pg_var_launch_pass(&A, P.tier, side_pass_grid(P.tier, cus, n_words), stream);
    PG_HIP(hipGetLastError());
  }
  std::vector<int64_t> got((size_t)n_rows * (size_t)P.slots);
  side_gather_rows(S, got, cancel, [&](const uint32_t* rows, int64_t* out) {
    pg_expr_launch_gather(table.as<int64_t>(), rows, n_rows, P.slots, P.groups.G, out, side_flat_grid(cus, (int64_t)got.size()), stream);
  });
  const float pass_ms = timer.stop_ms();
  if (q.n_group_by == 0 && got[0] != M)
    fail(PG_ERR_INTERNAL, "variance: %lld docs counted for %lld matching docs", (long long)got[0], (long long)M);
  // ---- the tuples: (count, sum, m2), each of the two doubles rounded once; (0, 0.0, 0.0) over no doc ----------------------------------------------
  std::vector<AggResult> out((size_t)q.n_aggregations);
  for (const VarColumn& vc : P.cols) {
    AggResult r;
    r.kind = PG_RESULT_VARIANCE_TUPLE;
    r.l[0].resize((size_t)n_rows);
    r.d[0].resize((size_t)n_rows);
    r.d[1].resize((size_t)n_rows);
    const int q1 = vc.is_int ? 0 : pg_var_q1(vc.exp), q2 = vc.is_int ? 0 : pg_var_q2(vc.exp);
    const int n_sx = vc.is_int ? 1 : PG_VAR_SUM_LIMBS, n_sq = vc.is_int ? 2 : PG_VAR_SQ_LIMBS;
    for (int32_t i = 0; i < n_rows; i++) {
      const int64_t* row = &got[(size_t)i * (size_t)P.slots];
      const int64_t* sx = row + vc.first_slot;
      const int64_t n = row[0];
      if (n < 0 || n > M) fail(PG_ERR_INTERNAL, "variance: %lld docs counted in a group of %lld matching docs", (long long)n, (long long)M);
      r.l[0][(size_t)i] = n;
      r.d[0][(size_t)i] = pg_limbs_to_double(sx, n_sx, q1);
      r.d[1][(size_t)i] = pg_var_m2(n, sx, n_sx, q1, sx + n_sx, n_sq, q2);
    }
    for (size_t k = 0; k + 1 < vc.aggs.size(); k++) out[(size_t)vc.aggs[k]] = r;
    out[(size_t)vc.aggs.back()] = std::move(r);
  }
  std::unique_ptr<Result> res = side_pass_finish(seg, q, B, S, out, {kTierKernel[P.tier], side_pass_bytes(seg, S, 1, doc_bits), P.n_columns_read, pass_ms, t0, t_plan});
  res->variance = true;
  return res;
}

}  // namespace pg
