// Queries with a SKEWNESS / KURTOSIS aggregation (PG_AGG_SKEWNESS / PG_AGG_KURTOSIS): a side pass joined to the ordinary plan by group key,
// in the frame of pg_exec_sidepass.hip (which runs step 1 and the filter, maps the admitted groups to rows and joins the result, step 4).
//   1. The ordinary part — the query without these aggregations (COUNT(*) if nothing else remains) — runs through execute_query unchanged,
//      never on a star-tree: it decides the groups, the numGroupsLimit admission and the other aggregations' results (a variance aggregation
//      or a PERCENTILE among them takes its own side pass from there).  An ORDER BY that names one of them leaves the segment untrimmed.
//   2. One accumulation pass for ALL of them over the filter's match words into a table [G][slots] of int64: slot 0 the doc count, then per
//      distinct argument column (at most PG_MOMENT_MAX_COLS; SKEWNESS(x), KURTOSIS(x) share one) the exact power sums of pg_moment4.h.
//      pg_moment_reg without GROUP BY, pg_moment_lds up to PG_MOMENT_LDS_SLOTS slots, pg_moment_hbm up to Knobs::moment_hbm_max_bytes;
//      beyond that the query is refused.
//   3. The rows of the admitted groups are gathered on the device (pg_expr_gather); the host forms m1 .. m4, each rounded once.
//   4. The tuples are joined to the ordinary part on the host.
// The kernels are those of pg_kernels_moment.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <set>
#include <string>

#include "pg_internal.hpp"
#include "pg_fixed_point.h"
#include "pg_moments.h"
#include "pg_moment4.h"

void pg_moment_launch_pass(const PgMomentArgs* args, int tier, int grid, hipStream_t stream);
void pg_expr_launch_gather(const int64_t* table, const uint32_t* rows, int32_t n_rows, int32_t slots, uint64_t n_groups, int64_t* out, int grid, hipStream_t stream);

namespace pg {
namespace {

const char* kWho = "fourth-moment";
const char* kSubject = "a SKEWNESS / KURTOSIS aggregation";
const char* const kTierKernel[3] = {"pg_moment_reg", "pg_moment_lds", "pg_moment_hbm"};

struct MomentColumn {
  Column* col = nullptr;
  std::vector<int> aggs;    // the aggregations over it (indexes into the query's)
  bool is_int = false;      // the integer path
  int exp = 0;              // double path: every finite |value| < 2^exp
  int32_t first_slot = 0;
};
struct MomentPlan {
  SideGroups groups;
  std::vector<MomentColumn> cols;
  int32_t slots = 1;            // slot 0: the doc count
  uint64_t n_slots = 0;
  int tier = TIER_REG;
  int n_columns_read = 0;       // distinct columns the query projects (ProjectOperator#getNumColumnsProjected)
};

MomentPlan moment_plan(Segment& seg, const pg_query& q) {
  side_query_check(q, kSubject);
  const bool null_handling = (q.flags & PG_QUERY_FLAG_NULL_HANDLING) != 0;
  MomentPlan P;
  std::set<std::string> read;
  std::lock_guard<std::mutex> lock(seg.mu);   // virtual dictionaries are built under the segment's lock
  for (int a = 0; a < q.n_aggregations; a++) {
    const pg_agg_spec& s = q.aggregations[a];
    if (!is_moment_agg(s)) {
      if (s.column && strcmp(s.column, "*") != 0) read.insert(s.column);
      continue;
    }
    const char* fn = agg_function_text(s.function);
    if (!s.column || strcmp(s.column, "*") == 0) fail(PG_ERR_INVALID_ARGUMENT, "%s needs a column", fn);
    Column* c = side_argument_column(seg, s.column, fn, "column", "argument column", "", null_handling);
    read.insert(c->name);
    if (c->val_type == PG_V_F32 || c->val_type == PG_V_F64) {
      // the registration pass (pg_segment.cpp) knows every FLOAT / DOUBLE column's non-finite values: the power sums have no digits for them
      if (c->has_nonfinite) fail(PG_ERR_UNSUPPORTED, "%s over %s, which holds a NaN or an infinity: the Java plan answers such a query", fn, c->name.c_str());
      if (pg_m4_overflows(c->fx_exp))
        fail(PG_ERR_UNSUPPORTED, "%s over %s: the column's bound 2^%d admits a fourth power that overflows a double: the Java plan answers such a query", fn,
             c->name.c_str(), c->fx_exp);
    }
    size_t k = 0;
    while (k < P.cols.size() && P.cols[k].col != c) k++;
    if (k == P.cols.size()) {
      if (k >= PG_MOMENT_MAX_COLS) fail(PG_ERR_UNSUPPORTED, "SKEWNESS / KURTOSIS aggregations over more than %d distinct columns in one query", PG_MOMENT_MAX_COLS);
      MomentColumn mc;
      mc.col = c;
      mc.is_int = c->val_type == PG_V_I32;
      mc.exp = c->val_type == PG_V_I64 ? PG_VAR_LONG_EXP : c->fx_exp;
      mc.first_slot = P.slots;
      P.slots += mc.is_int ? PG_M4_INT_SLOTS : PG_M4_DBL_SLOTS;
      P.cols.push_back(mc);
    }
    P.cols[k].aggs.push_back(a);
  }
  P.groups = side_groups(seg, q, kSubject, kWho, read);
  P.n_columns_read = (int)read.size();
  P.n_slots = P.groups.G * (uint64_t)P.slots;   // < 2^38
  const Knobs& K = knobs();
  P.tier = side_tier(q.n_group_by, P.n_slots, PG_MOMENT_LDS_SLOTS, P.n_slots * 8, K.moment_hbm_max_bytes);
  if (P.tier == TIER_REFUSED)
    fail(PG_ERR_UNSUPPORTED, "SKEWNESS / KURTOSIS aggregations: %llu groups x %d slots need a table of %llu bytes, more than PG_MOMENT_HBM_MAX_BYTES (%lld)",
         (unsigned long long)P.groups.G, P.slots, (unsigned long long)(P.n_slots * 8), (long long)K.moment_hbm_max_bytes);
  return P;
}

}  // namespace

bool is_moment_function(int32_t fn) { return fn == PG_AGG_SKEWNESS || fn == PG_AGG_KURTOSIS; }
bool is_moment_agg(const pg_agg_spec& s) { return is_moment_function(s.function); }
void moment_plan_check(Segment& seg, const pg_query& q) { (void)moment_plan(seg, q); }

std::unique_ptr<Result> execute_moment(Segment& seg, const pg_query& q, const CancelToken* cancel) {
  const double t0 = now_ms();
  use_device(seg.device);
  const MomentPlan P = moment_plan(seg, q);
  const double t_plan = now_ms();
  SideBaseQuery B;
  side_base_query(q, B);
  SidePass S = side_pass_begin(seg, q, B, P.groups, kWho, cancel);
  const int32_t n_rows = S.n_rows;
  const int64_t M = S.M, n_words = S.n_words;
  const int cus = S.cus;
  hipStream_t stream = S.stream;
  // ---- the accumulation pass -------------------------------------------------------------------------------------------------------------------
  PgMomentArgs A;
  memset(&A, 0, sizeof(A));
  int64_t doc_bits = side_scan_fill(A.scan, seg, S, P.groups);
  A.n_cols = (int32_t)P.cols.size();
  A.slots = P.slots;
  A.n_groups = P.groups.G;
  A.n_slots = P.n_slots;
  for (size_t i = 0; i < P.cols.size(); i++) {
    const MomentColumn& mc = P.cols[i];
    PgMomentCol& C = A.cols[i];
    expr_fill_src(C.src, *mc.col);
    C.is_int = mc.is_int ? 1 : 0;
    C.first_slot = mc.first_slot;
    C.q1 = pg_var_q1(mc.exp);
    C.q2 = pg_var_q2(mc.exp);
    C.q3 = pg_m4_q3(mc.exp);
    C.q4 = pg_m4_q4(mc.exp);
    doc_bits += value_src_bits(*mc.col);
  }
  DeviceBuffer table((size_t)P.n_slots * 8);
  A.table = table.as<int64_t>();
  // PG_QUERY_FLAG_PROFILE: the pass (initialisation, accumulation, gather and its copy) between two events of its own
  ProfileTimer timer(q.flags);
  timer.start(stream);
  PG_HIP(hipMemsetAsync(table.ptr, 0, (size_t)P.n_slots * 8, stream));
  if (M > 0 && n_words > 0) {
    pg_moment_launch_pass(&A, P.tier, side_pass_grid(P.tier, cus, n_words), stream);
    PG_HIP(hipGetLastError());
  }
  std::vector<int64_t> got((size_t)n_rows * (size_t)P.slots);
  side_gather_rows(S, got, cancel, [&](const uint32_t* rows, int64_t* out) {
    pg_expr_launch_gather(table.as<int64_t>(), rows, n_rows, P.slots, P.groups.G, out, side_flat_grid(cus, (int64_t)got.size()), stream);
  });
  const float pass_ms = timer.stop_ms();
  if (q.n_group_by == 0 && got[0] != M)
    fail(PG_ERR_INTERNAL, "fourth moment: %lld docs counted for %lld matching docs", (long long)got[0], (long long)M);
  // ---- the tuples: (n, m1, m2, m3, m4), each of the four doubles rounded once; (0, NaN, NaN, NaN, NaN) over no doc ---------------------------------
  std::vector<AggResult> out((size_t)q.n_aggregations);
  for (const MomentColumn& mc : P.cols) {
    AggResult r;
    r.kind = PG_RESULT_FOURTH_MOMENT;
    r.l[0].resize((size_t)n_rows);
    for (int k = 0; k < 4; k++) r.d[k].resize((size_t)n_rows);
    const int E = mc.exp;
    const int q1 = mc.is_int ? 0 : pg_var_q1(E), q2 = mc.is_int ? 0 : pg_var_q2(E), q3 = mc.is_int ? 0 : pg_m4_q3(E), q4 = mc.is_int ? 0 : pg_m4_q4(E);
    const int n1 = mc.is_int ? 1 : PG_VAR_SUM_LIMBS, n2 = mc.is_int ? 2 : PG_VAR_SQ_LIMBS, n3 = mc.is_int ? 3 : PG_M4_CUBE_LIMBS, n4 = mc.is_int ? 4 : PG_M4_QUAD_LIMBS;
    for (int32_t i = 0; i < n_rows; i++) {
      const int64_t* row = &got[(size_t)i * (size_t)P.slots];
      const int64_t* s1 = row + mc.first_slot;
      const int64_t n = row[0];
      if (n < 0 || n > M) fail(PG_ERR_INTERNAL, "fourth moment: %lld docs counted in a group of %lld matching docs", (long long)n, (long long)M);
      const pg_m4_tuple t = pg_m4_tuple_of(n, s1, n1, q1, s1 + n1, n2, q2, s1 + n1 + n2, n3, q3, s1 + n1 + n2 + n3, n4, q4);
      r.l[0][(size_t)i] = t.n;
      r.d[0][(size_t)i] = t.m1;
      r.d[1][(size_t)i] = t.m2;
      r.d[2][(size_t)i] = t.m3;
      r.d[3][(size_t)i] = t.m4;
    }
    for (size_t k = 0; k + 1 < mc.aggs.size(); k++) out[(size_t)mc.aggs[k]] = r;
    out[(size_t)mc.aggs.back()] = std::move(r);
  }
  std::unique_ptr<Result> res = side_pass_finish(seg, q, B, S, out, {kTierKernel[P.tier], side_pass_bytes(seg, S, 1, doc_bits), P.n_columns_read, pass_ms, t0, t_plan});
  res->fourth_moment = true;
  return res;
}

}  // namespace pg
