// Queries with a VAR_POP / VAR_SAMP / STDDEV_POP / STDDEV_SAMP aggregation (PG_AGG_VARPOP .. PG_AGG_STDDEVSAMP): a side pass joined to the
// ordinary plan by group key.  The pass is the sum-table pass of pg_exec_sidepass.hip (SumTablePass: the ordinary part, the filter's match
// words, the table, the timed accumulation and gather, the doc-count checks, the join and the statistics); this file holds what is the
// path's own:
//   the plan     one table [G][slots] of int64 for ALL variance aggregations of the query: slot 0 the doc count, then per distinct argument
//                column (at most PG_VAR_MAX_COLS; VAR_POP(x), STDDEV_SAMP(x) share one) the exact power sums of pg_moments.h.  pg_var_reg
//                without GROUP BY, pg_var_lds up to PG_VAR_LDS_SLOTS slots, pg_var_hbm up to Knobs::var_hbm_max_bytes; beyond that the
//                query is refused.
//   the kernels' arguments (PgVarArgs; the kernels are those of pg_kernels_var.hip)
//   the tuples   the host forms (count, sum, m2) of every admitted group from its gathered row, each of the two doubles rounded once.
// The ordinary part is the query without its variance aggregations (a PERCENTILE among the others takes its own side pass from there); an
// ORDER BY that names a variance aggregation leaves the segment untrimmed.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <set>
#include <string>

#include "pg_internal.hpp"
#include "pg_fixed_point.h"
#include "pg_moments.h"

void pg_var_launch_pass(const PgVarArgs* args, int tier, int grid, hipStream_t stream);

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
  SideTable table;
  std::vector<VarColumn> cols;
};

VarPlan var_plan(Segment& seg, const pg_query& q) {
  side_query_check(q, kSubject);
  const bool null_handling = (q.flags & PG_QUERY_FLAG_NULL_HANDLING) != 0;
  VarPlan P;
  int32_t slots = 1;   // slot 0: the doc count
  std::set<std::string> read;
  std::lock_guard<std::mutex> lock(seg.mu);   // virtual dictionaries are built under the segment's lock
  for (int a = 0; a < q.n_aggregations; a++) {
    const pg_agg_spec& s = q.aggregations[a];
    side_columns_read(s, read);
    if (!is_variance_agg(s)) continue;
    const char* fn = agg_function_text(s.function);
    if (!s.column || strcmp(s.column, "*") == 0) fail(PG_ERR_INVALID_ARGUMENT, "%s needs a column", fn);
    Column* c = side_value_column(seg, s.column, fn, null_handling);
    size_t k = 0;
    while (k < P.cols.size() && P.cols[k].col != c) k++;
    if (k == P.cols.size()) {
      if (k >= PG_VAR_MAX_COLS) fail(PG_ERR_UNSUPPORTED, "variance aggregations over more than %d distinct columns in one query", PG_VAR_MAX_COLS);
      VarColumn vc;
      vc.col = c;
      vc.is_int = c->val_type == PG_V_I32;
      vc.exp = c->val_type == PG_V_I64 ? PG_VAR_LONG_EXP : c->fx_exp;
      vc.first_slot = slots;
      slots += vc.is_int ? PG_VAR_INT_SLOTS : PG_VAR_DBL_SLOTS;
      P.cols.push_back(vc);
    }
    P.cols[k].aggs.push_back(a);
  }
  P.table = side_table_plan(seg, q, kSubject, kWho, read, slots, PG_VAR_LDS_SLOTS, 8, knobs().var_hbm_max_bytes, "variance aggregations", "PG_VAR_HBM_MAX_BYTES");
  return P;
}

}  // namespace

bool is_variance_agg(const pg_agg_spec& s) { return is_variance_function(s.function); }
void variance_plan_check(Segment& seg, const pg_query& q) { (void)var_plan(seg, q); }

std::unique_ptr<Result> execute_variance(Segment& seg, const pg_query& q, const CancelToken* cancel) {
  SumTablePass pass(seg, q, kWho, cancel);
  const VarPlan P = var_plan(seg, q);
  PgVarArgs A;
  int64_t doc_bits = pass.begin(P.table, A);
  A.n_cols = (int32_t)P.cols.size();
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
  pass.accumulate([&](int tier, int grid, hipStream_t stream) { pg_var_launch_pass(&A, tier, grid, stream); }, 1, 0);
  // ---- the tuples: (count, sum, m2), each of the two doubles rounded once; (0, 0.0, 0.0) over no doc ----------------------------------------------
  const int32_t n_rows = pass.n_rows();
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
      const int64_t* row = pass.row(i);
      const int64_t* sx = row + vc.first_slot;
      const int64_t n = row[0];
      r.l[0][(size_t)i] = n;
      r.d[0][(size_t)i] = pg_limbs_to_double(sx, n_sx, q1);
      r.d[1][(size_t)i] = pg_var_m2(n, sx, n_sx, q1, sx + n_sx, n_sq, q2);
    }
    side_share_result(out, vc.aggs, std::move(r));
  }
  return pass.finish(out, kTierKernel[P.table.tier], doc_bits, MERGED_VARIANCE);
}

}  // namespace pg
