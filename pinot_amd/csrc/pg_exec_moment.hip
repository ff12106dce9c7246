// Queries with a SKEWNESS / KURTOSIS aggregation (PG_AGG_SKEWNESS / PG_AGG_KURTOSIS): a side pass joined to the ordinary plan by group key.
// The pass is the sum-table pass of pg_exec_sidepass.hip (SumTablePass: the ordinary part, the filter's match words, the table, the timed
// accumulation and gather, the doc-count checks, the join and the statistics); this file holds what is the path's own:
//   the plan     one table [G][slots] of int64 for ALL of them: slot 0 the doc count, then per distinct argument column (at most
//                PG_MOMENT_MAX_COLS; SKEWNESS(x), KURTOSIS(x) share one) the exact power sums of pg_moment4.h.  pg_moment_reg without
//                GROUP BY, pg_moment_lds up to PG_MOMENT_LDS_SLOTS slots, pg_moment_hbm up to Knobs::moment_hbm_max_bytes; beyond that the
//                query is refused.
//   the kernels' arguments (PgMomentArgs; the kernels are those of pg_kernels_moment.hip)
//   the tuples   the host forms (n, m1, m2, m3, m4) of every admitted group from its gathered row, each of the four doubles rounded once.
// The ordinary part is the query without these aggregations (a variance aggregation or a PERCENTILE among the others takes its own side
// pass from there); an ORDER BY that names one of them leaves the segment untrimmed.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <set>
#include <string>

#include "pg_internal.hpp"
#include "pg_fixed_point.h"
#include "pg_moments.h"
#include "pg_moment4.h"

void pg_moment_launch_pass(const PgMomentArgs* args, int tier, int grid, hipStream_t stream);

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
  SideTable table;
  std::vector<MomentColumn> cols;
};

MomentPlan moment_plan(Segment& seg, const pg_query& q) {
  side_query_check(q, kSubject);
  const bool null_handling = (q.flags & PG_QUERY_FLAG_NULL_HANDLING) != 0;
  MomentPlan P;
  int32_t slots = 1;   // slot 0: the doc count
  std::set<std::string> read;
  std::lock_guard<std::mutex> lock(seg.mu);   // virtual dictionaries are built under the segment's lock
  for (int a = 0; a < q.n_aggregations; a++) {
    const pg_agg_spec& s = q.aggregations[a];
    if (!is_moment_agg(s)) {
      side_columns_read(s, read);
      continue;
    }
    const char* fn = agg_function_text(s.function);
    if (!s.column || strcmp(s.column, "*") == 0) fail(PG_ERR_INVALID_ARGUMENT, "%s needs a column", fn);
    Column* c = side_value_column(seg, s.column, fn, null_handling);
    read.insert(c->name);
    if ((c->val_type == PG_V_F32 || c->val_type == PG_V_F64) && pg_m4_overflows(c->fx_exp))
      fail(PG_ERR_UNSUPPORTED, "%s over %s: the column's bound 2^%d admits a fourth power that overflows a double: the Java plan answers such a query", fn,
           c->name.c_str(), c->fx_exp);
    size_t k = 0;
    while (k < P.cols.size() && P.cols[k].col != c) k++;
    if (k == P.cols.size()) {
      if (k >= PG_MOMENT_MAX_COLS) fail(PG_ERR_UNSUPPORTED, "SKEWNESS / KURTOSIS aggregations over more than %d distinct columns in one query", PG_MOMENT_MAX_COLS);
      MomentColumn mc;
      mc.col = c;
      mc.is_int = c->val_type == PG_V_I32;
      mc.exp = c->val_type == PG_V_I64 ? PG_VAR_LONG_EXP : c->fx_exp;
      mc.first_slot = slots;
      slots += mc.is_int ? PG_M4_INT_SLOTS : PG_M4_DBL_SLOTS;
      P.cols.push_back(mc);
    }
    P.cols[k].aggs.push_back(a);
  }
  P.table = side_table_plan(seg, q, kSubject, kWho, read, slots, PG_MOMENT_LDS_SLOTS, 8, knobs().moment_hbm_max_bytes, "SKEWNESS / KURTOSIS aggregations",
                            "PG_MOMENT_HBM_MAX_BYTES");
  return P;
}

}  // namespace

bool is_moment_agg(const pg_agg_spec& s) { return s.function == PG_AGG_SKEWNESS || s.function == PG_AGG_KURTOSIS; }
void moment_plan_check(Segment& seg, const pg_query& q) { (void)moment_plan(seg, q); }

std::unique_ptr<Result> execute_moment(Segment& seg, const pg_query& q, const CancelToken* cancel) {
  SumTablePass pass(seg, q, kWho, cancel);
  const MomentPlan P = moment_plan(seg, q);
  PgMomentArgs A;
  int64_t doc_bits = pass.begin(P.table, A);
  A.n_cols = (int32_t)P.cols.size();
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
  pass.accumulate([&](int tier, int grid, hipStream_t stream) { pg_moment_launch_pass(&A, tier, grid, stream); }, 1, 0);
  // ---- the tuples: (n, m1, m2, m3, m4), each of the four doubles rounded once; (0, NaN, NaN, NaN, NaN) over no doc ---------------------------------
  const int32_t n_rows = pass.n_rows();
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
      const int64_t* row = pass.row(i);
      const int64_t* s1 = row + mc.first_slot;
      const pg_m4_tuple t = pg_m4_tuple_of(row[0], s1, n1, q1, s1 + n1, n2, q2, s1 + n1 + n2, n3, q3, s1 + n1 + n2 + n3, n4, q4);
      r.l[0][(size_t)i] = t.n;
      r.d[0][(size_t)i] = t.m1;
      r.d[1][(size_t)i] = t.m2;
      r.d[2][(size_t)i] = t.m3;
      r.d[3][(size_t)i] = t.m4;
    }
    side_share_result(out, mc.aggs, std::move(r));
  }
  return pass.finish(out, kTierKernel[P.table.tier], doc_bits, MERGED_FOURTH_MOMENT);
}

}  // namespace pg
