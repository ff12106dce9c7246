// Queries with a COVAR_POP / COVAR_SAMP aggregation (PG_AGG_COVARPOP, PG_AGG_COVARSAMP): a side pass joined to the ordinary plan by group
// key.  The pass is the sum-table pass of pg_exec_sidepass.hip (SumTablePass: the ordinary part, the filter's match words, the table, the
// timed accumulation and gather, the doc-count checks, the join and the statistics); this file holds what is the path's own:
//   the plan     the argument lists, and one table [G][slots] of int64 for ALL covariance aggregations of the query, filled by one fused
//                pass: slot 0 the doc count, then per distinct argument column (at most PG_COVAR_MAX_COLS) the digits of its sum, then per
//                distinct ordered pair (at most PG_COVAR_MAX_PAIRS; COVAR_POP(x,y), COVAR_SAMP(x,y) share one) the digits of the rounded
//                products (pg_covar.h).  pg_covar_reg without GROUP BY (pg_covar_reg_wide for more than one pair), pg_covar_lds up to
//                PG_COVAR_LDS_SLOTS slots, pg_covar_hbm up to Knobs::covar_hbm_max_bytes; beyond that the query is refused.
//   the kernels' arguments (PgCovarArgs; the kernels are those of pg_kernels_covar.hip) and the LDS tier's workgroups per CU
//   the tuples   the host forms (sumX, sumY, sumXY, count) of every admitted group from its gathered row, each of the three sums rounded once.
// The ordinary part is the query without its covariance aggregations (a variance or a PERCENTILE among the others takes its own side pass
// from there); an ORDER BY that names a covariance leaves the segment untrimmed.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <set>
#include <string>

#include "pg_internal.hpp"
#include "pg_expr.h"
#include "pg_fixed_point.h"
#include "pg_covar.h"

void pg_covar_launch_pass(const PgCovarArgs* args, int tier, int grid, hipStream_t stream);

namespace pg {
namespace {

const char* kWho = "covariance";
const char* kSubject = "a covariance aggregation";
const char* const kTierKernel[3] = {"pg_covar_reg", "pg_covar_lds", "pg_covar_hbm"};
const char* kWideRegKernel = "pg_covar_reg_wide";   // the register tier beyond PG_COVAR_REG_COLS / PG_COVAR_REG_PAIRS (pg_covar_launch_pass chooses alike)

// the argument list of pg_agg_spec.column: x, y (include/pinot_gpu.h: the general form of aggregations with more than one argument)
void parse_arguments(const pg_agg_spec& s, std::string& x, std::string& y) {
  const char* fn = agg_function_text(s.function);
  if (!s.column) fail(PG_ERR_INVALID_ARGUMENT, "%s needs its argument list: two columns", fn);
  std::vector<ExprArgument> args;
  std::string error;
  const int32_t st = expr_split_arguments(s.column, args, error);
  if (st != PG_OK) fail(st, "%s(%s): %s", fn, s.column, error.c_str());
  if (args.size() != 2) fail(PG_ERR_INVALID_ARGUMENT, "%s takes 2 arguments (two columns), %d given: %s", fn, (int)args.size(), s.column);
  for (int k = 0; k < 2; k++) {
    if (args[(size_t)k].quoted) fail(PG_ERR_INVALID_ARGUMENT, "%s: argument %d must be a column, not the literal '%s'", fn, k + 1, args[(size_t)k].text.c_str());
    if (expr_is_expression(args[(size_t)k].text.c_str())) fail(PG_ERR_UNSUPPORTED, "%s over an expression (%s): its arguments are columns on the GPU path", fn, args[(size_t)k].text.c_str());
  }
  x = args[0].text;
  y = args[1].text;
}

struct CovarColumn {
  Column* col = nullptr;
  bool is_int = false;      // one integer slot
  int exp = 0;              // every finite |value| < 2^exp
  int32_t first_slot = 0;
};
struct CovarPair {
  int x = 0, y = 0;         // indexes into the plan's columns
  int exp = 0;              // Ep: every |fl(x y)| < 2^exp
  int32_t first_slot = 0;
  std::vector<int> aggs;    // the covariance aggregations over it (indexes into the query's)
};
struct CovarPlan {
  SideTable table;
  std::vector<CovarColumn> cols;
  std::vector<CovarPair> pairs;
};

CovarPlan covar_plan(Segment& seg, const pg_query& q) {
  side_query_check(q, kSubject);
  const bool null_handling = (q.flags & PG_QUERY_FLAG_NULL_HANDLING) != 0;
  CovarPlan P;
  std::set<std::string> read;
  std::lock_guard<std::mutex> lock(seg.mu);   // virtual dictionaries are built under the segment's lock
  auto column_index = [&](const std::string& name, const char* fn) {
    Column* c = side_value_column(seg, name.c_str(), fn, null_handling);
    size_t k = 0;
    while (k < P.cols.size() && P.cols[k].col != c) k++;
    if (k == P.cols.size()) {
      if (k >= PG_COVAR_MAX_COLS) fail(PG_ERR_UNSUPPORTED, "covariance aggregations over more than %d distinct columns in one query", PG_COVAR_MAX_COLS);
      CovarColumn cc;
      cc.col = c;
      cc.is_int = c->val_type == PG_V_I32;
      cc.exp = cc.is_int ? PG_COVAR_INT_EXP : c->val_type == PG_V_I64 ? PG_VAR_LONG_EXP : c->fx_exp;
      P.cols.push_back(cc);
      read.insert(c->name);
    }
    return (int)k;
  };
  for (int a = 0; a < q.n_aggregations; a++) {
    const pg_agg_spec& s = q.aggregations[a];
    if (!is_covariance_agg(s)) {
      side_columns_read(s, read);
      continue;
    }
    const char* fn = agg_function_text(s.function);
    std::string xn, yn;
    parse_arguments(s, xn, yn);
    const int x = column_index(xn, fn), y = column_index(yn, fn);
    size_t k = 0;
    while (k < P.pairs.size() && !(P.pairs[k].x == x && P.pairs[k].y == y)) k++;
    if (k == P.pairs.size()) {
      if (k >= PG_COVAR_MAX_PAIRS) fail(PG_ERR_UNSUPPORTED, "covariance aggregations over more than %d distinct column pairs in one query", PG_COVAR_MAX_PAIRS);
      const int Ex = P.cols[(size_t)x].exp, Ey = P.cols[(size_t)y].exp;
      if (pg_covar_overflows(Ex, Ey))
        fail(PG_ERR_UNSUPPORTED, "%s(%s,%s): the columns' bounds 2^%d and 2^%d admit a product that overflows a double: the Java plan answers such a query", fn,
             P.cols[(size_t)x].col->name.c_str(), P.cols[(size_t)y].col->name.c_str(), Ex, Ey);
      CovarPair cp;
      cp.x = x;
      cp.y = y;
      cp.exp = pg_covar_prod_exp(Ex, Ey);
      P.pairs.push_back(cp);
    }
    P.pairs[k].aggs.push_back(a);
  }
  int32_t slots = 1;   // slot 0: the doc count
  for (CovarColumn& cc : P.cols) { cc.first_slot = slots; slots += pg_covar_col_slots(cc.is_int); }
  for (CovarPair& cp : P.pairs) { cp.first_slot = slots; slots += PG_COVAR_PROD_LIMBS; }
  P.table = side_table_plan(seg, q, kSubject, kWho, read, slots, PG_COVAR_LDS_SLOTS, 8, knobs().covar_hbm_max_bytes, "covariance aggregations", "PG_COVAR_HBM_MAX_BYTES");
  return P;
}

}  // namespace

bool is_covariance_agg(const pg_agg_spec& s) { return s.function == PG_AGG_COVARPOP || s.function == PG_AGG_COVARSAMP; }
void covariance_plan_check(Segment& seg, const pg_query& q) { (void)covar_plan(seg, q); }

std::unique_ptr<Result> execute_covariance(Segment& seg, const pg_query& q, const CancelToken* cancel) {
  SumTablePass pass(seg, q, kWho, cancel);
  const CovarPlan P = covar_plan(seg, q);
  PgCovarArgs A;
  int64_t doc_bits = pass.begin(P.table, A);
  A.n_cols = (int32_t)P.cols.size();
  A.n_pairs = (int32_t)P.pairs.size();
  for (size_t i = 0; i < P.cols.size(); i++) {
    const CovarColumn& cc = P.cols[i];
    PgCovarCol& C = A.cols[i];
    expr_fill_src(C.src, *cc.col);
    C.is_int = cc.is_int ? 1 : 0;
    C.first_slot = cc.first_slot;
    C.q1 = pg_var_q1(cc.exp);
    doc_bits += value_src_bits(*cc.col);   // every distinct column once
  }
  for (size_t i = 0; i < P.pairs.size(); i++) {
    const CovarPair& cp = P.pairs[i];
    PgCovarPair& C = A.pairs[i];
    C.x = cp.x;
    C.y = cp.y;
    C.first_slot = cp.first_slot;
    C.qp = pg_covar_qp(cp.exp);
  }
  // the LDS tier's workgroups are persistent: one per CU for a full table, up to four (32 waves) where the tables are small enough to
  // share the CU's LDS — the plain loop keeps one load per wave in flight, so the waves per CU decide how much of the bandwidth it
  // reaches (measured on the FIRSTWITHTIME / LASTWITHTIME pass)
  const int64_t lds_wgs = std::max<int64_t>(1, std::min<int64_t>(4, (int64_t)PG_COVAR_LDS_SLOTS / (int64_t)std::max<uint64_t>(1, P.table.n_slots)));
  pass.accumulate([&](int tier, int grid, hipStream_t stream) { pg_covar_launch_pass(&A, tier, grid, stream); }, lds_wgs, 0);
  // ---- the tuples: (sumX, sumY, sumXY, count), each of the three doubles rounded once; (0.0, 0.0, 0.0, 0) over no doc ------------------------------
  const int32_t n_rows = pass.n_rows();
  std::vector<AggResult> out((size_t)q.n_aggregations);
  for (const CovarPair& cp : P.pairs) {
    const CovarColumn& X = P.cols[(size_t)cp.x];
    const CovarColumn& Y = P.cols[(size_t)cp.y];
    AggResult r;
    r.kind = PG_RESULT_COVARIANCE_TUPLE;
    r.l[0].resize((size_t)n_rows);
    for (int k = 0; k < 3; k++) r.d[k].resize((size_t)n_rows);
    for (int32_t i = 0; i < n_rows; i++) {
      const int64_t* row = pass.row(i);
      const pg_covar_tuple t = pg_covar_tuple_of(row[0], row + X.first_slot, X.is_int, X.exp, row + Y.first_slot, Y.is_int, Y.exp, row + cp.first_slot, cp.exp);
      r.l[0][(size_t)i] = t.count;
      r.d[0][(size_t)i] = t.sum_x;
      r.d[1][(size_t)i] = t.sum_y;
      r.d[2][(size_t)i] = t.sum_xy;
    }
    side_share_result(out, cp.aggs, std::move(r));
  }
  const bool wide = P.table.tier == TIER_REG && ((int)P.cols.size() > PG_COVAR_REG_COLS || (int)P.pairs.size() > PG_COVAR_REG_PAIRS);
  return pass.finish(out, wide ? kWideRegKernel : kTierKernel[P.table.tier], doc_bits, MERGED_COVARIANCE);
}

}  // namespace pg
