// Queries with an aggregation over an arithmetic expression — SUM / MIN / MAX / AVG / MINMAXRANGE whose pg_agg_spec.column is an expression
// text (pg_expr.h: add / sub / mult / div over single-value numeric columns and literals): a side pass joined to the ordinary plan by group
// key.  The pass is the sum-table pass of pg_exec_sidepass.hip (SumTablePass: the ordinary part, the filter's match words, the table, the
// timed accumulation and gather, the doc-count check, the join and the statistics); this file holds what is the path's own:
//   the bounds   a pass per (segment, expression text) over ALL docs (pg_expr_bounds): the largest finite |value| fixes the scale of the
//                exact fixed-point SUM (pg_fixed_point.h, L = 4 limbs, q = E - 127 with every |value| < 2^E); an expression that yields a
//                NaN / Inf anywhere in the segment is refused by pg_query_exec.  Cached in the segment (at most 256 texts, filled under its
//                lock; the pass itself runs outside it).
//   the plan     one table [G][slots] of int64 for ALL expressions of the query: per expression the SUM's limbs, the MIN, the MAX, as far
//                as an aggregation asks for them, and one doc count for AVG.  pg_expr_reg without GROUP BY, pg_expr_lds up to
//                Knobs::expr_lds_max_slots slots, pg_expr_hbm up to Knobs::expr_hbm_max_bytes; beyond that the query is refused.
//   the kernels' arguments (PgExprArgs; the kernels are those of pg_kernels_expr.hip) and the table's initial values: the MIN / MAX
//                identities (pg_expr_init)
//   the results  SUM, MIN, MAX, AVG's pair and MINMAXRANGE's pair from the gathered rows; the reference's defaults over no doc fall out of
//                the identities.
// An expression may hold CASEs: more steps of the same program — comparisons, logical operations, selects —, resolved against
// the operand columns' types by expr_resolve_operands (pg_plan.cpp) before the bounds pass; nothing else of the path knows of them.
// The ordinary part is the query without its expression aggregations (a PERCENTILE among the others takes its own side pass from there);
// an ORDER BY that names an expression aggregation leaves the segment untrimmed.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <set>
#include <string>

#include "pg_internal.hpp"
#include "pg_expr.h"
#include "pg_fixed_point.h"

void pg_expr_launch_bounds(const PgExprArgs* args, unsigned long long* out, int grid, hipStream_t stream);
void pg_expr_launch_init(const PgExprArgs* args, int grid, hipStream_t stream);
void pg_expr_launch_pass(const PgExprArgs* args, int tier, int grid, hipStream_t stream);

namespace pg {
namespace {

const char* kWho = "expression";
const char* kSubject = "an aggregation over an expression";
constexpr size_t kMaxCachedBounds = 256;   // Segment::expr_bounds entries per segment (some tens of bytes each)
const char* const kTierKernel[3] = {"pg_expr_reg", "pg_expr_lds", "pg_expr_hbm"};

struct ExprItem {
  std::string text;
  ExprProgram prog;
  std::vector<int> src;     // per operand column of the program: its index among the query's sources
  std::vector<int> aggs;    // the aggregations over it (indexes into the query's)
  int32_t acc = 0;          // PgExprAcc bits
  int32_t sum_slot = -1, min_slot = -1, max_slot = -1;
  bool bounds_known = false;
  Segment::ExprBounds bounds;
};
struct ExprPlan {
  SideTable table;
  std::vector<ExprItem> exprs;
  std::vector<Column*> srcs;    // the distinct operand columns of all expressions
  int32_t count_slot = -1;
};

void fill_src(PgValueSrc& S, const Column& c) { expr_fill_src(S, c); }

// the bounds pass of one expression over every doc of the segment (seg.mu NOT held: it only reads registered columns, which never change or
// go away while the segment lives; the device is current)
Segment::ExprBounds run_bounds(Segment& seg, const ExprItem& item, const std::vector<Column*>& cols) {
  Segment::ExprBounds b;
  if (seg.total_docs <= 0) return b;
  PgExprArgs A;
  memset(&A, 0, sizeof(A));
  A.scan.n_docs = seg.total_docs;
  A.scan.n_words = ((int64_t)seg.total_docs + 63) / 64;
  A.n_srcs = (int32_t)cols.size();
  A.n_exprs = 1;
  A.count_slot = -1;
  for (size_t i = 0; i < cols.size(); i++) fill_src(A.srcs[i], *cols[i]);
  A.exprs[0].first_step = 0;
  A.exprs[0].n_steps = item.prog.n_steps;
  for (int k = 0; k < item.prog.n_steps; k++) A.steps[k] = item.prog.steps[k];
  hipStream_t stream = thread_stream(seg.device);
  DeviceBuffer out(16);
  PG_HIP(hipMemsetAsync(out.ptr, 0, 16, stream));
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)device_cus(seg.device) * 8, ((int64_t)seg.total_docs + 255) / 256));
  pg_expr_launch_bounds(&A, out.as<unsigned long long>(), grid, stream);
  PG_HIP(hipGetLastError());
  unsigned long long h[2] = {0, 0};
  PG_HIP(hipMemcpyAsync(h, out.ptr, sizeof(h), hipMemcpyDeviceToHost, stream));
  PG_HIP(hipStreamSynchronize(stream));
  double mx;
  memcpy(&mx, &h[0], 8);
  if (mx > 0) {
    int e = 0;
    (void)std::frexp(mx, &e);   // mx = f * 2^e, f in [0.5, 1): every finite |value| < 2^e
    b.exp = e;
  }
  b.has_nonfinite = h[1] != 0;
  return b;
}

[[noreturn]] void refuse_nonfinite(const ExprItem& item) {
  fail(PG_ERR_UNSUPPORTED, "expression %s yields a NaN or an infinity in this segment (a division by zero, an overflow): the Java plan answers such a query", item.text.c_str());
}

ExprPlan expr_plan(Segment& seg, const pg_query& q, bool compute_bounds) {
  side_query_check(q, kSubject);
  const bool null_handling = (q.flags & PG_QUERY_FLAG_NULL_HANDLING) != 0;
  ExprPlan P;
  std::set<std::string> read;
  bool need_count = false;
  if (compute_bounds) use_device(seg.device);
  std::unique_lock<std::mutex> lock(seg.mu);   // virtual dictionaries and the bounds cache are filled under the segment's lock
  for (int a = 0; a < q.n_aggregations; a++) {
    const pg_agg_spec& s = q.aggregations[a];
    if (!is_expression_agg(s)) {
      side_columns_read(s, read);
      continue;
    }
    int32_t acc = 0;
    switch (s.function) {
      case PG_AGG_SUM: acc = PG_EXPR_ACC_SUM; break;
      case PG_AGG_MIN: acc = PG_EXPR_ACC_MIN; break;
      case PG_AGG_MAX: acc = PG_EXPR_ACC_MAX; break;
      case PG_AGG_AVG: acc = PG_EXPR_ACC_SUM; need_count = true; break;
      case PG_AGG_MINMAXRANGE: acc = PG_EXPR_ACC_MIN | PG_EXPR_ACC_MAX; break;
      default:
        fail(PG_ERR_UNSUPPORTED, "%s over an expression (%s): SUM, MIN, MAX, AVG and MINMAXRANGE take one on the GPU path", agg_function_text(s.function), s.column);
    }
    size_t k = 0;
    while (k < P.exprs.size() && P.exprs[k].text != s.column) k++;
    if (k == P.exprs.size()) {
      if (k >= PG_EXPR_MAX_EXPRS) fail(PG_ERR_UNSUPPORTED, "more than %d distinct expressions in the aggregations of one query", PG_EXPR_MAX_EXPRS);
      ExprItem item;
      item.text = s.column;
      std::string error;
      const int32_t st = expr_parse(s.column, item.prog, error);
      if (st != PG_OK) fail(st, "%s (in %s)", error.c_str(), item.text.size() > 200 ? (item.text.substr(0, 197) + "...").c_str() : item.text.c_str());
      const std::vector<Column*> cols = expr_resolve_operands(seg, item.prog, null_handling);   // the rules expression predicates share; a CASE typed (pg_plan.cpp)
      for (Column* c : cols) {
        read.insert(c->name);
        size_t j = 0;
        while (j < P.srcs.size() && P.srcs[j] != c) j++;
        if (j == P.srcs.size()) {
          if (j >= PG_EXPR_MAX_SRCS) fail(PG_ERR_UNSUPPORTED, "the expressions of one query over more than %d distinct columns", PG_EXPR_MAX_SRCS);
          P.srcs.push_back(c);
        }
        item.src.push_back((int)j);
      }
      auto cached = seg.expr_bounds.find(item.text);
      if (cached != seg.expr_bounds.end()) {
        item.bounds = cached->second;
        item.bounds_known = true;
      } else if (compute_bounds) {
        // the pass runs WITHOUT the segment's lock — a full-segment kernel must not stall the other planners of the segment; two threads
        // that meet on a new text both run it and find the same answer.  The cache is bounded: texts that differ only in a literal are
        // entries of their own, so at kMaxCachedBounds the map is emptied and fills again (a text then costs one more pass)
        lock.unlock();
        item.bounds = run_bounds(seg, item, cols);
        lock.lock();
        item.bounds_known = true;
        if (seg.expr_bounds.size() >= kMaxCachedBounds) seg.expr_bounds.clear();
        seg.expr_bounds.emplace(item.text, item.bounds);
      }
      if (item.bounds_known && item.bounds.has_nonfinite) refuse_nonfinite(item);
      P.exprs.push_back(std::move(item));
    }
    P.exprs[k].acc |= acc;
    P.exprs[k].aggs.push_back(a);
  }
  // the group's row: per expression the SUM's limbs, the MIN, the MAX, as far as an aggregation asks for them; one doc count for AVG
  int32_t slots = 0;
  for (ExprItem& item : P.exprs) {
    if (item.acc & PG_EXPR_ACC_SUM) { item.sum_slot = slots; slots += PG_EXPR_SUM_LIMBS; }
    if (item.acc & PG_EXPR_ACC_MIN) item.min_slot = slots++;
    if (item.acc & PG_EXPR_ACC_MAX) item.max_slot = slots++;
  }
  if (need_count) P.count_slot = slots++;
  const Knobs& K = knobs();
  P.table = side_table_plan(seg, q, kSubject, kWho, read, slots, (uint64_t)std::min<int64_t>(K.expr_lds_max_slots, PG_EXPR_LDS_SLOTS), 8, K.expr_hbm_max_bytes,
                            "aggregations over expressions", "PG_EXPR_HBM_MAX_BYTES");
  return P;
}

double order_key_to_double(int64_t k) {
  const int64_t b = k ^ ((k >> 63) & 0x7FFFFFFFFFFFFFFFLL);
  double d;
  memcpy(&d, &b, 8);
  return d;
}

}  // namespace

// (a HISTOGRAM's argument list holds parentheses of its own — arrayvalueconstructor(...) —: its path looks at the first argument itself; a
// MODE over an expression is refused by the counting path, in its own words)
bool is_expression_agg(const pg_agg_spec& s) { return s.function != PG_AGG_HISTOGRAM && s.function != PG_AGG_MODE && expr_is_expression(s.column); }
void expression_plan_check(Segment& seg, const pg_query& q) { (void)expr_plan(seg, q, false); }

std::unique_ptr<Result> execute_expression(Segment& seg, const pg_query& q, const CancelToken* cancel) {
  SumTablePass pass(seg, q, kWho, cancel);
  const ExprPlan P = expr_plan(seg, q, true);
  PgExprArgs A;
  int64_t doc_bits = pass.begin(P.table, A);
  A.n_srcs = (int32_t)P.srcs.size();
  A.n_exprs = (int32_t)P.exprs.size();
  A.count_slot = P.count_slot;
  for (size_t i = 0; i < P.srcs.size(); i++) {
    fill_src(A.srcs[i], *P.srcs[i]);
    doc_bits += value_src_bits(*P.srcs[i]);
  }
  int32_t n_steps = 0;
  for (size_t e = 0; e < P.exprs.size(); e++) {
    const ExprItem& item = P.exprs[e];
    PgExprDesc& X = A.exprs[e];
    X.first_step = n_steps;
    X.n_steps = item.prog.n_steps;
    X.acc = item.acc;
    X.q = item.bounds.exp - (32 * PG_EXPR_SUM_LIMBS - 1);
    X.sum_slot = item.sum_slot;
    X.min_slot = item.min_slot;
    X.max_slot = item.max_slot;
    for (int k = 0; k < item.prog.n_steps; k++) {
      pg_expr_step st = item.prog.steps[k];   // the program's column indexes -> the query's sources
      if (st.a >= 0 && st.a < PG_EXPR_MAX_SRCS) st.a = item.src[(size_t)st.a];
      if (st.b >= 0 && st.b < PG_EXPR_MAX_SRCS) st.b = item.src[(size_t)st.b];
      if (st.c >= 0 && st.c < PG_EXPR_MAX_SRCS) st.c = item.src[(size_t)st.c];
      A.steps[n_steps++] = st;
    }
    if (item.min_slot >= 0) A.ident[item.min_slot] = INT64_MAX;
    if (item.max_slot >= 0) A.ident[item.max_slot] = INT64_MIN;
  }
  pass.accumulate([&](int tier, int grid, hipStream_t stream) { pg_expr_launch_pass(&A, tier, grid, stream); }, 1, P.count_slot,
                  [&](int grid, hipStream_t stream) { pg_expr_launch_init(&A, grid, stream); });
  // ---- the expression aggregations' results: the reference's defaults over no doc fall out of the identities -----------------------------------
  const int32_t n_rows = pass.n_rows();
  std::vector<AggResult> out((size_t)q.n_aggregations);
  for (const ExprItem& item : P.exprs) {
    const int fx_q = item.bounds.exp - (32 * PG_EXPR_SUM_LIMBS - 1);
    auto sum_of = [&](int32_t i) { return pg_limbs_to_double(pass.row(i) + item.sum_slot, PG_EXPR_SUM_LIMBS, fx_q); };
    auto min_of = [&](int32_t i) {
      const int64_t k = pass.row(i)[item.min_slot];
      return k == INT64_MAX ? std::numeric_limits<double>::infinity() : order_key_to_double(k);   // MinAggregationFunction's default
    };
    auto max_of = [&](int32_t i) {
      const int64_t k = pass.row(i)[item.max_slot];
      return k == INT64_MIN ? -std::numeric_limits<double>::infinity() : order_key_to_double(k);
    };
    for (int a : item.aggs) {
      AggResult& r = out[(size_t)a];
      switch (q.aggregations[a].function) {
        case PG_AGG_SUM:
          r.kind = PG_RESULT_DOUBLE;
          r.d[0].resize((size_t)n_rows);
          for (int32_t i = 0; i < n_rows; i++) r.d[0][(size_t)i] = sum_of(i);
          break;
        case PG_AGG_MIN:
          r.kind = PG_RESULT_DOUBLE;
          r.d[0].resize((size_t)n_rows);
          for (int32_t i = 0; i < n_rows; i++) r.d[0][(size_t)i] = min_of(i);
          break;
        case PG_AGG_MAX:
          r.kind = PG_RESULT_DOUBLE;
          r.d[0].resize((size_t)n_rows);
          for (int32_t i = 0; i < n_rows; i++) r.d[0][(size_t)i] = max_of(i);
          break;
        case PG_AGG_AVG:
          r.kind = PG_RESULT_AVG_PAIR;
          r.d[0].resize((size_t)n_rows);
          r.l[0].resize((size_t)n_rows);
          for (int32_t i = 0; i < n_rows; i++) { r.d[0][(size_t)i] = sum_of(i); r.l[0][(size_t)i] = pass.row(i)[P.count_slot]; }
          break;
        default:   // PG_AGG_MINMAXRANGE
          r.kind = PG_RESULT_MINMAX_PAIR;
          r.d[0].resize((size_t)n_rows);
          r.d[1].resize((size_t)n_rows);
          for (int32_t i = 0; i < n_rows; i++) { r.d[0][(size_t)i] = min_of(i); r.d[1][(size_t)i] = max_of(i); }
          break;
      }
    }
  }
  return pass.finish(out, kTierKernel[P.table.tier], doc_bits, MERGED_EXPRESSION);
}

}  // namespace pg
