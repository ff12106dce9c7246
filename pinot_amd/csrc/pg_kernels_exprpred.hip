// An arithmetic expression as a filter leaf — the reference's ExpressionFilterOperator (operator/filter/ExpressionFilterOperator.java,
// dociditerators/ExpressionScanDocIdIterator.java): WHERE add(a,b) > 10, WHERE div(a,b) BETWEEN 1 AND 2, and every column-to-column
// comparison (PredicateComparisonRewriter turns a > b into minus(a,b) > 0).
//   pg_expr_pred  one pass over ALL docs of the segment per leaf: the operand columns loaded as doubles (expr_load), the program run one rounded
//                 IEEE operation at a time (expr_eval, contraction off: pg_expr_device.h), the raw DOUBLE predicate applied, and the leaf's doc
//                 set written as match words — the layout PG_F_PUSH_WORDS reads (bit doc & 31 of dword doc >> 5).
// The predicates restate the reference's raw DOUBLE evaluators, not the raw-column scan kernels:
//   RANGE   v >= lo && v <= hi              (RangePredicateEvaluatorFactory.java:532; exclusive bounds moved by nextUp / nextDown on the host)
//   EQ / NOT_EQ   v == x / v != x           (EqualsPredicateEvaluatorFactory.java:336, NotEqualsPredicateEvaluatorFactory.java:298)
//   IN / NOT_IN   a DoubleOpenHashSet       (InPredicateEvaluatorFactory.java:360): membership by Double.doubleToLongBits — -0.0 is not in
//                 {0.0}, a NaN is in a set that holds NaN.  (in_set_f64 of the raw-column scans compares numerically; it stays as it is.)
// Shape: lane = doc; a wavefront takes kPredWords 64-doc words per iteration and issues the operand loads of all of them before the first
// program runs (the accumulation kernels of pg_kernels_expr.hip are a load -> evaluate -> load chain); one __ballot per 64 docs gives the
// word, lanes 0 .. kPredWords-1 store one word each with a plain vector store.  No atomics, no LDS, no scratch (the resource log of this
// file is checked by tests/test_gpu_expression_filters.py).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pg_internal.hpp"
#include "pg_expr_device.h"

#pragma clang fp contract(off)

namespace {

constexpr int kPredWords = PG_EXPR_PRED_WORDS;

// Double.doubleToLongBits: every NaN is the canonical one
PG_EXPR_DEVFN uint64_t pred_long_bits(double v) {
  return v != v ? 0x7FF8000000000000ULL : (uint64_t)__double_as_longlong(v);
}

PG_EXPR_DEVFN bool pred_apply(const PgExprPred& P, double v) {
  switch (P.kind) {   // wave-uniform
    case PG_XP_RANGE: return v >= P.lo && v <= P.hi;
    case PG_XP_EQ: return v == P.lo;
    case PG_XP_NOT_EQ: return v != P.lo;
    default: {
      const uint64_t b = pred_long_bits(v);
      bool in = false;
      for (int i = 0; i < P.n_set; i++) in = in || P.set[i] == b;   // (the set's words come through the scalar cache)
      return in == (P.kind == PG_XP_IN);
    }
  }
}

}  // namespace

extern "C" __global__ void __launch_bounds__(256) pg_expr_pred(const PgExprArgs a, const PgExprPred P) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int waves = blockDim.x >> 6;
  const int64_t n_docs = a.scan.n_docs;
  const int64_t stride = (int64_t)gridDim.x * waves * kPredWords;
  for (int64_t w0 = ((int64_t)blockIdx.x * waves + wave) * kPredWords; w0 < P.n_words; w0 += stride) {
    pg_d8 s[kPredWords];
#pragma unroll
    for (int u = 0; u < kPredWords; u++) s[u] = pg_d8{0, 0, 0, 0, 0, 0, 0, 0};
    // Every word's operands first, column by column: the loads of a column over the kPredWords words are independent and in flight
    // together.  Two columns per trip: unrolled whole, the eight columns' descriptors crowded the scalar registers until the compiler
    // spilled to scratch; in pairs they stay in kernel-argument memory.
#pragma unroll 2
    for (int i = 0; i < a.n_srcs; i++) {   // wave-uniform
      double v[kPredWords];
#pragma unroll
      for (int u = 0; u < kPredWords; u++) {
        const int64_t doc = (w0 + u) * 64 + lane;
        v[u] = doc < n_docs ? expr_load(a.srcs[i], (uint32_t)doc) : 0.0;
      }
#pragma unroll
      for (int u = 0; u < kPredWords; u++) s[u][i & 7] = v[u];
    }
    uint64_t mine = 0;
#pragma unroll
    for (int u = 0; u < kPredWords; u++) {
      const int64_t doc = (w0 + u) * 64 + lane;
      const double v = expr_eval(a, 0, s[u]);
      const uint64_t m = __ballot(doc < n_docs && pred_apply(P, v));   // docs at and beyond numDocs: clear
      if (lane == u) mine = m;
    }
    if (lane < kPredWords && w0 + lane < P.n_words) P.out[w0 + lane] = mine;
  }
}

// ---- launcher (pg_plan.cpp) --------------------------------------------------------------------------------------------------------------------
void pg_expr_launch_pred(const PgExprArgs* args, const PgExprPred* pred, int grid, hipStream_t stream) {
  const PgExprArgs a = *args;
  const PgExprPred p = *pred;
  hipLaunchKernelGGL(pg_expr_pred, dim3(grid), dim3(256), 0, stream, a, p);
}
