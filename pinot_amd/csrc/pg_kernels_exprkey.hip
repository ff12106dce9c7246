// An arithmetic expression as a group-by / DISTINCT key — the reference groups a transform's result through the no-dictionary key generators
// (NoDictionarySingleColumnGroupKeyGenerator / NoDictionaryMultiColumnGroupKeyGenerator over the transform's DOUBLE values, fastutil
// Double2Int maps comparing doubleToLongBits).  pg_vdict.hip restates those maps for stored raw columns as a virtual dictionary; this is the
// pass that feeds it from an expression instead of from a column:
//   pg_expr_keys  one pass over ALL docs of the segment per (segment, expression text): the operand columns loaded as doubles (expr_load), the
//                 program run one rounded IEEE operation at a time (expr_eval, contraction off: pg_expr_device.h), and the value's
//                 order-preserving 64-bit DOUBLE key (pg_vdict_key.h: NaN canonicalised, then the sign flip) written per doc.
// Shape: that of pg_expr_pred (pg_kernels_exprpred.hip) — lane = doc; a wavefront takes kKeyWords 64-doc words per iteration and issues the
// operand loads of all of them, column by column and two columns per trip, before the first program runs; a word's 64 keys go out as one
// coalesced 512-byte vector store.  No atomics, no LDS, no scratch (the resource log of this file is checked by
// tests/test_gpu_expression_keys.py).  Docs at and beyond numDocs are not written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pg_internal.hpp"
#include "pg_expr_device.h"
#include "pg_vdict_key.h"

#pragma clang fp contract(off)

namespace {
constexpr int kKeyWords = PG_EXPR_PRED_WORDS;
}  // namespace

extern "C" __global__ void __launch_bounds__(256) pg_expr_keys(const PgExprArgs a, uint64_t* __restrict__ keys) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int waves = blockDim.x >> 6;
  const int64_t n_docs = a.scan.n_docs, n_words = a.scan.n_words;
  const int64_t stride = (int64_t)gridDim.x * waves * kKeyWords;
  for (int64_t w0 = ((int64_t)blockIdx.x * waves + wave) * kKeyWords; w0 < n_words; w0 += stride) {
    pg_d8 s[kKeyWords];
#pragma unroll
    for (int u = 0; u < kKeyWords; u++) s[u] = pg_d8{0, 0, 0, 0, 0, 0, 0, 0};
    // every word's operands first, column by column; two columns per trip (unrolled whole, the eight columns' descriptors crowd the scalar
    // registers until the compiler spills them: DESIGN 4.7)
#pragma unroll 2
    for (int i = 0; i < a.n_srcs; i++) {   // wave-uniform
      double v[kKeyWords];
#pragma unroll
      for (int u = 0; u < kKeyWords; u++) {
        const int64_t doc = (w0 + u) * 64 + lane;
        v[u] = doc < n_docs ? expr_load(a.srcs[i], (uint32_t)doc) : 0.0;
      }
#pragma unroll
      for (int u = 0; u < kKeyWords; u++) s[u][i & 7] = v[u];
    }
#pragma unroll
    for (int u = 0; u < kKeyWords; u++) {
      const int64_t doc = (w0 + u) * 64 + lane;
      const double v = expr_eval(a, 0, s[u]);
      if (doc < n_docs) keys[doc] = pg_vdict_key_of_bits((uint64_t)__double_as_longlong(v), 3);
    }
  }
}

// ---- launcher (pg_vdict.hip) -------------------------------------------------------------------------------------------------------------------
void pg_expr_launch_keys(const PgExprArgs* args, uint64_t* keys, int grid, hipStream_t stream) {
  const PgExprArgs a = *args;
  hipLaunchKernelGGL(pg_expr_keys, dim3(grid), dim3(256), 0, stream, a, keys);
}
