// A time-bucket transform as a group-by / DISTINCT key — the reference groups timeConvert / toEpoch... / dateTimeConvert /
// dateTrunc through the no-dictionary key generators over the transform's LONG values (LONG_SV_NO_DICTIONARY_METADATA, Long2Int maps).
// pg_vdict.hip restates those maps for stored raw columns as a virtual dictionary; this is the pass that feeds it from a time function:
//   pg_time_keys  one pass over ALL docs of the segment per (segment, text): the value column loaded as a long (INT widened, as
//                 transformToLongValuesSV does), the normal form of pg_time_program.h evaluated (pg_time_eval, the function the stand-alone host
//                 test runs as well), and the value's order-preserving 64-bit LONG key (pg_vdict_key.h, kind 1) written per doc.
// Shape: that of pg_expr_keys (pg_kernels_exprkey.hip) — lane = doc; a wavefront takes kKeyWords 64-doc words per iteration and issues the
// loads of all of them before the first program runs; a word's 64 keys go out as one coalesced 512-byte vector store.  The program is
// wave-uniform (kernel arguments): its branches are scalar.  No division instruction runs per doc: every divisor of the query arrives as a
// multiply-high reciprocal, the calendar's are compile-time constants.  No atomics, no LDS, no scratch (the resource log of this file is
// checked by tests/test_gpu_time_keys.py).  Docs at and beyond numDocs are not written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pg_internal.hpp"
#include "pg_vdict_key.h"

namespace {
constexpr int kKeyWords = PG_EXPR_PRED_WORDS;

__device__ __forceinline__ int64_t time_load(const PgValueSrc& S, uint32_t doc) {
  if (S.col_kind == PG_COL_FIXED_BIT) {   // wave-uniform
    const uint32_t id = pg_fixed_bit_id(S.data, S.bits, doc);
    return S.val_type == PG_V_I32 ? (int64_t)reinterpret_cast<const int32_t*>(S.dict)[id] : (int64_t)reinterpret_cast<const long long*>(S.dict)[id];
  }
  if (S.col_kind == PG_COL_RAW32) return (int64_t)(int32_t)__builtin_bswap32(reinterpret_cast<const uint32_t*>(S.data)[doc]);
  return (int64_t)__builtin_bswap64(reinterpret_cast<const unsigned long long*>(S.data)[doc]);
}
}  // namespace

extern "C" __global__ void __launch_bounds__(256) pg_time_keys(const PgTimeKeyArgs a, uint64_t* __restrict__ keys) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int waves = blockDim.x >> 6;
  const int64_t n_docs = a.n_docs, n_words = a.n_words;
  const int64_t stride = (int64_t)gridDim.x * waves * kKeyWords;
  for (int64_t w0 = ((int64_t)blockIdx.x * waves + wave) * kKeyWords; w0 < n_words; w0 += stride) {
    int64_t x[kKeyWords];
#pragma unroll
    for (int u = 0; u < kKeyWords; u++) {
      const int64_t doc = (w0 + u) * 64 + lane;
      x[u] = doc < n_docs ? time_load(a.src, (uint32_t)doc) : 0;
    }
#pragma unroll
    for (int u = 0; u < kKeyWords; u++) {
      const int64_t doc = (w0 + u) * 64 + lane;
      const int64_t v = pg_time_eval(a.prog, x[u]);
      if (doc < n_docs) keys[doc] = pg_vdict_key_of_bits((uint64_t)v, 1);
    }
  }
}

// ---- launcher (pg_vdict.hip) -------------------------------------------------------------------------------------------------------------------
void pg_time_launch_keys(const PgTimeKeyArgs* args, uint64_t* keys, int grid, hipStream_t stream) {
  const PgTimeKeyArgs a = *args;
  hipLaunchKernelGGL(pg_time_keys, dim3(grid), dim3(256), 0, stream, a, keys);
}
