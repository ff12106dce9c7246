// The device half of the slot-table side passes (pg_kernels_expr.hip, pg_kernels_var.hip, pg_kernels_covar.hip, pg_kernels_moment.hip,
// pg_kernels_hist.hip, pg_kernels_withtime.hip; the host half is the frame of pg_exec_sidepass.hip): the walk over the filter's match words, the reductions
// across a wavefront, the skeleton of the two tiers with a table and the launcher of the three tiers.  A family's kernels supply what is
// theirs as callables — what a matching doc adds to its group's row, a slot's initial value, how a touched slot is flushed; the families
// whose slots are int64 sums (the variance family, covariance, SKEWNESS / KURTOSIS, HISTOGRAM) share those two in side_sum_table_pass, the addition
// of a digit and the load of an INT column.  Everything here is inlined into the kernels, and what they compute per doc stays in their
// own translation unit (pg_kernels_expr.hip and pg_kernels_covar.hip keep contraction off for what they instantiate from here).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pg_internal.hpp"

#define PG_SIDE_DEVFN __device__ __forceinline__
#define PG_SIDE_INLINE __attribute__((always_inline))   // on the callables handed to the templates below: inlined as early as the templates are

constexpr int kWordsPerWave = 4;

// where a thread stands in its wavefront and workgroup
struct SideWave { int lane, wave, waves; };
static PG_SIDE_DEVFN SideWave side_wave() { return {(int)(threadIdx.x & 63), __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), (int)(blockDim.x >> 6)}; }

// f(doc) for every matching doc: a wavefront takes kWordsPerWave 64-doc words per iteration, lane = doc (no match words: every doc).  A
// plain tile loop, not a software pipeline.
template <typename F>
PG_SIDE_DEVFN void side_scan_walk(const PgGroupScan& scan, const SideWave& at, F&& f) {
  const int64_t stride = (int64_t)gridDim.x * at.waves * kWordsPerWave;
  for (int64_t w0 = ((int64_t)blockIdx.x * at.waves + at.wave) * kWordsPerWave; w0 < scan.n_words; w0 += stride) {
#pragma unroll 1
    for (int u = 0; u < kWordsPerWave; u++) {
      const int64_t w = w0 + u;
      if (w >= scan.n_words) break;
      const uint64_t m = pg_scan_match_word(scan, w);
      if (m == 0) continue;   // a word without a match costs one scalar load
      if ((m >> at.lane) & 1) f((uint32_t)(w * 64 + at.lane));
    }
  }
}
template <typename F>
PG_SIDE_DEVFN void side_scan_walk(const PgGroupScan& scan, F&& f) { side_scan_walk(scan, side_wave(), f); }

static PG_SIDE_DEVFN int64_t wave_sum_i64(int64_t v) {
  for (int off = 32; off > 0; off >>= 1) v += (int64_t)__shfl_xor((long long)v, off);
  return v;
}
static PG_SIDE_DEVFN int64_t wave_min_i64(int64_t v) {
  for (int off = 32; off > 0; off >>= 1) { const int64_t o = (int64_t)__shfl_xor((long long)v, off); v = o < v ? o : v; }
  return v;
}
static PG_SIDE_DEVFN int64_t wave_max_i64(int64_t v) {
  for (int off = 32; off > 0; off >>= 1) { const int64_t o = (int64_t)__shfl_xor((long long)v, off); v = o > v ? o : v; }
  return v;
}
static PG_SIDE_DEVFN unsigned long long wave_max_u64(unsigned long long v) {
  for (int off = 32; off > 0; off >>= 1) { const unsigned long long o = (unsigned long long)__shfl_xor((long long)v, off); v = o > v ? o : v; }
  return v;
}

// The tiers with a table of `n_slots` 64-bit slots.  LDS: the workgroup's copy is set to initial(i), update(copy, doc) runs for every
// matching doc, and flush(i, value) hands every slot of the copy to the caller, which adds the touched ones to `table`; else update(table,
// doc) works on the table in HBM.
template <bool LDS, typename T, typename Initial, typename Update, typename Flush>
PG_SIDE_DEVFN void side_table_pass(const PgGroupScan& scan, uint64_t n_slots, T* table, Initial&& initial, Update&& update, Flush&& flush) {
  extern __shared__ unsigned long long side_lds[];
  static_assert(sizeof(T) == 8, "64-bit slots");
  // read before the barriers (the compiler does not move it across them): read after them, pg_expr_lds, which sits at the SGPR limit, spills
  // past its spill registers into scratch
  const SideWave at = side_wave();
  if (LDS) {
    T* tab = reinterpret_cast<T*>(side_lds);
    for (uint32_t i = threadIdx.x; i < (uint32_t)n_slots; i += blockDim.x) tab[i] = initial(i);
    __syncthreads();
    side_scan_walk(scan, at, [&](uint32_t doc) PG_SIDE_INLINE { update(tab, doc); });
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < (uint32_t)n_slots; i += blockDim.x) flush(i, tab[i]);
  } else {
    side_scan_walk(scan, at, [&](uint32_t doc) PG_SIDE_INLINE { update(table, doc); });
  }
}

// ---- tables of int64 sums ----------------------------------------------------------------------------------------------------------------
// a digit added to its slot, in LDS or in HBM; zero digits are skipped
template <typename Ptr>
PG_SIDE_DEVFN void side_sum_add(Ptr slot, int64_t d) {
  if (d) atomicAdd(reinterpret_cast<unsigned long long*>(slot), (unsigned long long)d);
}

// an INT column's value: raw big-endian, or through its INT dictionary
static PG_SIDE_DEVFN int64_t side_load_int(const PgValueSrc& S, uint32_t doc) {
  if (S.col_kind == PG_COL_FIXED_BIT) return (int64_t)reinterpret_cast<const int32_t*>(S.dict)[pg_fixed_bit_id(S.data, S.bits, doc)];   // wave-uniform
  return (int64_t)(int32_t)__builtin_bswap32(reinterpret_cast<const uint32_t*>(S.data)[doc]);
}

// side_table_pass over sums: the workgroup's copy starts at zero and only its touched slots are added to `table`.  update(row0, doc):
// `row0` is the table's first slot — the workgroup's copy in LDS, or the table in HBM.
template <bool LDS, typename Update>
PG_SIDE_DEVFN void side_sum_table_pass(const PgGroupScan& scan, uint64_t n_slots, int64_t* table, Update&& update) {
  side_table_pass<LDS>(
      scan, n_slots, table, [](uint32_t) PG_SIDE_INLINE { return (int64_t)0; }, update,
      [&](uint32_t i, int64_t v) PG_SIDE_INLINE { side_sum_add(table + i, v); });
}

// the pass of one tier: the LDS tier's workgroup has 512 threads and a table of `lds_bytes` (at most `lds_max_bytes`), the others 256 threads
template <typename Args>
void side_launch_pass(void (*reg)(Args), void (*lds)(Args), void (*hbm)(Args), size_t lds_max_bytes, const Args& a, size_t lds_bytes, int tier, int grid,
                      hipStream_t stream) {
  if (tier == pg::TIER_LDS) {
    PG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(lds), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max_bytes));
    hipLaunchKernelGGL(lds, dim3(grid), dim3(512), lds_bytes, stream, a);
  } else if (tier == pg::TIER_HBM) {
    hipLaunchKernelGGL(hbm, dim3(grid), dim3(256), 0, stream, a);
  } else {
    hipLaunchKernelGGL(reg, dim3(grid), dim3(256), 0, stream, a);
  }
}
