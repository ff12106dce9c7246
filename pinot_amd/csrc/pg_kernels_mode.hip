// MODE on the device: the selection over the counting pass of pg_kernels_percentile.hip.  ModeAggregationFunction keeps a map value -> count
// per group and returns the key of greatest count; the counting pass already holds that map — a row of C counters over the value-ordered
// ids (the dense tiers), or the row's (key, count) runs (the sort tier).  What is selected is the partial of pg_mode.h,
// (max_count, n_tied, lowest tied id, highest tied id), whose combine rule is associative and commutative: any split of a row into ranges,
// lanes or wavefronts gives the row's partial.
//   pg_mode_select       grid over (row, share): a wavefront walks share_ids consecutive ids of a row, four 64-id loads in flight, every lane
//                        folding the ids it sees, then a butterfly over the lanes; it also sums the row's n and non-zero counters, which the
//                        runs need.  With shares == 1 a wavefront takes a whole row (many narrow rows) and its record is final; else
//   pg_mode_finish       one wavefront per row combines the shares' records (few wide rows: without GROUP BY over a 10^6-value column one
//                        wavefront would walk C / 64 dependent steps alone — the latency chain DESIGN 4.5 (d) names).
//   pg_mode_sort_select  one wavefront per row over its runs, found by binary search for row x C as pg_pctl_sort_select does.
// The tied ids an AVG over more than two ties needs are compacted by pg_pctl_runs / pg_pctl_sort_runs under a per-row count threshold.
// Kernel names are stable (rocprofv3 kernel traces).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pg_internal.hpp"

#define DEVFN __device__ __forceinline__

namespace {

DEVFN pg_mode_partial wave_combine(pg_mode_partial p) {
  for (int off = 32; off > 0; off >>= 1) {
    pg_mode_partial o;
    o.max_count = (uint32_t)__shfl_xor((int)p.max_count, off);
    o.n_tied = (uint32_t)__shfl_xor((int)p.n_tied, off);
    o.lo = (uint32_t)__shfl_xor((int)p.lo, off);
    o.hi = (uint32_t)__shfl_xor((int)p.hi, off);
    p = pg_mode_combine(p, o);
  }
  return p;
}
DEVFN uint64_t wave_sum(uint64_t v) {
  for (int off = 32; off > 0; off >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, off);
  return v;
}
DEVFN void store_row(PgModeRow* out, uint64_t n, uint64_t nz, const pg_mode_partial& p) {
  PgModeRow r;
  r.n = n;
  r.nnz = (uint32_t)nz;
  r.pad = 0;
  r.p = p;
  *out = r;
}

constexpr int kLoads = 4;   // 64-id loads of a wavefront in flight

}  // namespace

extern "C" __global__ void __launch_bounds__(256) pg_mode_select(const PgModeSelectArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int waves = blockDim.x >> 6;
  const int64_t items = (int64_t)a.n_rows * a.shares;
  for (int64_t item = (int64_t)blockIdx.x * waves + wave; item < items; item += (int64_t)gridDim.x * waves) {
    const int64_t row = item / a.shares;
    const uint32_t share = (uint32_t)(item - row * a.shares);
    const uint32_t* r = a.table + (uint64_t)a.rows[row] * a.card;
    const uint64_t i0 = (uint64_t)share * a.share_ids;
    const uint64_t i1 = i0 + a.share_ids < (uint64_t)a.card ? i0 + a.share_ids : (uint64_t)a.card;   // (a share past the row's end is empty)
    pg_mode_partial p = pg_mode_identity();
    uint64_t n = 0, nz = 0;
    for (uint64_t base = i0; base < i1; base += 64 * kLoads) {
      uint32_t c[kLoads];
#pragma unroll
      for (int u = 0; u < kLoads; u++) {
        const uint64_t i = base + (uint64_t)u * 64 + lane;
        c[u] = i < i1 ? r[i] : 0u;
      }
#pragma unroll
      for (int u = 0; u < kLoads; u++) {
        n += c[u];
        nz += c[u] != 0;
        p = pg_mode_combine(p, pg_mode_of((uint32_t)(base + (uint64_t)u * 64 + lane), c[u]));
      }
    }
    p = wave_combine(p);
    n = wave_sum(n);
    nz = wave_sum(nz);
    if (lane == 0) store_row(a.out + item, n, nz, p);
  }
}

// One wavefront per row: the records of its shares combined
extern "C" __global__ void __launch_bounds__(256) pg_mode_finish(const PgModeRow* __restrict__ parts, int32_t n_rows, uint32_t shares, PgModeRow* __restrict__ out) {
  const uint32_t lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int waves = blockDim.x >> 6;
  for (int64_t row = (int64_t)blockIdx.x * waves + wave; row < n_rows; row += (int64_t)gridDim.x * waves) {
    const PgModeRow* s = parts + row * shares;
    pg_mode_partial p = pg_mode_identity();
    uint64_t n = 0, nz = 0;
    for (uint32_t i = lane; i < shares; i += 64) {
      const PgModeRow x = s[i];
      n += x.n;
      nz += x.nnz;
      p = pg_mode_combine(p, x.p);
    }
    p = wave_combine(p);
    n = wave_sum(n);
    nz = wave_sum(nz);
    if (lane == 0) store_row(out + row, n, nz, p);
  }
}

// One wavefront per admitted group: its runs are [lower_bound(g C), lower_bound((g + 1) C)) (every lane does the same search)
extern "C" __global__ void __launch_bounds__(256) pg_mode_sort_select(const PgModeSortSelectArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int waves = blockDim.x >> 6;
  for (int64_t row = (int64_t)blockIdx.x * waves + wave; row < a.n_rows; row += (int64_t)gridDim.x * waves) {
    const uint64_t k0 = (uint64_t)a.rows[row] * a.card, k1 = k0 + a.card;
    auto lower = [&](uint64_t key) {
      int64_t lo = 0, hi = a.n_runs;
      while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (a.run_keys[mid] < key) lo = mid + 1; else hi = mid;
      }
      return lo;
    };
    const int64_t first = lower(k0), end = lower(k1);
    pg_mode_partial p = pg_mode_identity();
    uint64_t n = 0;
    for (int64_t i = first + lane; i < end; i += 64) {
      const uint32_t c = a.run_counts[i];
      n += c;
      p = pg_mode_combine(p, pg_mode_of((uint32_t)(a.run_keys[i] - k0), c));
    }
    p = wave_combine(p);
    n = wave_sum(n);
    if (lane == 0) {
      store_row(a.out + row, n, (uint64_t)(end - first), p);
      a.first_run[row] = first;
    }
  }
}

// ---- launchers (pg_exec_percentile.hip) -----------------------------------------------------------------------------------------------------------
void pg_mode_launch_select(const PgModeSelectArgs* args, int grid, hipStream_t stream) {
  const PgModeSelectArgs a = *args;
  hipLaunchKernelGGL(pg_mode_select, dim3(grid), dim3(256), 0, stream, a);
}
void pg_mode_launch_finish(const PgModeRow* parts, int32_t n_rows, uint32_t shares, PgModeRow* out, int grid, hipStream_t stream) {
  hipLaunchKernelGGL(pg_mode_finish, dim3(grid), dim3(256), 0, stream, parts, n_rows, shares, out);
}
void pg_mode_launch_sort_select(const PgModeSortSelectArgs* args, int grid, hipStream_t stream) {
  const PgModeSortSelectArgs a = *args;
  hipLaunchKernelGGL(pg_mode_sort_select, dim3(grid), dim3(256), 0, stream, a);
}
