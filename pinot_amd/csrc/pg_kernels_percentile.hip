// Exact PERCENTILE(col, p) on the device: PercentileAggregationFunction (core/query/aggregation/function/PercentileAggregationFunction.java)
// keeps every matching value per group in a DoubleArrayList, sorts it at the end and takes sorted[(int)((long) size * p / 100)].  The result
// is a pure function of the multiset of values per group, and both kinds of column here have a value-ordered id space (sorted dictionaries,
// the virtual dictionary of a raw column): the multiset is a row of counters over the ids.  Three stages:
//   1. a counting pass over the filter's match words: key = groupKey x C + valueId, one 32-bit counter per key — per workgroup in LDS for
//      tables of up to PG_PCTL_LDS_KEYS counters (pg_pctl_lds: persistent workgroups, ds_add_u32 per matching doc, one flush of the non-zero
//      counters), in HBM beyond that (pg_pctl_hbm: a wavefront first folds the docs of its 64 that share a key — low-cardinality columns make
//      runs of equal keys common — then one global atomic per distinct key);
//   2. rank selection (pg_pctl_select): one wavefront per admitted group scans its row of C counters — the total n, then per requested p a
//      wave-level prefix sum that stops at the first id whose cumulative count exceeds the rank;
//   3. for the intermediate form, the row's non-zero (valueId, count) runs written compacted (pg_pctl_runs): only they cross PCIe.
// Key spaces whose table would exceed the HBM budget take the sort tier instead of stage 1 and 2: pg_pctl_sort writes the 64-bit key of every
// matching doc compacted — at offsets from the tiles' match counts, no atomic — a rocprim radix sort runs over the key's significant bits, a
// run-length encode leaves (key, count) runs, and pg_pctl_sort_select does prefix sums' binary search per admitted group.
// Kernel names are stable (rocprofv3 kernel traces); the executor reports pg_pctl_lds / pg_pctl_hbm / pg_pctl_sort (pg_exec_percentile.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "pg_internal.hpp"

#define DEVFN __device__ __forceinline__

namespace {

constexpr uint32_t kNoKey = 0xFFFFFFFFu;   // n_keys < 2^32: never a key

// key = groupKey x C + valueId: the ids are per-doc gathers of one or two dwords (pg_fixed_bit_id_at, pg_device.h), as the DISTINCT path reads them
DEVFN uint64_t pctl_key64_of(const PgPctlArgs& a, uint32_t doc) { return pg_scan_group_key(a.scan, doc) * a.card + pg_fixed_bit_id_at(a.vcol, doc); }

DEVFN uint32_t pctl_key_of(const PgPctlArgs& a, uint32_t doc) {   // the dense tiers' key: below n_keys < 2^32
  const uint64_t key = pctl_key64_of(a, doc);
  return key < a.n_keys ? (uint32_t)key : kNoKey;   // (ids below their cardinalities always are)
}

// A wavefront takes kWordsPerWave consecutive 64-doc match words per iteration (lane = doc of each): the ids of all of them are loaded before
// any counter is touched, so several words' loads are in flight; words without a match cost one scalar load.
constexpr int kWordsPerWave = 4;
template <bool LDS>
DEVFN void pctl_count_body(const PgPctlArgs& a) {
  extern __shared__ uint32_t s_cnt[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int waves = blockDim.x >> 6;
  if (LDS) {
    for (uint32_t i = threadIdx.x; i < a.n_keys; i += blockDim.x) s_cnt[i] = 0;
    __syncthreads();
  }
  const int64_t stride = (int64_t)gridDim.x * waves * kWordsPerWave;
  for (int64_t w0 = ((int64_t)blockIdx.x * waves + wave) * kWordsPerWave; w0 < a.scan.n_words; w0 += stride) {
    uint64_t m[kWordsPerWave];
#pragma unroll
    for (int u = 0; u < kWordsPerWave; u++) {
      const int64_t w = w0 + u;
      m[u] = w < a.scan.n_words ? pg_scan_match_word(a.scan, w) : 0;
    }
    if ((m[0] | m[1] | m[2] | m[3]) == 0) continue;
    uint32_t key[kWordsPerWave];
#pragma unroll
    for (int u = 0; u < kWordsPerWave; u++) key[u] = ((m[u] >> lane) & 1) ? pctl_key_of(a, (uint32_t)((w0 + u) * 64 + lane)) : kNoKey;
#pragma unroll
    for (int u = 0; u < kWordsPerWave; u++) {
      if (m[u] == 0) continue;
      const uint32_t k = key[u];
      bool active = k != kNoKey;
      if (LDS) {
        if (active) atomicAdd(&s_cnt[k], 1u);
      } else {
        // fold the lanes that share a key: up to four distinct keys take one atomic each, whatever is left its own
        for (int round = 0; round < 4; round++) {
          const uint64_t act = __ballot(active);
          if (!act) break;
          const int leader = __ffsll((unsigned long long)act) - 1;
          const uint32_t k0 = (uint32_t)__shfl((int)k, leader);
          const bool same = active && k == k0;
          const uint64_t grp = __ballot(same);
          if (lane == leader) atomicAdd(a.table + k0, (uint32_t)__popcll(grp));
          if (same) active = false;
        }
        if (active) atomicAdd(a.table + k, 1u);
      }
    }
  }
  if (LDS) {
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < a.n_keys; i += blockDim.x) {
      const uint32_t v = s_cnt[i];
      if (v) atomicAdd(a.table + i, v);
    }
  }
}

DEVFN uint64_t wave_sum(uint64_t v) {
  for (int off = 32; off > 0; off >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, off);
  return v;
}

}  // namespace

extern "C" __global__ void __launch_bounds__(1024) pg_pctl_lds(const PgPctlArgs a) { pctl_count_body<true>(a); }
extern "C" __global__ void __launch_bounds__(256) pg_pctl_hbm(const PgPctlArgs a) { pctl_count_body<false>(a); }

// One wavefront per row: n and the non-zero counters of the row, then per p the smallest id whose cumulative count exceeds the rank
// (int)((double)n * p / 100) — the reference's two IEEE operations in its order — or n - 1 for p = 100.
extern "C" __global__ void __launch_bounds__(256) pg_pctl_select(const PgPctlSelectArgs a) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int waves = blockDim.x >> 6;
  for (int64_t row = (int64_t)blockIdx.x * waves + wave; row < a.n_rows; row += (int64_t)gridDim.x * waves) {
    const uint32_t* r = a.table + (uint64_t)a.rows[row] * a.card;
    uint64_t n = 0, nz = 0;
    for (uint32_t i = lane; i < a.card; i += 64) {
      const uint32_t c = r[i];
      n += c;
      nz += c != 0;
    }
    n = wave_sum(n);
    nz = wave_sum(nz);
    for (int k = 0; k < a.n_p; k++) {
      int32_t id = -1;
      if (n > 0) {
        const double p = a.p[k];
        const uint64_t rank = p == 100.0 ? n - 1 : (uint64_t)(int32_t)((double)(int64_t)n * p / 100.0);
        uint64_t base = 0;
        for (uint32_t i0 = 0; i0 < a.card; i0 += 64) {
          const uint32_t c = i0 + lane < a.card ? r[i0 + lane] : 0u;
          unsigned long long incl = c;
          for (int off = 1; off < 64; off <<= 1) {
            const unsigned long long t = __shfl_up(incl, off);
            if (lane >= off) incl += t;
          }
          const uint64_t hit = __ballot(base + incl > rank);
          if (hit) { id = (int32_t)(i0 + (uint32_t)__ffsll((unsigned long long)hit) - 1u); break; }
          base += __shfl(incl, 63);
        }
      }
      if (lane == 0) a.sel[row * a.n_p + k] = id;
    }
    if (lane == 0) { a.totals[row] = (int64_t)n; a.nnz[row] = (uint32_t)nz; }
  }
}

// One wavefront per row: its (id, count) runs whose count reaches the row's threshold, ascending, at offsets[row].  Without `min_counts` the
// threshold is 1 — the row's non-zero runs, PERCENTILE's and MODE's intermediate —; MODE passes a row's greatest count and gets its tied ids.
extern "C" __global__ void __launch_bounds__(256) pg_pctl_runs(const uint32_t* __restrict__ table, const uint32_t* __restrict__ rows, int32_t n_rows,
                                                               uint32_t card, const int64_t* __restrict__ offsets, const uint32_t* __restrict__ min_counts,
                                                               uint32_t* __restrict__ out_ids, uint32_t* __restrict__ out_counts) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int waves = blockDim.x >> 6;
  for (int64_t row = (int64_t)blockIdx.x * waves + wave; row < n_rows; row += (int64_t)gridDim.x * waves) {
    const uint32_t* r = table + (uint64_t)rows[row] * card;
    int64_t at = offsets[row];
    const int64_t end = offsets[row + 1];
    const uint32_t least = min_counts ? min_counts[row] : 1u;   // (never 0: a row without a counted id has no run)
    if (at == end) continue;
    for (uint32_t i0 = 0; i0 < card; i0 += 64) {
      const uint32_t c = i0 + lane < card ? r[i0 + lane] : 0u;
      const uint64_t nzm = __ballot(c >= least);
      const int64_t pos = at + __popcll(nzm & ((1ULL << lane) - 1ULL));
      if (c >= least && pos < end) { out_ids[pos] = i0 + lane; out_counts[pos] = c; }
      at += __popcll(nzm);
    }
  }
}

// ---- the sort tier -----------------------------------------------------------------------------------------------------------------------------------
// matches per 16 384-doc tile (one workgroup per tile, one match word per thread)
extern "C" __global__ void __launch_bounds__(PG_TILE_WORDS) pg_pctl_tile_counts(const PgPctlArgs a, int64_t* __restrict__ counts) {
  __shared__ uint32_t s[PG_TILE_WORDS];
  const int64_t w = (int64_t)blockIdx.x * PG_TILE_WORDS + threadIdx.x;
  s[threadIdx.x] = w < a.scan.n_words ? (uint32_t)__popcll(pg_scan_match_word(a.scan, w)) : 0u;
  __syncthreads();
  for (int off = PG_TILE_WORDS / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) s[threadIdx.x] += s[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) counts[blockIdx.x] = s[0];
}

// One workgroup per tile: an exclusive scan of the words' match counts gives every word its offset behind the tile's; a wavefront then
// writes the keys of a word's matching docs (lane = doc) at consecutive positions.  No atomic; keys come in docId order.
extern "C" __global__ void __launch_bounds__(PG_TILE_WORDS) pg_pctl_sort(const PgPctlArgs a, const int64_t* __restrict__ tile_offsets, int64_t n_out,
                                                                        uint64_t* __restrict__ keys) {
  __shared__ uint32_t s[PG_TILE_WORDS];
  const int t = threadIdx.x;
  const int64_t w_t = (int64_t)blockIdx.x * PG_TILE_WORDS + t;
  const uint32_t pc = w_t < a.scan.n_words ? (uint32_t)__popcll(pg_scan_match_word(a.scan, w_t)) : 0u;
  s[t] = pc;
  for (int off = 1; off < PG_TILE_WORDS; off <<= 1) {
    __syncthreads();
    const uint32_t x = t >= off ? s[t - off] : 0u;
    __syncthreads();
    s[t] += x;
  }
  __syncthreads();   // s[t]: inclusive
  const int lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int64_t base = tile_offsets[blockIdx.x];
  for (int i = wave; i < PG_TILE_WORDS; i += PG_TILE_WORDS / 64) {
    const int64_t w = (int64_t)blockIdx.x * PG_TILE_WORDS + i;
    if (w >= a.scan.n_words) break;
    const uint64_t m = pg_scan_match_word(a.scan, w);
    if (m == 0) continue;
    if ((m >> lane) & 1) {
      const int64_t pos = base + (i ? s[i - 1] : 0u) + __popcll(m & ((1ULL << lane) - 1ULL));
      if (pos < n_out) keys[pos] = pctl_key64_of(a, (uint32_t)(w * 64 + lane));
    }
  }
}

// One thread per admitted group: its runs are [lower_bound(g C), lower_bound((g + 1) C)); n from the cumulative counts, then per p the
// first run whose cumulative count exceeds the rank
extern "C" __global__ void __launch_bounds__(256) pg_pctl_sort_select(const PgPctlSortSelectArgs a) {
  const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= a.n_rows) return;
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
  const uint64_t before = first > 0 ? a.run_cum[first - 1] : 0;
  const uint64_t n = end > first ? a.run_cum[end - 1] - before : 0;
  a.totals[row] = (int64_t)n;
  a.nnz[row] = (uint32_t)(end - first);
  a.first_run[row] = first;
  for (int k = 0; k < a.n_p; k++) {
    int32_t id = -1;
    if (n > 0) {
      const double p = a.p[k];
      const uint64_t rank = p == 100.0 ? n - 1 : (uint64_t)(int32_t)((double)(int64_t)n * p / 100.0);
      int64_t lo = first, hi = end - 1;   // the first run with cum - before > rank (the last run always qualifies)
      while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (a.run_cum[mid] - before > rank) hi = mid; else lo = mid + 1;
      }
      id = (int32_t)(a.run_keys[lo] - k0);
    }
    a.sel[row * a.n_p + k] = id;
  }
}

// One wavefront per admitted group: its runs' (value id, count) at offsets[row] — all of them, or with `min_counts` (MODE's tied ids) those of
// its `n_runs[row]` runs whose count reaches the row's threshold, compacted
extern "C" __global__ void __launch_bounds__(256) pg_pctl_sort_runs(const uint64_t* __restrict__ run_keys, const uint32_t* __restrict__ run_counts,
                                                                    const uint32_t* __restrict__ rows, const int64_t* __restrict__ first_run, int32_t n_rows,
                                                                    uint32_t card, const int64_t* __restrict__ offsets, const uint32_t* __restrict__ min_counts,
                                                                    const uint32_t* __restrict__ n_runs, uint32_t* __restrict__ out_ids,
                                                                    uint32_t* __restrict__ out_counts) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int waves = blockDim.x >> 6;
  for (int64_t row = (int64_t)blockIdx.x * waves + wave; row < n_rows; row += (int64_t)gridDim.x * waves) {
    const int64_t at = offsets[row], n = offsets[row + 1] - at, src = first_run[row];
    const uint64_t k0 = (uint64_t)rows[row] * card;
    if (!min_counts) {
      for (int64_t i = lane; i < n; i += 64) {
        out_ids[at + i] = (uint32_t)(run_keys[src + i] - k0);
        out_counts[at + i] = run_counts[src + i];
      }
      continue;
    }
    if (n == 0) continue;
    const uint32_t least = min_counts[row];
    const int64_t in_row = n_runs[row];
    int64_t pos0 = at;
    for (int64_t i0 = 0; i0 < in_row; i0 += 64) {
      const uint32_t c = i0 + lane < in_row ? run_counts[src + i0 + lane] : 0u;
      const uint64_t hit = __ballot(c >= least);
      const int64_t pos = pos0 + __popcll(hit & ((1ULL << lane) - 1ULL));
      if (c >= least && pos < at + n) { out_ids[pos] = (uint32_t)(run_keys[src + i0 + lane] - k0); out_counts[pos] = c; }
      pos0 += __popcll(hit);
    }
  }
}

namespace {
struct CountToU64 {
  __host__ __device__ uint64_t operator()(uint32_t c) const { return (uint64_t)c; }
};
}  // namespace

namespace pg {
size_t pctl_sort_bytes(int64_t n_matches) {
  const size_t n = (size_t)std::max<int64_t>(n_matches, 1);
  size_t sort_tmp = 0, rle_tmp = 0, scan_tmp = 0;
  (void)rocprim::radix_sort_keys(nullptr, sort_tmp, (uint64_t*)nullptr, (uint64_t*)nullptr, n);
  (void)rocprim::run_length_encode(nullptr, rle_tmp, (uint64_t*)nullptr, (unsigned int)std::min<size_t>(n, 0x7FFFFFFF), (uint64_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr);
  (void)rocprim::inclusive_scan(nullptr, scan_tmp, (uint64_t*)nullptr, (uint64_t*)nullptr, n, rocprim::plus<uint64_t>());
  return n * (8 + 8 + 8 + 4 + 8) + std::max(sort_tmp, std::max(rle_tmp, scan_tmp)) + 4096;   // keys, sorted, run keys, run counts, cumulative counts
}

void pctl_sort_build(const PgPctlArgs& A, int64_t n_matches, int key_bits, hipStream_t stream, PctlSortRuns& out) {
  out.n_runs = 0;
  if (n_matches <= 0) return;
  const size_t n = (size_t)n_matches;
  const int64_t n_tiles = (A.scan.n_words + PG_TILE_WORDS - 1) / PG_TILE_WORDS;
  // offsets from the tiles' match counts
  DeviceBuffer counts((size_t)(n_tiles + 1) * 8), offsets((size_t)(n_tiles + 1) * 8);
  PG_HIP(hipMemsetAsync(counts.ptr, 0, (size_t)(n_tiles + 1) * 8, stream));
  hipLaunchKernelGGL(pg_pctl_tile_counts, dim3((unsigned)n_tiles), dim3(PG_TILE_WORDS), 0, stream, A, counts.as<int64_t>());
  PG_HIP(hipGetLastError());
  size_t tmp_bytes = 0;
  PG_HIP(rocprim::exclusive_scan(nullptr, tmp_bytes, counts.as<int64_t>(), offsets.as<int64_t>(), (int64_t)0, (size_t)n_tiles + 1, rocprim::plus<int64_t>(), stream));
  DeviceBuffer tmp(std::max<size_t>(tmp_bytes, 16));
  PG_HIP(rocprim::exclusive_scan(tmp.ptr, tmp_bytes, counts.as<int64_t>(), offsets.as<int64_t>(), (int64_t)0, (size_t)n_tiles + 1, rocprim::plus<int64_t>(), stream));
  int64_t total = 0;
  PG_HIP(hipMemcpyAsync(&total, offsets.as<int64_t>() + n_tiles, 8, hipMemcpyDeviceToHost, stream));
  PG_HIP(hipStreamSynchronize(stream));
  if (total != n_matches) fail(PG_ERR_INTERNAL, "PERCENTILE sort tier: %lld matches in the match words, the filter reported %lld", (long long)total, (long long)n_matches);
  DeviceBuffer keys(n * 8), sorted(n * 8);
  hipLaunchKernelGGL(pg_pctl_sort, dim3((unsigned)n_tiles), dim3(PG_TILE_WORDS), 0, stream, A, offsets.as<int64_t>(), n_matches, keys.as<uint64_t>());
  PG_HIP(hipGetLastError());
  const unsigned end_bit = (unsigned)std::max(1, std::min(64, key_bits));
  PG_HIP(rocprim::radix_sort_keys(nullptr, tmp_bytes, keys.as<uint64_t>(), sorted.as<uint64_t>(), n, 0u, end_bit, stream));
  if (tmp.size < tmp_bytes) { PG_HIP(hipStreamSynchronize(stream)); tmp.alloc(tmp_bytes); }
  PG_HIP(rocprim::radix_sort_keys(tmp.ptr, tmp_bytes, keys.as<uint64_t>(), sorted.as<uint64_t>(), n, 0u, end_bit, stream));
  // (key, count) runs; `keys` is free again and takes the distinct keys
  if (n > 0x7FFFFFFFull) fail(PG_ERR_UNSUPPORTED, "PERCENTILE sort tier over %zu matching docs", n);
  out.counts.alloc(n * 4);
  DeviceBuffer n_runs_dev(8, false);
  PG_HIP(hipMemsetAsync(n_runs_dev.ptr, 0, 8, stream));
  PG_HIP(rocprim::run_length_encode(nullptr, tmp_bytes, sorted.as<uint64_t>(), (unsigned int)n, keys.as<uint64_t>(), out.counts.as<uint32_t>(), n_runs_dev.as<uint32_t>(), stream));
  if (tmp.size < tmp_bytes) { PG_HIP(hipStreamSynchronize(stream)); tmp.alloc(tmp_bytes); }
  PG_HIP(rocprim::run_length_encode(tmp.ptr, tmp_bytes, sorted.as<uint64_t>(), (unsigned int)n, keys.as<uint64_t>(), out.counts.as<uint32_t>(), n_runs_dev.as<uint32_t>(), stream));
  uint32_t n_runs = 0;
  PG_HIP(hipMemcpyAsync(&n_runs, n_runs_dev.ptr, 4, hipMemcpyDeviceToHost, stream));
  PG_HIP(hipStreamSynchronize(stream));
  if (n_runs == 0 || (size_t)n_runs > n) fail(PG_ERR_INTERNAL, "PERCENTILE sort tier: %u runs of %zu keys", n_runs, n);
  // prefix sums over the runs
  out.cum.alloc((size_t)n_runs * 8);
  auto counts64 = rocprim::make_transform_iterator(out.counts.as<uint32_t>(), CountToU64());
  PG_HIP(rocprim::inclusive_scan(nullptr, tmp_bytes, counts64, out.cum.as<uint64_t>(), (size_t)n_runs, rocprim::plus<uint64_t>(), stream));
  if (tmp.size < tmp_bytes) { PG_HIP(hipStreamSynchronize(stream)); tmp.alloc(tmp_bytes); }
  PG_HIP(rocprim::inclusive_scan(tmp.ptr, tmp_bytes, counts64, out.cum.as<uint64_t>(), (size_t)n_runs, rocprim::plus<uint64_t>(), stream));
  PG_HIP(hipStreamSynchronize(stream));   // `sorted` and `tmp` go out of scope
  out.keys = std::move(keys);
  out.n_runs = n_runs;
}
}  // namespace pg

void pg_pctl_launch_sort_select(const PgPctlSortSelectArgs* args, hipStream_t stream) {
  const PgPctlSortSelectArgs a = *args;
  hipLaunchKernelGGL(pg_pctl_sort_select, dim3((unsigned)((a.n_rows + 255) / 256)), dim3(256), 0, stream, a);
}
void pg_pctl_launch_sort_runs(const uint64_t* run_keys, const uint32_t* run_counts, const uint32_t* rows, const int64_t* first_run, int32_t n_rows,
                              uint32_t card, const int64_t* offsets, const uint32_t* min_counts, const uint32_t* n_runs, uint32_t* out_ids, uint32_t* out_counts,
                              int grid, hipStream_t stream) {
  hipLaunchKernelGGL(pg_pctl_sort_runs, dim3(grid), dim3(256), 0, stream, run_keys, run_counts, rows, first_run, n_rows, card, offsets, min_counts, n_runs, out_ids, out_counts);
}

// ---- launchers (pg_exec_percentile.hip) -----------------------------------------------------------------------------------------------------------
void pg_pctl_launch_count(const PgPctlArgs* args, int lds, int grid, hipStream_t stream) {
  const PgPctlArgs a = *args;
  if (lds) {
    const size_t bytes = (size_t)a.n_keys * 4;
    PG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(pg_pctl_lds), hipFuncAttributeMaxDynamicSharedMemorySize, PG_PCTL_LDS_KEYS * 4));
    hipLaunchKernelGGL(pg_pctl_lds, dim3(grid), dim3(1024), bytes, stream, a);
  } else {
    hipLaunchKernelGGL(pg_pctl_hbm, dim3(grid), dim3(256), 0, stream, a);
  }
}
void pg_pctl_launch_select(const PgPctlSelectArgs* args, int grid, hipStream_t stream) {
  const PgPctlSelectArgs a = *args;
  hipLaunchKernelGGL(pg_pctl_select, dim3(grid), dim3(256), 0, stream, a);
}
void pg_pctl_launch_runs(const uint32_t* table, const uint32_t* rows, int32_t n_rows, uint32_t card, const int64_t* offsets, const uint32_t* min_counts,
                         uint32_t* out_ids, uint32_t* out_counts, int grid, hipStream_t stream) {
  hipLaunchKernelGGL(pg_pctl_runs, dim3(grid), dim3(256), 0, stream, table, rows, n_rows, card, offsets, min_counts, out_ids, out_counts);
}
