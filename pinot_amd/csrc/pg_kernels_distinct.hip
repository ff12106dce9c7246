// SELECT DISTINCT on the device: DistinctOperator (core/operator/query/DistinctOperator.java) over the filter's match bitmap.  Three stages:
//   1. the filter (the executor's filter kernels) leaves one match bit per doc;
//   2. a presence pass turns every matching doc into the mixed-radix key of its DISTINCT columns' ids and sets that key's bit: in a
//      bitmap per workgroup in LDS for key spaces up to PG_DISTINCT_LDS_MAX_KEYS (persistent workgroups, one flush of the non-zero words
//      each), in one HBM bitmap beyond that (every word is read before an atomicOr: most docs hit a key that is already set);
//   3. a select: popcounts per chunk, a scan, and the first `limit` set bits written as positions, decoded to per-column ids on the
//      device — only the result rows leave HBM.
// Under ORDER BY the key is built in order space (order-by columns most significant, DESC digits mirrored), so the first set bits ARE the
// answer.  Without ORDER BY the answer is the first `limit` tuples in docId order: the executor runs the presence pass over doc windows
// into a bitmap of NEW keys (keys absent from every earlier window), ranks them, takes each new key's smallest docId (pg_distinct_first)
// and marks that doc in a doc bitmap; the first `limit` marked docs, decoded from the forward indexes, are the tuples in first-occurrence
// order.  Kernel names are stable (rocprofv3 kernel traces).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pg_device.h"

#define DEVFN __device__ __forceinline__

namespace {

// id of `doc` in a fixed-bit column (MSB-first, big-endian 32-bit words; 1 <= bits <= 31).  The second word is read only when the value
// straddles it, so the last value of the stream never reads past it.
DEVFN uint32_t distinct_id_at(const PgDistinctCol& c, uint32_t doc) { return pg_fixed_bit_id_at(c, doc); }

DEVFN uint64_t distinct_key_of(const PgDistinctArgs& a, uint32_t doc) {
  uint64_t key = 0;
  for (int j = 0; j < a.n_cols; j++) {
    const PgDistinctCol& c = a.cols[j];
    uint32_t d = distinct_id_at(c, doc);
    if (c.desc) d = (uint32_t)c.card - 1u - d;
    key += (uint64_t)d * c.mult;
  }
  return key;
}

DEVFN uint32_t load_relaxed(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

enum { KEYS_LDS = 0, KEYS_HBM = 1, KEYS_FIRST = 2 };

// A wavefront takes kWordsPerWave consecutive 64-doc match words per iteration (lane = doc of each): the match words and then the column
// ids of all of them are loaded before any bit is set, so several words' loads are in flight; words without a match cost one scalar load.
constexpr int kWordsPerWave = 4;
template <int MODE>
DEVFN void distinct_keys_body(const PgDistinctArgs& a) {
  extern __shared__ uint32_t s_bits[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int waves = blockDim.x >> 6;
  if (MODE == KEYS_LDS) {
    for (int64_t i = threadIdx.x; i < a.key_words; i += blockDim.x) s_bits[i] = 0;
    __syncthreads();
  }
  const int64_t stride = (int64_t)gridDim.x * waves * kWordsPerWave;
  for (int64_t w0 = a.w_begin + ((int64_t)blockIdx.x * waves + wave) * kWordsPerWave; w0 < a.w_end; w0 += stride) {
    uint64_t m[kWordsPerWave];
#pragma unroll
    for (int u = 0; u < kWordsPerWave; u++) m[u] = w0 + u < a.w_end ? a.match[w0 + u] : 0;
    if ((m[0] | m[1] | m[2] | m[3]) == 0) continue;
    uint64_t key[kWordsPerWave];
#pragma unroll
    for (int u = 0; u < kWordsPerWave; u++) key[u] = ((m[u] >> lane) & 1) ? distinct_key_of(a, (uint32_t)((w0 + u) * 64 + lane)) : ~0ULL;
#pragma unroll
    for (int u = 0; u < kWordsPerWave; u++) {
      if (key[u] == ~0ULL) continue;
      const int64_t kw = (int64_t)(key[u] >> 5);
      if (kw >= a.key_words) continue;   // (cannot happen for ids below their cardinalities)
      const uint32_t bit = 1u << (key[u] & 31);
      if (MODE != KEYS_FIRST && a.seen && (a.seen[kw] & bit)) continue;
      if (MODE == KEYS_LDS) {
        if (!(s_bits[kw] & bit)) atomicOr(&s_bits[kw], bit);
      } else if (MODE == KEYS_HBM) {
        if (!(load_relaxed(a.keys + kw) & bit)) atomicOr(a.keys + kw, bit);
      } else {
        const uint32_t* nw = a.keys;
        if (!(nw[kw] & bit)) continue;
        const int64_t g0 = kw & ~(int64_t)(PG_DISTINCT_GROUP_WORDS - 1);
        uint32_t rank = a.group_rank[kw / PG_DISTINCT_GROUP_WORDS];
        for (int64_t i = g0; i < kw; i++) rank += __popc(nw[i]);
        rank += __popc(nw[kw] & (bit - 1u));
        atomicMin(a.first_doc + rank, (uint32_t)((w0 + u) * 64 + lane));
      }
    }
  }
  if (MODE == KEYS_LDS) {
    __syncthreads();
    for (int64_t i = threadIdx.x; i < a.key_words; i += blockDim.x) {
      const uint32_t v = s_bits[i];
      if (v && (load_relaxed(a.keys + i) & v) != v) atomicOr(a.keys + i, v);
    }
  }
}

// exclusive scan of one value per thread over a 256-thread workgroup
DEVFN uint32_t block_exclusive_scan(uint32_t v, uint32_t* s) {
  const int t = threadIdx.x;
  s[t] = v;
  for (int off = 1; off < 256; off <<= 1) {
    __syncthreads();
    const uint32_t x = t >= off ? s[t - off] : 0u;
    __syncthreads();
    s[t] += x;
  }
  __syncthreads();
  return s[t] - v;
}

constexpr int kWordsPerThread = PG_DISTINCT_CHUNK_WORDS / 256;

}  // namespace

extern "C" __global__ void __launch_bounds__(256) pg_distinct_keys_lds(const PgDistinctArgs a) { distinct_keys_body<KEYS_LDS>(a); }
extern "C" __global__ void __launch_bounds__(256) pg_distinct_keys_hbm(const PgDistinctArgs a) { distinct_keys_body<KEYS_HBM>(a); }
extern "C" __global__ void __launch_bounds__(256) pg_distinct_first(const PgDistinctArgs a) { distinct_keys_body<KEYS_FIRST>(a); }

// set bits per chunk of a bitmap padded to whole chunks
extern "C" __global__ void __launch_bounds__(256) pg_distinct_count(const uint32_t* __restrict__ bm, uint32_t* __restrict__ counts) {
  __shared__ uint32_t s[256];
  const uint32_t* w = bm + (int64_t)blockIdx.x * PG_DISTINCT_CHUNK_WORDS + threadIdx.x * kWordsPerThread;
  uint32_t n = 0;
  for (int i = 0; i < kWordsPerThread; i++) n += __popc(w[i]);
  const uint32_t before = block_exclusive_scan(n, s);
  if (threadIdx.x == 255) counts[blockIdx.x] = before + n;
}

// rank of every PG_DISTINCT_GROUP_WORDS-word group's first bit among all set bits (chunk_off: exclusive prefix of the chunk counts)
extern "C" __global__ void __launch_bounds__(256) pg_distinct_rank(const uint32_t* __restrict__ bm, const uint64_t* __restrict__ chunk_off,
                                                                   uint32_t* __restrict__ group_rank) {
  __shared__ uint32_t s[256];
  const int64_t w0 = (int64_t)blockIdx.x * PG_DISTINCT_CHUNK_WORDS + threadIdx.x * kWordsPerThread;
  uint32_t n = 0;
  for (int i = 0; i < kWordsPerThread; i++) n += __popc(bm[w0 + i]);
  uint32_t r = (uint32_t)chunk_off[blockIdx.x] + block_exclusive_scan(n, s);
  for (int g = 0; g < kWordsPerThread / PG_DISTINCT_GROUP_WORDS; g++) {
    group_rank[w0 / PG_DISTINCT_GROUP_WORDS + g] = r;
    for (int i = 0; i < PG_DISTINCT_GROUP_WORDS; i++) r += __popc(bm[w0 + g * PG_DISTINCT_GROUP_WORDS + i]);
  }
}

// positions of the first n_out set bits, ascending (chunks 0 .. gridDim.x - 1)
extern "C" __global__ void __launch_bounds__(256) pg_distinct_expand(const uint32_t* __restrict__ bm, const uint64_t* __restrict__ chunk_off,
                                                                     uint64_t n_out, uint32_t* __restrict__ out) {
  __shared__ uint32_t s[256];
  const int64_t w0 = (int64_t)blockIdx.x * PG_DISTINCT_CHUNK_WORDS + threadIdx.x * kWordsPerThread;
  uint32_t n = 0;
  for (int i = 0; i < kWordsPerThread; i++) n += __popc(bm[w0 + i]);
  uint64_t idx = chunk_off[blockIdx.x] + block_exclusive_scan(n, s);
  for (int i = 0; i < kWordsPerThread && idx < n_out; i++) {
    uint32_t v = bm[w0 + i];
    while (v && idx < n_out) {
      const int b = __builtin_ctz(v);
      v &= v - 1u;
      out[idx++] = (uint32_t)((uint64_t)(w0 + i) * 32u + (uint32_t)b);
    }
  }
}

// the first doc of every new key into the doc bitmap
extern "C" __global__ void __launch_bounds__(256) pg_distinct_mark(const uint32_t* __restrict__ first_doc, int64_t n, uint32_t* __restrict__ doc_bits) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const uint32_t d = first_doc[i];
    if (d == 0xFFFFFFFFu) continue;   // (every new key has a doc: the host checks the marks against the keys)
    atomicOr(doc_bits + (d >> 5), 1u << (d & 31));
  }
}

// seen |= fresh; fresh = 0 — in the chunks that hold a fresh key only
extern "C" __global__ void __launch_bounds__(256) pg_distinct_fold(uint32_t* __restrict__ seen, uint32_t* __restrict__ fresh, const uint32_t* __restrict__ counts) {
  if (counts[blockIdx.x] == 0) return;
  const int64_t w0 = (int64_t)blockIdx.x * PG_DISTINCT_CHUNK_WORDS;
  for (int i = threadIdx.x; i < PG_DISTINCT_CHUNK_WORDS; i += 256) {
    const uint32_t v = fresh[w0 + i];
    if (v) { seen[w0 + i] |= v; fresh[w0 + i] = 0; }
  }
}

// result rows: per column the ids, column-major [n_cols][n].  from_docs: pos are docIds (read from the forward indexes); else keys
extern "C" __global__ void __launch_bounds__(256) pg_distinct_decode(const PgDistinctArgs a, const uint32_t* __restrict__ pos, int64_t n, int from_docs,
                                                                     int32_t* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const uint32_t p = pos[i];
    for (int j = 0; j < a.n_cols; j++) {
      const PgDistinctCol& c = a.cols[j];
      uint32_t d;
      if (from_docs) {
        d = distinct_id_at(c, p);
      } else {
        d = (uint32_t)(((uint64_t)p / c.mult) % (uint64_t)c.card);
        if (c.desc) d = (uint32_t)c.card - 1u - d;
      }
      out[(int64_t)j * n + i] = (int32_t)d;
    }
  }
}

// ---- launchers (pg_exec.hip; pg_distinct_keys_lds takes up to 128 KiB of dynamic LDS: opted in per device by use_device) ---------------------------------------------------------------------------------------------------------
extern "C" void pg_distinct_launch_keys(const PgDistinctArgs* args, int mode, int grid, hipStream_t stream) {
  const PgDistinctArgs a = *args;
  if (mode == KEYS_LDS) hipLaunchKernelGGL(pg_distinct_keys_lds, dim3(grid), dim3(256), (size_t)a.key_words * 4, stream, a);
  else if (mode == KEYS_HBM) hipLaunchKernelGGL(pg_distinct_keys_hbm, dim3(grid), dim3(256), 0, stream, a);
  else hipLaunchKernelGGL(pg_distinct_first, dim3(grid), dim3(256), 0, stream, a);
}
extern "C" void pg_distinct_launch_count(const uint32_t* bm, int64_t n_chunks, uint32_t* counts, hipStream_t stream) {
  hipLaunchKernelGGL(pg_distinct_count, dim3((unsigned)n_chunks), dim3(256), 0, stream, bm, counts);
}
extern "C" void pg_distinct_launch_rank(const uint32_t* bm, int64_t n_chunks, const uint64_t* chunk_off, uint32_t* group_rank, hipStream_t stream) {
  hipLaunchKernelGGL(pg_distinct_rank, dim3((unsigned)n_chunks), dim3(256), 0, stream, bm, chunk_off, group_rank);
}
extern "C" void pg_distinct_launch_expand(const uint32_t* bm, int64_t n_chunks, const uint64_t* chunk_off, uint64_t n_out, uint32_t* out, hipStream_t stream) {
  hipLaunchKernelGGL(pg_distinct_expand, dim3((unsigned)n_chunks), dim3(256), 0, stream, bm, chunk_off, n_out, out);
}
extern "C" void pg_distinct_launch_mark(const uint32_t* first_doc, int64_t n, uint32_t* doc_bits, int grid, hipStream_t stream) {
  hipLaunchKernelGGL(pg_distinct_mark, dim3(grid), dim3(256), 0, stream, first_doc, n, doc_bits);
}
extern "C" void pg_distinct_launch_fold(uint32_t* seen, uint32_t* fresh, const uint32_t* counts, int64_t n_chunks, hipStream_t stream) {
  hipLaunchKernelGGL(pg_distinct_fold, dim3((unsigned)n_chunks), dim3(256), 0, stream, seen, fresh, counts);
}
extern "C" void pg_distinct_launch_decode(const PgDistinctArgs* args, const uint32_t* pos, int64_t n, int from_docs, int32_t* out, int grid, hipStream_t stream) {
  const PgDistinctArgs a = *args;
  hipLaunchKernelGGL(pg_distinct_decode, dim3(grid), dim3(256), 0, stream, a, pos, n, from_docs, out);
}
