// Selection queries on the device: SelectionOnlyOperator / SelectionOrderByOperator (core/operator/query/) over the filter's match bitmap.
//   pg_select_topk_lds  ORDER BY ... LIMIT k, k <= PG_SELECT_LDS_MAX_K (_dict / _i32 / _i64 / _f32 / _f64: one ORDER BY column of that kind):
//                       a persistent grid streams the match words and the ORDER BY columns.
//                       Every doc's ORDER BY values are folded into one 64-bit order-space key (the K smallest keys are the answer).  A
//                       wavefront compares its docs' keys with a threshold T held in a register; docs with key < T are appended (ballot /
//                       mbcnt) to the wavefront's candidate buffer in LDS.  A full buffer is sorted in place (bitonic, within the
//                       wavefront) and cut to its best K; the K-th key is then published with a 64-bit atomicMin on one word in HBM, which
//                       every wavefront re-reads (relaxed) every few iterations.  A threshold is published only by a buffer that keeps K
//                       candidates at or below it to the end, so rejecting key >= T drops at most rows tied at the cut (the reference's heap
//                       leaves which of them survive unspecified).  The common path (no candidate in a word) has no barrier and no atomic.
//                       Each wavefront finally writes its survivors at or below T; one radix sort of them gives the K rows in order.
//   pg_select_keys      the large-K tier: the (key, docId) pair of every matching doc (at offsets from the tiles' match counts), radix-sorted
//                       whole.
//   pg_select_gather    the output columns of the result rows at their docIds (dictIds, raw values, var-byte lengths), and
//   pg_select_gather_bytes  the var-byte values copied to their offsets: only the result rows leave HBM.
// Kernel names are stable (rocprofv3 kernel traces).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <rocprim/device/device_radix_sort.hpp>

#include "pg_device.h"

#define DEVFN __device__ __forceinline__

namespace {

// id of `doc` in a fixed-bit column (MSB-first big-endian 32-bit words; 1 <= bits <= 31); the second word is read only when the value straddles it
DEVFN uint32_t fixed_bit_at(const uint8_t* data, int bits, uint32_t doc) {
  const uint64_t bit0 = (uint64_t)doc * (uint32_t)bits;
  const uint32_t* w = reinterpret_cast<const uint32_t*>(data) + (bit0 >> 5);
  const uint32_t sh = (uint32_t)(bit0 & 31);
  uint64_t win = (uint64_t)__builtin_bswap32(w[0]) << 32;
  if (sh + (uint32_t)bits > 32) win |= __builtin_bswap32(w[1]);
  return (uint32_t)(win >> (64u - sh - (uint32_t)bits)) & ((1u << bits) - 1u);
}
DEVFN uint32_t be32_at(const uint8_t* data, uint32_t doc) { return __builtin_bswap32(reinterpret_cast<const uint32_t*>(data)[doc]); }
DEVFN uint64_t be64_at(const uint8_t* data, uint32_t doc) { return __builtin_bswap64(reinterpret_cast<const unsigned long long*>(data)[doc]); }

// the field of one ORDER BY column in order space: ascending unsigned order = the reference's compareTo order (dictIds; Integer / Long;
// Float.compare / Double.compare: -0.0 < 0.0, every NaN one value above +inf); DESC mirrors it
DEVFN uint64_t key_field(const PgSelectKeyCol& c, uint32_t doc) {
  switch (c.kind) {
    case PG_SK_DICT: {
      const uint32_t id = fixed_bit_at(c.data, c.bits, doc);
      return c.desc ? (uint64_t)((uint32_t)c.card - 1u - id) : (uint64_t)id;
    }
    case PG_SK_I32: {
      const uint32_t f = be32_at(c.data, doc) ^ 0x80000000u;
      return c.desc ? (uint64_t)(~f) : (uint64_t)f;
    }
    case PG_SK_I64: {
      const uint64_t f = be64_at(c.data, doc) ^ 0x8000000000000000ull;
      return c.desc ? ~f : f;
    }
    case PG_SK_F32: {
      uint32_t b = be32_at(c.data, doc);
      if ((b & 0x7FFFFFFFu) > 0x7F800000u) b = 0x7FC00000u;   // Float.floatToIntBits: one NaN
      const uint32_t f = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
      return c.desc ? (uint64_t)(~f) : (uint64_t)f;
    }
    default: {
      uint64_t b = be64_at(c.data, doc);
      if ((b & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull) b = 0x7FF8000000000000ull;   // Double.doubleToLongBits: one NaN
      const uint64_t f = (b & 0x8000000000000000ull) ? ~b : (b | 0x8000000000000000ull);
      return c.desc ? ~f : f;
    }
  }
}

// KIND >= 0: one ORDER BY column of that kind (the field is the key: no loop, no switch); -1: any columns
template <int KIND>
DEVFN uint64_t order_key(const PgSelectKeyArgs& a, uint32_t doc) {
  if (KIND >= 0) {
    PgSelectKeyCol c = a.cols[0];
    c.kind = KIND;
    return key_field(c, doc);
  }
  uint64_t key = 0;
  for (int j = 0; j < a.n_cols; j++) key |= key_field(a.cols[j], doc) << a.cols[j].shift;
  return key;
}

// the match word `w` (every doc below n_docs when there is no match bitmap)
DEVFN uint64_t match_word(const PgSelectKeyArgs& a, int64_t w) {
  if (a.match) return a.match[w];
  const int64_t left = a.n_docs - w * 64;
  return left >= 64 ? ~0ull : (left <= 0 ? 0ull : ((1ull << left) - 1ull));
}

DEVFN void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

constexpr uint32_t kNoDoc = 0xFFFFFFFFu;   // an empty slot: (~0, kNoDoc) sorts after every real pair (docIds are below 2^31)

// ascending bitonic sort of the wavefront's n (a power of two >= 64) pairs in LDS, by (key, docId)
DEVFN void wave_sort(unsigned long long* keys, uint32_t* docs, int n, int lane) {
  for (int k = 2; k <= n; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = lane; i < n; i += 64) {
        const int p = i ^ j;
        if (p > i) {
          const unsigned long long ka = keys[i], kb = keys[p];
          const uint32_t da = docs[i], db = docs[p];
          const bool b_less = kb < ka || (kb == ka && db < da);
          if (b_less == ((i & k) == 0)) {
            keys[i] = kb; keys[p] = ka;
            docs[i] = db; docs[p] = da;
          }
        }
      }
      wave_sync();
    }
  }
}

DEVFN unsigned long long load_threshold(const unsigned long long* t) { return __hip_atomic_load(t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

constexpr int kWordsPerWave = 4;
constexpr int kRefreshIters = 16;   // the published threshold is re-read every 16 iterations (16 x 256 docs per wavefront)

}  // namespace

// n_slots: LDS pairs per wavefront, a power of two >= 2 * max(64, next power of two >= k)
template <int KIND>
DEVFN void topk_body(const PgSelectKeyArgs& a, int n_slots) {
  extern __shared__ unsigned long long s_keys[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int waves = blockDim.x >> 6;
  unsigned long long* keys = s_keys + (size_t)wave * n_slots;
  uint32_t* docs = reinterpret_cast<uint32_t*>(s_keys + (size_t)waves * n_slots) + (size_t)wave * n_slots;
  for (int i = lane; i < n_slots; i += 64) { keys[i] = ~0ull; docs[i] = kNoDoc; }
  wave_sync();
  const int K = a.k;
  int count = 0;                         // pairs held (wavefront-uniform)
  unsigned long long T = load_threshold(a.threshold);
  // sort, keep the best K, publish the K-th key when K are held
  auto flush = [&]() {
    wave_sort(keys, docs, n_slots, lane);
    if (count > K) {
      for (int i = K + lane; i < n_slots; i += 64) { keys[i] = ~0ull; docs[i] = kNoDoc; }
      count = K;
      wave_sync();
    }
    if (count == K) {
      const unsigned long long t = keys[K - 1];
      if (t < T) {
        T = t;
        if (lane == 0) atomicMin(a.threshold, t);
      }
    }
  };
  const int64_t n_words = (a.n_docs + 63) / 64;
  const int64_t stride = (int64_t)gridDim.x * waves * kWordsPerWave;
  int iter = 0;
  for (int64_t w0 = ((int64_t)blockIdx.x * waves + wave) * kWordsPerWave; w0 < n_words; w0 += stride) {
    if (++iter == kRefreshIters) {
      iter = 0;
      const unsigned long long g = load_threshold(a.threshold);
      T = g < T ? g : T;
    }
    uint64_t m[kWordsPerWave];
#pragma unroll
    for (int u = 0; u < kWordsPerWave; u++) m[u] = w0 + u < n_words ? match_word(a, w0 + u) : 0;
    if ((m[0] | m[1] | m[2] | m[3]) == 0) continue;
    unsigned long long key[kWordsPerWave];
#pragma unroll
    for (int u = 0; u < kWordsPerWave; u++) key[u] = ((m[u] >> lane) & 1) ? order_key<KIND>(a, (uint32_t)((w0 + u) * 64 + lane)) : 0ull;
#pragma unroll
    for (int u = 0; u < kWordsPerWave; u++) {
      // T == ~0: nothing published yet, every key (~0 included) is a candidate
      const bool take = ((m[u] >> lane) & 1) && (key[u] < T || T == ~0ull);
      const uint64_t ballot = __ballot(take);
      if (ballot == 0) continue;
      const int n = __popcll(ballot);
      if (count + n > n_slots) flush();   // after a flush at most K <= n_slots / 2 pairs are held: 64 more fit
      if (take) {
        const int pos = count + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
        keys[pos] = key[u];
        docs[pos] = (uint32_t)((w0 + u) * 64 + lane);
      }
      count += n;
      wave_sync();
    }
  }
  flush();
  // the survivors: at or below the threshold as last published (its publisher holds K pairs at or below it)
  const unsigned long long g = load_threshold(a.threshold);
  T = g < T ? g : T;
  const int held = count < K ? count : K;
  int n_out = 0;
  for (int i = 0; i < held; i++) n_out += (keys[i] <= T || T == ~0ull) ? 1 : 0;   // keys are ascending: a prefix survives
  if (n_out == 0) return;
  uint32_t base = 0;
  if (lane == 0) base = atomicAdd(a.out_count, (uint32_t)n_out);
  base = __shfl(base, 0);
  for (int i = lane; i < n_out; i += 64) {
    a.out_keys[base + i] = keys[i];
    a.out_docs[base + i] = docs[i];
  }
}

// the generic kernel, and one per kind of a lone ORDER BY column (the common case: its field is the key)
extern "C" __global__ void __launch_bounds__(256) pg_select_topk_lds(const PgSelectKeyArgs a, int n_slots) { topk_body<-1>(a, n_slots); }
extern "C" __global__ void __launch_bounds__(256) pg_select_topk_lds_dict(const PgSelectKeyArgs a, int n_slots) { topk_body<PG_SK_DICT>(a, n_slots); }
extern "C" __global__ void __launch_bounds__(256) pg_select_topk_lds_i32(const PgSelectKeyArgs a, int n_slots) { topk_body<PG_SK_I32>(a, n_slots); }
extern "C" __global__ void __launch_bounds__(256) pg_select_topk_lds_i64(const PgSelectKeyArgs a, int n_slots) { topk_body<PG_SK_I64>(a, n_slots); }
extern "C" __global__ void __launch_bounds__(256) pg_select_topk_lds_f32(const PgSelectKeyArgs a, int n_slots) { topk_body<PG_SK_F32>(a, n_slots); }
extern "C" __global__ void __launch_bounds__(256) pg_select_topk_lds_f64(const PgSelectKeyArgs a, int n_slots) { topk_body<PG_SK_F64>(a, n_slots); }

// every matching doc's (key, docId), in docId order: one 16 384-doc tile per iteration of a workgroup, the tile's first pair at
// tile_offsets[tile] (exclusive prefix of the tiles' match counts), a word's first pair after the words before it (a scan over the tile's
// 256 words); each wavefront then writes 64 words, one doc per lane — coalesced, no atomic
extern "C" __global__ void __launch_bounds__(256) pg_select_keys(const PgSelectKeyArgs a, const int64_t* __restrict__ tile_offsets, int n_tiles) {
  __shared__ uint32_t s_scan[PG_TILE_WORDS];
  __shared__ uint64_t s_words[PG_TILE_WORDS];
  const int t = threadIdx.x;
  const int lane = t & 63;
  const int wave = t >> 6;
  const int64_t n_words = (a.n_docs + 63) / 64;
  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t w = (int64_t)tile * PG_TILE_WORDS + t;
    const uint64_t m = w < n_words ? match_word(a, w) : 0ull;
    const uint32_t c = (uint32_t)__popcll(m);
    s_words[t] = m;
    s_scan[t] = c;
    __syncthreads();
    for (int off = 1; off < PG_TILE_WORDS; off <<= 1) {   // inclusive scan of the words' counts
      const uint32_t v = t >= off ? s_scan[t - off] : 0u;
      __syncthreads();
      s_scan[t] += v;
      __syncthreads();
    }
    for (int i = 0; i < 64; i++) {
      const int wi = wave * 64 + i;
      const uint64_t mw = s_words[wi];
      if (mw == 0) continue;
      const int64_t base = tile_offsets[tile] + (int64_t)(s_scan[wi] - (uint32_t)__popcll(mw));
      if ((mw >> lane) & 1) {
        const uint32_t doc = (uint32_t)(((int64_t)tile * PG_TILE_WORDS + wi) * 64 + lane);
        const int64_t pos = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(mw >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mw, 0u));
        a.out_keys[pos] = order_key<-1>(a, doc);
        a.out_docs[pos] = doc;
      }
    }
    __syncthreads();
  }
}

// row i, column j -> out[j * n + i]: dictId, INT / LONG value, FLOAT / DOUBLE as IEEE double bits, or a var-byte value's length
extern "C" __global__ void __launch_bounds__(256) pg_select_gather(const PgSelectOutCol* __restrict__ cols, int n_cols, const uint32_t* __restrict__ docs,
                                                                   int64_t n, int64_t* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const uint32_t d = docs[i];
    for (int j = 0; j < n_cols; j++) {
      const PgSelectOutCol c = cols[j];
      int64_t v;
      switch (c.kind) {
        case PG_SO_DICT: v = (int64_t)fixed_bit_at(c.data, c.bits, d); break;
        case PG_SO_I32: v = (int64_t)(int32_t)be32_at(c.data, d); break;
        case PG_SO_I64: v = (int64_t)be64_at(c.data, d); break;
        case PG_SO_F32: v = __double_as_longlong((double)__uint_as_float(be32_at(c.data, d))); break;
        case PG_SO_F64: v = (int64_t)be64_at(c.data, d); break;
        default: v = c.vb_offsets[d + 1] - c.vb_offsets[d]; break;
      }
      out[(int64_t)j * n + i] = v;
    }
  }
}

// a var-byte column's values of the rows, back to back at `off` (n + 1 offsets)
extern "C" __global__ void __launch_bounds__(256) pg_select_gather_bytes(const PgSelectOutCol c, const uint32_t* __restrict__ docs, int64_t n,
                                                                         const int64_t* __restrict__ off, uint8_t* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const uint32_t d = docs[i];
    const uint8_t* src = c.data + c.vb_offsets[d];
    const int64_t len = off[i + 1] - off[i];
    for (int64_t b = 0; b < len; b++) out[off[i] + b] = src[b];
  }
}

// ---- launchers (pg_exec.hip) -------------------------------------------------------------------------------------------------------------
extern "C" size_t pg_select_topk_lds_bytes(int n_slots) { return (size_t)4 * n_slots * (8 + 4); }
// up to 96 KiB of dynamic LDS (n_slots = 2 * PG_SELECT_LDS_MAX_K): opted in per device by use_device
extern "C" void pg_select_lds_opt_in() {
  for (void (*k)(const PgSelectKeyArgs, int) : {pg_select_topk_lds, pg_select_topk_lds_dict, pg_select_topk_lds_i32, pg_select_topk_lds_i64,
                                                pg_select_topk_lds_f32, pg_select_topk_lds_f64})
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)pg_select_topk_lds_bytes(2 * PG_SELECT_LDS_MAX_K));
}
extern "C" void pg_select_launch_topk(const PgSelectKeyArgs* args, int n_slots, int grid, hipStream_t stream) {
  const PgSelectKeyArgs a = *args;
  void (*kern)(const PgSelectKeyArgs, int) = pg_select_topk_lds;
  if (a.n_cols == 1) {
    switch (a.cols[0].kind) {
      case PG_SK_DICT: kern = pg_select_topk_lds_dict; break;
      case PG_SK_I32: kern = pg_select_topk_lds_i32; break;
      case PG_SK_I64: kern = pg_select_topk_lds_i64; break;
      case PG_SK_F32: kern = pg_select_topk_lds_f32; break;
      default: kern = pg_select_topk_lds_f64; break;
    }
  }
  hipLaunchKernelGGL(kern, dim3(grid), dim3(256), pg_select_topk_lds_bytes(n_slots), stream, a, n_slots);
}
extern "C" void pg_select_launch_keys(const PgSelectKeyArgs* args, const int64_t* tile_offsets, int n_tiles, int grid, hipStream_t stream) {
  const PgSelectKeyArgs a = *args;
  hipLaunchKernelGGL(pg_select_keys, dim3(grid), dim3(256), 0, stream, a, tile_offsets, n_tiles);
}
extern "C" void pg_select_launch_gather(const PgSelectOutCol* cols_dev, int n_cols, const uint32_t* docs, int64_t n, int64_t* out, int grid, hipStream_t stream) {
  hipLaunchKernelGGL(pg_select_gather, dim3(grid), dim3(256), 0, stream, cols_dev, n_cols, docs, n, out);
}
extern "C" void pg_select_launch_gather_bytes(const PgSelectOutCol* col, const uint32_t* docs, int64_t n, const int64_t* off, uint8_t* out, int grid,
                                              hipStream_t stream) {
  const PgSelectOutCol c = *col;
  hipLaunchKernelGGL(pg_select_gather_bytes, dim3(grid), dim3(256), 0, stream, c, docs, n, off, out);
}
// ascending radix sort of n (key, docId) pairs over the key's low end_bit bits; tmp == nullptr: *tmp_bytes gets the scratch size
extern "C" hipError_t pg_select_sort_pairs(void* tmp, size_t* tmp_bytes, const unsigned long long* keys_in, unsigned long long* keys_out,
                                           const uint32_t* docs_in, uint32_t* docs_out, size_t n, int end_bit, hipStream_t stream) {
  return rocprim::radix_sort_pairs(tmp, *tmp_bytes, keys_in, keys_out, docs_in, docs_out, n, 0u, (unsigned)end_bit, stream);
}
