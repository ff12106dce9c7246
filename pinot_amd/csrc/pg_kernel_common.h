// Device helpers every query kernel is written in: address spaces, non-temporal loads, wavefront reductions and the two mask
// layouts of a wave tile.  PG_WAVES_PER_BLOCK, when a kernel file sets its own, is defined before this header (pg_device.h reads it).
#ifndef PG_KERNEL_COMMON_H
#define PG_KERNEL_COMMON_H

#include <hip/hip_runtime.h>

#include "pg_device.h"

#ifndef DEVFN
#define DEVFN __device__ __forceinline__
#endif

// Pointers that were themselves loaded from memory (plan leaves) have no address space the compiler can infer and would
// be accessed with flat_load; every column / index byte lives in HBM, so say so.
#define GAS __attribute__((address_space(1)))
template <typename T> DEVFN const GAS T* gptr(const void* p) { return (const GAS T*)p; }
// Plan descriptors (filter program, leaves) are written by the host before the launch and never by a kernel: reading
// them through the constant address space lets the compiler use scalar loads (s_load → SGPRs, hoistable out of the tile
// loop) instead of a chain of vector loads each waited for with vmcnt(0).
#define CAS __attribute__((address_space(4)))
template <typename T> DEVFN const CAS T* cptr(const T* p) { return (const CAS T*)p; }
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef u32x2 u32x2_a4 __attribute__((aligned(4)));   // dword-aligned pair (bit-packed windows)

// Column and posting bytes are streamed once per query: non-temporal loads (measured +5 points of HBM roofline on cfg 3).
template <typename T> DEVFN T ldnt(const GAS T* p) { return __builtin_nontemporal_load(p); }
DEVFN uint32_t bswap32(uint32_t x) { return __builtin_bswap32(x); }
DEVFN int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// OR across aligned groups of 8 lanes (two quads) with DPP row operations.
DEVFN uint32_t or_reduce8(uint32_t v) {
  v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true);    // quad_perm [1,0,3,2]
  v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, true);    // quad_perm [2,3,0,1]
  v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, true);   // row_half_mirror
  return v;
}

DEVFN uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
// fold of an int64 accumulator across the wavefront (fn: PgAccFn; COUNT / SUM add, MIN, MAX) — every lane gets the result
DEVFN int64_t wave_fold_i64(int64_t v, int fn) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t lo = __shfl_xor((uint32_t)v, off, 64), hi = __shfl_xor((uint32_t)((uint64_t)v >> 32), off, 64);
    const int64_t o = (int64_t)(((uint64_t)hi << 32) | (uint64_t)lo);
    v = fn == PG_ACC_MIN ? (o < v ? o : v) : (fn == PG_ACC_MAX ? (o > v ? o : v) : v + o);
  }
  return v;
}

// ---- mask layouts ---------------------------------------------------------------------------------------------------------
// linear: lane L holds docs 32L .. 32L+31 of the wave tile (bit i = doc 32L+i) — what bitmap containers deliver
// quad:   lane L holds quads k*64+L, k = 0..7 (bit 4k+i = doc 4(k*64+L)+i)    — what 16 B/lane column loads deliver
DEVFN uint32_t lin_to_quad(uint32_t w, int lane) {
  uint32_t out = 0;
  const uint32_t sh = (uint32_t)(lane & 7) * 4u;
  const int src0 = lane >> 3;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const uint32_t x = (uint32_t)__shfl((int)w, k * 8 + src0, 64);   // dword holding quads 8(k*8+src0) .. +7
    out |= ((x >> sh) & 0xFu) << (4 * k);
  }
  return out;
}
DEVFN uint32_t quad_to_lin(uint32_t m, int lane) {
  uint32_t out = 0;
  const uint32_t sh = (uint32_t)(lane & 7) * 4u;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    uint32_t x = ((m >> (4 * k)) & 0xFu) << sh;
    x = or_reduce8(x);                                                 // lanes 8g..8g+7 hold linear dword k*8+g
    const uint32_t z = (uint32_t)__shfl((int)x, (lane & 7) * 8, 64);
    if ((lane >> 3) == k) out = z;
  }
  return out;
}
DEVFN uint32_t valid_lin_mask(int32_t n_valid, int lane) {   // n_valid: docs of this wave tile below numDocs
  const int rem = n_valid - lane * 32;
  return rem >= 32 ? 0xFFFFFFFFu : (rem <= 0 ? 0u : ((1u << rem) - 1u));
}
DEVFN uint32_t valid_quad_mask(int32_t n_valid, int lane) {
  if (n_valid >= PG_WAVE_DOCS) return 0xFFFFFFFFu;
  uint32_t m = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const int nv = n_valid - 4 * (k * 64 + lane);
    const uint32_t nib = nv >= 4 ? 0xFu : (nv <= 0 ? 0u : ((1u << nv) - 1u));
    m |= nib << (4 * k);
  }
  return m;
}

#endif  // PG_KERNEL_COMMON_H
