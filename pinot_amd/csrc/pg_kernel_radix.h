// Keys and source values of the radix / hash partitioned group-by, per batch of quads and per doc.
#ifndef PG_KERNEL_RADIX_H
#define PG_KERNEL_RADIX_H

#include "pg_kernel_filter.h"

// raw keys of the 4 docs of B quads: Σ dictId_j · mult_j, one group column at a time (any width)
template <int B>
DEVFN void radix_keys_of(const PgQueryPlan& p, const uint32_t (&qi)[B], int wtile, uint32_t (&key)[B][4]) {
#pragma unroll
  for (int u = 0; u < B; u++)
#pragma unroll
    for (int i = 0; i < 4; i++) key[u][i] = 0;
  for (int g = 0; g < p.n_group_cols; g++) {
    const PgGroupCol& gc = p.gcols[g];
    const GAS uint32_t* tw = packed_wtile_base(gc.data, wtile, gc.bits);
    const uint32_t bits = (uint32_t)gc.bits, mask = (1u << gc.bits) - 1u, mult = (uint32_t)gc.mult;
    if (bits <= 8) {
      uint32_t r[B][2];
#pragma unroll
      for (int u = 0; u < B; u++) load_packed_quad<true>(tw, qi[u], bits, r[u]);
#pragma unroll
      for (int u = 0; u < B; u++) {
        uint32_t d[4];
        decode_packed_quad<true>(r[u], qi[u], bits, mask, d);
#pragma unroll
        for (int i = 0; i < 4; i++) key[u][i] += d[i] * mult;
      }
    } else {
      uint32_t r[B][8];
#pragma unroll
      for (int u = 0; u < B; u++) load_packed_quad<false>(tw, qi[u], bits, r[u]);
#pragma unroll
      for (int u = 0; u < B; u++) {
        uint32_t d[4];
        decode_packed_quad<false>(r[u], qi[u], bits, mask, d);
#pragma unroll
        for (int i = 0; i < 4; i++) key[u][i] += d[i] * mult;
      }
    }
  }
}

// 64-bit raw keys (PG_AGG_RADIX_HASH): Σ dictId_j · mult_j in int64
template <int B>
DEVFN void radix_keys_of64(const PgQueryPlan& p, const uint32_t (&qi)[B], int wtile, uint64_t (&key)[B][4]) {
#pragma unroll
  for (int u = 0; u < B; u++)
#pragma unroll
    for (int i = 0; i < 4; i++) key[u][i] = 0;
  for (int g = 0; g < p.n_group_cols; g++) {
    const PgGroupCol& gc = p.gcols[g];
    if (gc.col_kind != PG_COL_FIXED_BIT) {   // no-dictionary group column: key = value ^ 2^63
      if (gc.col_kind == PG_COL_RAW32) {
        const GAS uint8_t* tb = gptr<uint8_t>(gc.data + (size_t)wtile * (PG_WAVE_DOCS * 4));
#pragma unroll
        for (int u = 0; u < B; u++) {
          const u32x4 v = ldnt((const GAS u32x4*)(tb + qi[u] * 16u));
          key[u][0] = (uint64_t)(int64_t)(int32_t)bswap32(v.x) ^ (1ULL << 63); key[u][1] = (uint64_t)(int64_t)(int32_t)bswap32(v.y) ^ (1ULL << 63);
          key[u][2] = (uint64_t)(int64_t)(int32_t)bswap32(v.z) ^ (1ULL << 63); key[u][3] = (uint64_t)(int64_t)(int32_t)bswap32(v.w) ^ (1ULL << 63);
        }
      } else {
        const GAS uint8_t* tb = gptr<uint8_t>(gc.data + (size_t)wtile * (PG_WAVE_DOCS * 8));
#pragma unroll
        for (int u = 0; u < B; u++) {
          const GAS u32x4* pp = (const GAS u32x4*)(tb + qi[u] * 32u);
          const u32x4 a = ldnt(pp), b = ldnt(pp + 1);
          key[u][0] = ((((uint64_t)bswap32(a.x) << 32) | bswap32(a.y))) ^ (1ULL << 63); key[u][1] = ((((uint64_t)bswap32(a.z) << 32) | bswap32(a.w))) ^ (1ULL << 63);
          key[u][2] = ((((uint64_t)bswap32(b.x) << 32) | bswap32(b.y))) ^ (1ULL << 63); key[u][3] = ((((uint64_t)bswap32(b.z) << 32) | bswap32(b.w))) ^ (1ULL << 63);
        }
      }
      continue;
    }
    const GAS uint32_t* tw = packed_wtile_base(gc.data, wtile, gc.bits);
    const uint32_t bits = (uint32_t)gc.bits, mask = (1u << gc.bits) - 1u;
    const uint64_t mult = (uint64_t)gc.mult;
#pragma unroll
    for (int u = 0; u < B; u++) {
      uint32_t r[8], d[4];
      if (bits <= 8) { load_packed_quad<true>(tw, qi[u], bits, r); decode_packed_quad<true>(r, qi[u], bits, mask, d); }
      else { load_packed_quad<false>(tw, qi[u], bits, r); decode_packed_quad<false>(r, qi[u], bits, mask, d); }
#pragma unroll
      for (int i = 0; i < 4; i++) key[u][i] += (uint64_t)d[i] * mult;
    }
  }
}
DEVFN uint64_t radix_mix64(uint64_t x) {   // splitmix64 finaliser: bucket = low bits, LDS slot = bits 16..
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ULL;
  x ^= x >> 27; x *= 0x94D049BB133111EBULL;
  return x ^ (x >> 31);
}

// values of one source for the 4 docs of B quads, as the int64 the accumulators take (INT / LONG sign-extended, FLOAT / DOUBLE as
// the bits of the double) — raw 32/64-bit columns and dictionary-encoded ones
template <int B>
DEVFN void radix_source_values(const PgValueSrc& S, const uint32_t (&qi)[B], int wt, int64_t (&out)[B][4]) {
  if (S.col_kind == PG_COL_RAW32) {
    const GAS uint8_t* tb = gptr<uint8_t>(S.data + (size_t)wt * (PG_WAVE_DOCS * 4));
    u32x4 v[B];
#pragma unroll
    for (int u = 0; u < B; u++) v[u] = ldnt((const GAS u32x4*)(tb + qi[u] * 16u));
#pragma unroll
    for (int u = 0; u < B; u++) {
      const uint32_t x[4] = {bswap32(v[u].x), bswap32(v[u].y), bswap32(v[u].z), bswap32(v[u].w)};
#pragma unroll
      for (int i = 0; i < 4; i++)
        out[u][i] = S.val_type == PG_V_I32 ? (int64_t)(int32_t)x[i] : __double_as_longlong((double)__uint_as_float(x[i]));
    }
  } else if (S.col_kind == PG_COL_RAW64) {
    const GAS uint8_t* tb = gptr<uint8_t>(S.data + (size_t)wt * (PG_WAVE_DOCS * 8));
    u32x4 a[B], b[B];
#pragma unroll
    for (int u = 0; u < B; u++) {
      const GAS u32x4* pp = (const GAS u32x4*)(tb + qi[u] * 32u);
      a[u] = ldnt(pp);
      b[u] = ldnt(pp + 1);
    }
#pragma unroll
    for (int u = 0; u < B; u++) {
      out[u][0] = (int64_t)(((uint64_t)bswap32(a[u].x) << 32) | bswap32(a[u].y)); out[u][1] = (int64_t)(((uint64_t)bswap32(a[u].z) << 32) | bswap32(a[u].w));
      out[u][2] = (int64_t)(((uint64_t)bswap32(b[u].x) << 32) | bswap32(b[u].y)); out[u][3] = (int64_t)(((uint64_t)bswap32(b[u].z) << 32) | bswap32(b[u].w));
    }
  } else {   // dictionary-encoded: dictIds → values (every dictId read is a valid one: idle lanes re-read quad 0 of the tile)
    const GAS uint32_t* tw = packed_wtile_base(S.data, wt, S.bits);
    const uint32_t bits = (uint32_t)S.bits, mask = (1u << S.bits) - 1u;
#pragma unroll
    for (int u = 0; u < B; u++) {
      uint32_t r[8], d[4];
      if (bits <= 8) { load_packed_quad<true>(tw, qi[u], bits, r); decode_packed_quad<true>(r, qi[u], bits, mask, d); }
      else { load_packed_quad<false>(tw, qi[u], bits, r); decode_packed_quad<false>(r, qi[u], bits, mask, d); }
#pragma unroll
      for (int i = 0; i < 4; i++) {
        if (S.val_type == PG_V_I32) out[u][i] = (int64_t)(int32_t)gptr<uint32_t>(S.dict)[d[i]];
        else if (S.val_type == PG_V_F32) out[u][i] = __double_as_longlong((double)__uint_as_float(gptr<uint32_t>(S.dict)[d[i]]));
        else out[u][i] = (int64_t)gptr<uint64_t>(S.dict)[d[i]];
      }
    }
  }
}

// one value of a bit-packed column at in-tile doc index `doc` (any width)
DEVFN uint32_t packed_value_at(const GAS uint32_t* __restrict__ tw, uint32_t doc, uint32_t bits) {
  const uint32_t bit0 = doc * bits;
  const u32x2 v = *(const GAS u32x2_a4*)(tw + (bit0 >> 5));
  const uint64_t win = ((uint64_t)bswap32(v.x) << 32) | (uint64_t)bswap32(v.y);
  return (uint32_t)(win >> (64u - (bit0 & 31u) - bits)) & ((1u << bits) - 1u);
}
DEVFN int64_t source_value_at(const PgValueSrc& S, int wt, uint32_t doc) {
  if (S.col_kind == PG_COL_RAW32) {
    const uint32_t x = bswap32(gptr<uint32_t>(S.data + (size_t)wt * (PG_WAVE_DOCS * 4))[doc]);
    return S.val_type == PG_V_I32 ? (int64_t)(int32_t)x : __double_as_longlong((double)__uint_as_float(x));
  }
  if (S.col_kind == PG_COL_RAW64) {
    const u32x2 v = gptr<u32x2>(S.data + (size_t)wt * (PG_WAVE_DOCS * 8))[doc];
    return (int64_t)(((uint64_t)bswap32(v.x) << 32) | bswap32(v.y));
  }
  const uint32_t d = packed_value_at(packed_wtile_base(S.data, wt, S.bits), doc, (uint32_t)S.bits);
  if (S.val_type == PG_V_I32) return (int64_t)(int32_t)gptr<uint32_t>(S.dict)[d];
  if (S.val_type == PG_V_F32) return __double_as_longlong((double)__uint_as_float(gptr<uint32_t>(S.dict)[d]));
  return (int64_t)gptr<uint64_t>(S.dict)[d];
}

// payload of one source for a doc: (register index | rank << log2m) of the value a DISTINCTCOUNTHLL offers, or the dictId
DEVFN uint32_t packed_hll_payload(uint32_t index_rank, int log2m) { return (index_rank & 0xFFFFu) | ((index_rank >> 16) << log2m); }

#endif  // PG_KERNEL_RADIX_H
