// Filter leaves over one wave tile: predicates, bit-packed access, the scan, posting, range-index and docId-range leaves, the
// index-only filter program and the register stack of match masks.
#ifndef PG_KERNEL_FILTER_H
#define PG_KERNEL_FILTER_H

#include "pg_kernel_common.h"

// ---- predicates -----------------------------------------------------------------------------------------------------------
struct RangeI32 { int32_t lo; uint32_t span; bool empty; };
DEVFN RangeI32 make_range_i32(int64_t lo, int64_t hi) {
  RangeI32 r;
  r.empty = hi < lo;
  r.lo = (int32_t)lo;
  r.span = (uint32_t)(hi - lo);
  return r;
}
DEVFN bool in_range_i32(const RangeI32& r, int32_t v) { return (uint32_t)(v - r.lo) <= r.span; }

template <class LeafT> DEVFN bool in_set_i64(const LeafT& L, int64_t v) {
  const GAS int64_t* s = gptr<int64_t>(L.set_values);
  bool hit = false;
#pragma unroll 1
  for (int i = 0; i < L.n_set; i++) hit |= (s[i] == v);
  return hit != (L.exclusive != 0);
}
template <class LeafT> DEVFN bool in_set_f64(const LeafT& L, double v) {
  const GAS double* s = gptr<double>(L.set_values);
  bool hit = false;
#pragma unroll 1
  for (int i = 0; i < L.n_set; i++) hit |= (s[i] == v);
  return hit != (L.exclusive != 0);
}

// KIND selects column layout × value type × predicate form.
enum ScanKind : int {
  SK_DICT_RANGE_SMALL, SK_DICT_RANGE_WIDE, SK_DICT_LUT_SMALL, SK_DICT_LUT_WIDE,
  SK_I32_RANGE, SK_I32_SET, SK_F32_RANGE, SK_F32_SET, SK_I64_RANGE, SK_I64_SET, SK_F64_RANGE, SK_F64_SET
};
DEVFN constexpr bool sk_small(int k) { return k == SK_DICT_RANGE_SMALL || k == SK_DICT_LUT_SMALL; }
DEVFN constexpr bool sk_dict(int k) { return k <= SK_DICT_LUT_WIDE; }
DEVFN constexpr bool sk_raw32(int k) { return k >= SK_I32_RANGE && k <= SK_F32_SET; }
DEVFN constexpr int sk_words(int k) { return sk_small(k) ? 2 : (sk_raw32(k) ? 4 : 8); }   // dwords fetched per quad

// ---- bit-packed (FixedBitSVForwardIndexReaderV2) access ---------------------------------------------------------------------
// tw: wave-uniform pointer to the wave tile's first dword (2 048 values start on a dword boundary for any width);
// q: quad index inside the wave tile (values 4q .. 4q+3).  SMALL (bits <= 8): the four values sit inside one 64-bit
// window; otherwise one window per value.
template <bool SMALL>
DEVFN void load_packed_quad(const GAS uint32_t* __restrict__ tw, uint32_t q, uint32_t bits, uint32_t* r) {
  if (SMALL) {
    const uint32_t di = __umul24(4u * q, bits) >> 5;   // q < 512, bits <= 8: v_mul_u32_u24 is full rate, v_mul_lo_u32 a quarter
    const u32x2 v = ldnt((const GAS u32x2_a4*)(tw + di));
    r[0] = v.x; r[1] = v.y;
  } else {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const uint32_t di = ((4u * q + (uint32_t)i) * bits) >> 5;
      const u32x2 v = ldnt((const GAS u32x2_a4*)(tw + di));
      r[2 * i] = v.x; r[2 * i + 1] = v.y;
    }
  }
}
template <bool SMALL>
DEVFN void decode_packed_quad(const uint32_t* r, uint32_t q, uint32_t bits, uint32_t mask, uint32_t out[4]) {
  if (SMALL) {
    const uint32_t sh = __umul24(4u * q, bits) & 31u;
    const uint64_t win = ((uint64_t)bswap32(r[0]) << 32) | (uint64_t)bswap32(r[1]);
    const uint32_t top = (uint32_t)((win << sh) >> 32);   // one 64-bit shift: the quad's four values now start at bit 31
    out[0] = top >> (32u - bits);
#pragma unroll
    for (int i = 1; i < 4; i++) out[i] = (top >> (32u - (uint32_t)(i + 1) * bits)) & mask;
  } else {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const uint32_t sh = ((4u * q + (uint32_t)i) * bits) & 31u;
      const uint64_t win = ((uint64_t)bswap32(r[2 * i]) << 32) | (uint64_t)bswap32(r[2 * i + 1]);
      out[i] = (uint32_t)(win >> (64u - sh - bits)) & mask;
    }
  }
}
DEVFN const GAS uint32_t* packed_wtile_base(const uint8_t* data, int wtile, int bits) {
  return gptr<uint32_t>(data + (size_t)wtile * (size_t)(PG_WAVE_DOCS / 8) * (size_t)bits);
}

template <int KIND, class LeafT>
DEVFN void load_quad(const LeafT& L, const GAS uint8_t* __restrict__ tb, uint32_t q, uint32_t* r) {
  if (sk_dict(KIND)) {
    load_packed_quad<sk_small(KIND)>((const GAS uint32_t*)tb, q, (uint32_t)L.bits, r);
  } else if (sk_raw32(KIND)) {
    const u32x4 v = ldnt((const GAS u32x4*)(tb + q * 16u));
    r[0] = v.x; r[1] = v.y; r[2] = v.z; r[3] = v.w;
  } else {
    const GAS u32x4* p = (const GAS u32x4*)(tb + q * 32u);
    const u32x4 a = ldnt(p), b = ldnt(p + 1);
    r[0] = a.x; r[1] = a.y; r[2] = a.z; r[3] = a.w; r[4] = b.x; r[5] = b.y; r[6] = b.z; r[7] = b.w;
  }
}

// Predicate over the 4 docs of a fetched quad → nibble.
template <int KIND, class LeafT>
DEVFN uint32_t test_quad(const LeafT& L, const uint32_t* r, uint32_t q, const RangeI32& r32) {
  uint32_t res = 0;
  if (sk_dict(KIND)) {
    uint32_t d[4];
    decode_packed_quad<sk_small(KIND)>(r, q, (uint32_t)L.bits, (1u << L.bits) - 1u, d);
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const bool m = (KIND == SK_DICT_RANGE_SMALL || KIND == SK_DICT_RANGE_WIDE)
                         ? in_range_i32(r32, (int32_t)d[i])
                         : (bool)((gptr<uint32_t>(L.lut)[d[i] >> 5] >> (d[i] & 31u)) & 1u);
      res |= (uint32_t)m << i;
    }
  } else if (sk_raw32(KIND)) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const uint32_t x = bswap32(r[i]);
      bool m;
      if (KIND == SK_I32_RANGE) m = in_range_i32(r32, (int32_t)x);
      else if (KIND == SK_I32_SET) m = in_set_i64(L, (int64_t)(int32_t)x);
      else if (KIND == SK_F32_RANGE) { const double f = (double)__uint_as_float(x); m = f >= __longlong_as_double(L.lo) && f <= __longlong_as_double(L.hi); }
      else m = in_set_f64(L, (double)__uint_as_float(x));
      res |= (uint32_t)m << i;
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const uint64_t x = ((uint64_t)bswap32(r[2 * i]) << 32) | bswap32(r[2 * i + 1]);
      bool m;
      if (KIND == SK_I64_RANGE) m = (int64_t)x >= L.lo && (int64_t)x <= L.hi;
      else if (KIND == SK_I64_SET) m = in_set_i64(L, (int64_t)x);
      else if (KIND == SK_F64_RANGE) { const double f = __longlong_as_double((int64_t)x); m = f >= __longlong_as_double(L.lo) && f <= __longlong_as_double(L.hi); }
      else m = in_set_f64(L, __longlong_as_double((int64_t)x));
      res |= (uint32_t)m << i;
    }
  }
  return res;
}

#ifndef PG_SCAN_B
#define PG_SCAN_B 4
#endif
// Scan leaf over one wave tile: evaluates the predicate for the docs of `cand` (quad layout) only — the whole tile for a
// pushed scan, the surviving candidates for a restricted one (ScanBasedDocIdIterator.applyAnd).  All quads of a lane
// are fetched before the first is tested; quads without a candidate are neither fetched nor tested.
template <int KIND, class LeafT>
DEVFN uint32_t scan_wtile(const LeafT& L, uint32_t cand, const GAS uint8_t* __restrict__ tb, int lane) {
  constexpr int W = sk_words(KIND);
  // quads in flight per lane: 4 (4 KB per wavefront for a raw INT column).  With 16 wavefronts per CU, 8 in flight measured slower
  // (cfg 3: 79.8 -> 80.5 % of the HBM roofline; the pure-scan probe 6.5 -> 6.95 TB/s, profiles/r02_scan_bw_probe.txt)
  constexpr int B = W <= 4 ? PG_SCAN_B : (PG_SCAN_B > 4 ? 4 : PG_SCAN_B);
  const RangeI32 r32 = make_range_i32(L.lo, L.hi);
  if ((KIND == SK_DICT_RANGE_SMALL || KIND == SK_DICT_RANGE_WIDE || KIND == SK_I32_RANGE) && r32.empty) return 0;
  uint32_t res = 0;
#pragma unroll
  for (int k0 = 0; k0 < 8; k0 += B) {
    // Loads are unconditional (a load under a per-lane branch is waited for inside the branch, which serialises the
    // batch); lanes whose quad has no candidate re-read quad `lane` of the tile's first KB instead, so no cache line is
    // touched that candidates do not need.
    uint32_t r[B][W];
#pragma unroll
    for (int u = 0; u < B; u++) {
      const uint32_t nib = (cand >> (4 * (k0 + u))) & 0xFu;
      load_quad<KIND>(L, tb, nib ? (uint32_t)((k0 + u) * 64 + lane) : 0u, r[u]);
    }
#pragma unroll
    for (int u = 0; u < B; u++) {
      const uint32_t nib = (cand >> (4 * (k0 + u))) & 0xFu;
      const uint32_t q = nib ? (uint32_t)((k0 + u) * 64 + lane) : 0u;
      if (KIND == SK_DICT_LUT_SMALL || KIND == SK_DICT_LUT_WIDE || KIND == SK_I32_SET || KIND == SK_F32_SET || KIND == SK_I64_SET || KIND == SK_F64_SET) {
        if (nib) res |= (test_quad<KIND>(L, r[u], q, r32) & nib) << (4 * (k0 + u));   // these read a LUT / value set
      } else {
        res |= (test_quad<KIND>(L, r[u], q, r32) & nib) << (4 * (k0 + u));
      }
    }
  }
  return res;
}

template <class LeafT>
DEVFN uint32_t scan_dispatch(const LeafT& L, uint32_t cand, int wtile, int lane) {
  if (L.col_kind == PG_COL_FIXED_BIT) {
    const GAS uint8_t* tb = (const GAS uint8_t*)packed_wtile_base(L.data, wtile, L.bits);
    if (L.pred_kind == PG_P_RANGE)
      return L.bits <= 8 ? scan_wtile<SK_DICT_RANGE_SMALL>(L, cand, tb, lane) : scan_wtile<SK_DICT_RANGE_WIDE>(L, cand, tb, lane);
    return L.bits <= 8 ? scan_wtile<SK_DICT_LUT_SMALL>(L, cand, tb, lane) : scan_wtile<SK_DICT_LUT_WIDE>(L, cand, tb, lane);
  }
  if (L.col_kind == PG_COL_RAW32) {
    const GAS uint8_t* tb = gptr<uint8_t>(L.data + (size_t)wtile * (PG_WAVE_DOCS * 4));
    if (L.val_type == PG_V_I32)
      return L.pred_kind == PG_P_RANGE ? scan_wtile<SK_I32_RANGE>(L, cand, tb, lane) : scan_wtile<SK_I32_SET>(L, cand, tb, lane);
    return L.pred_kind == PG_P_RANGE ? scan_wtile<SK_F32_RANGE>(L, cand, tb, lane) : scan_wtile<SK_F32_SET>(L, cand, tb, lane);
  }
  const GAS uint8_t* tb = gptr<uint8_t>(L.data + (size_t)wtile * (PG_WAVE_DOCS * 8));
  if (L.val_type == PG_V_I64)
    return L.pred_kind == PG_P_RANGE ? scan_wtile<SK_I64_RANGE>(L, cand, tb, lane) : scan_wtile<SK_I64_SET>(L, cand, tb, lane);
  return L.pred_kind == PG_P_RANGE ? scan_wtile<SK_F64_RANGE>(L, cand, tb, lane) : scan_wtile<SK_F64_SET>(L, cand, tb, lane);
}

// ---- posting leaf: OR the leaf's RoaringBitmap containers that intersect the wave tile (linear layout) ---------------------
// Container descriptors of the chunk are fetched with ONE vector load (lane e holds entry e) and broadcast with readlane,
// so the dependent chain per leaf is chunk_start → entries → payload regardless of how many postings are OR-ed.
// Array / run containers set their bits in the wavefront's private 2 048-bit LDS scratch.
template <class LeafT>
DEVFN uint32_t postings_wtile(const LeafT& L, int wtile, uint32_t valid_lin, uint32_t* __restrict__ wscratch, int lane) {
  const int chunk = wtile / PG_WTILES_PER_CHUNK;
  const int sub = wtile % PG_WTILES_PER_CHUNK;
  uint32_t acc = 0;
  if (chunk < L.dense_chunks) {   // wave-uniform: dense bitmap postings, address = base + 8 KB * chunk
    const uint32_t di = (uint32_t)wtile * 64u + (uint32_t)lane;   // = chunk * 2048 + sub * 64 + lane
    // unused pointers repeat dense[0] (OR is idempotent): 8 unconditional loads, no branches (skipping the unused slots with
    // wave-uniform branches costs the headline kernel its last free VGPRs: 16 bytes of scratch and 8 points of roofline, measured)
    uint32_t v[PG_MAX_DENSE];
#pragma unroll
    for (int j = 0; j < PG_MAX_DENSE; j++) v[j] = ldnt(gptr<uint32_t>(L.dense[j]) + di);
#pragma unroll
    for (int j = 0; j < PG_MAX_DENSE; j++) acc |= v[j];
  }
  uint32_t cs = 0, ce = 0;
  if (L.has_csr) { cs = gptr<uint32_t>(L.chunk_start)[chunk]; ce = gptr<uint32_t>(L.chunk_start)[chunk + 1]; }
  bool scatter = false;
  for (uint32_t base = cs; base < ce; base += 64) {
    const uint32_t n = (ce - base) < 64u ? (ce - base) : 64u;
    u32x4 ent = {0, 0, 0, 0};
    if ((uint32_t)lane < n) ent = gptr<u32x4>(L.entries)[base + lane];
    for (uint32_t e = 0; e < n; e++) {
      const uint32_t off_lo = __builtin_amdgcn_readlane(ent.x, e), off_hi = __builtin_amdgcn_readlane(ent.y, e);
      const uint32_t kt = __builtin_amdgcn_readlane(ent.w, e);   // key | type << 16
      if ((kt >> 16) == 1u) {
        const GAS uint32_t* w = gptr<uint32_t>(L.containers + (((uint64_t)off_hi << 32) | off_lo));
        acc |= w[sub * 64 + lane];
      } else {
        scatter = true;
      }
    }
  }
  if (scatter) {  // wave-uniform
    wscratch[lane] = acc;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    const uint32_t lo = (uint32_t)sub * PG_WAVE_DOCS, hi = lo + PG_WAVE_DOCS;  // low-16 range of this wave tile
    for (uint32_t e = cs; e < ce; e++) {
      const u32x4 ce4 = gptr<u32x4>(L.entries)[e];
      const uint64_t off = ((uint64_t)ce4.y << 32) | ce4.x;
      const uint32_t n = ce4.z, type = ce4.w >> 16;
      if (type == 0) {
        const GAS uint16_t* vals = gptr<uint16_t>(L.containers + off);
        uint32_t a = 0, b = n;  // lower_bound(lo)
        while (a < b) {
          const uint32_t m = (a + b) >> 1;
          if (vals[m] < lo) a = m + 1; else b = m;
        }
        for (uint32_t i = a + lane; i < n; i += 64) {
          uint32_t v = vals[i];
          if (v >= hi) break;
          v -= lo;
          atomicOr(&wscratch[v >> 5], 1u << (v & 31));
        }
      } else if (type == 2) {
        const GAS uint16_t* runs = gptr<uint16_t>(L.containers + off);
        for (uint32_t r = lane; r < n; r += 64) {
          uint32_t s = runs[2 * r], eend = s + runs[2 * r + 1] + 1;  // [s, eend)
          if (eend <= lo || s >= hi) continue;
          s = (s < lo ? lo : s) - lo;
          eend = (eend > hi ? hi : eend) - lo;
          const uint32_t fw = s >> 5, lw = (eend - 1) >> 5;
          const uint32_t fm = 0xFFFFFFFFu << (s & 31), lm = 0xFFFFFFFFu >> (31 - ((eend - 1) & 31));
          if (fw == lw) {
            atomicOr(&wscratch[fw], fm & lm);
          } else {
            atomicOr(&wscratch[fw], fm);
            for (uint32_t w = fw + 1; w < lw; w++) atomicOr(&wscratch[w], 0xFFFFFFFFu);
            atomicOr(&wscratch[lw], lm);
          }
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    acc = *(volatile uint32_t*)&wscratch[lane];
  }
  return (L.exclusive ? ~acc : acc) & valid_lin;
}

// One container's bits of the wave tile `sub` (2 048 docs of its 2^16-row chunk) OR-ed into the wavefront's LDS scratch (array / run
// containers; bitmap containers are read directly).  The caller zeroes / fences the scratch.
DEVFN void container_scatter(const GAS uint8_t* payload, uint32_t n, uint32_t type, int sub, uint32_t* __restrict__ wscratch, int lane) {
  const uint32_t lo = (uint32_t)sub * PG_WAVE_DOCS, hi = lo + PG_WAVE_DOCS;
  if (type == 0) {
    const GAS uint16_t* vals = (const GAS uint16_t*)payload;
    uint32_t a = 0, b = n;
    while (a < b) {
      const uint32_t m = (a + b) >> 1;
      if (vals[m] < lo) a = m + 1; else b = m;
    }
    for (uint32_t i = a + lane; i < n; i += 64) {
      uint32_t v = vals[i];
      if (v >= hi) break;
      v -= lo;
      atomicOr(&wscratch[v >> 5], 1u << (v & 31));
    }
  } else if (type == 2) {
    const GAS uint16_t* runs = (const GAS uint16_t*)payload;
    for (uint32_t r = lane; r < n; r += 64) {
      uint32_t s = runs[2 * r], eend = s + runs[2 * r + 1] + 1;
      if (eend <= lo || s >= hi) continue;
      s = (s < lo ? lo : s) - lo;
      eend = (eend > hi ? hi : eend) - lo;
      const uint32_t fw = s >> 5, lw = (eend - 1) >> 5;
      const uint32_t fm = 0xFFFFFFFFu << (s & 31), lm = 0xFFFFFFFFu >> (31 - ((eend - 1) & 31));
      if (fw == lw) atomicOr(&wscratch[fw], fm & lm);
      else {
        atomicOr(&wscratch[fw], fm);
        for (uint32_t w = fw + 1; w < lw; w++) atomicOr(&wscratch[w], 0xFFFFFFFFu);
        atomicOr(&wscratch[lw], lm);
      }
    }
  }
}

// Bit-sliced range index leaf (PgRangeIdxLeaf): the descriptors of the chunk's slices arrive with one vector load (lane s holds slice
// s), each slice's 2 048-bit window is folded into the two running "<= threshold" masks.
template <class LeafT>
DEVFN uint32_t rangeidx_wtile(const LeafT& L, int wtile, uint32_t valid_lin, uint32_t* __restrict__ wscratch, int lane) {
  const int chunk = wtile / PG_WTILES_PER_CHUNK, sub = wtile % PG_WTILES_PER_CHUNK;
  u32x4 ent = {0u, 0u, 0u, 3u << 16};
  if (lane < L.n_slices) ent = gptr<u32x4>(L.descs)[(size_t)chunk * (size_t)L.n_slices + (size_t)lane];
  uint32_t le_hi = 0xFFFFFFFFu, le_lo = 0xFFFFFFFFu;
  for (int s = 0; s < L.n_slices; s++) {
    const uint32_t off_lo = __builtin_amdgcn_readlane(ent.x, s), off_hi = __builtin_amdgcn_readlane(ent.y, s);
    const uint32_t n = __builtin_amdgcn_readlane(ent.z, s), type = __builtin_amdgcn_readlane(ent.w, s) >> 16;
    const GAS uint8_t* payload = gptr<uint8_t>(L.containers + (((uint64_t)off_hi << 32) | off_lo));
    uint32_t S = 0;
    if (type == 1) S = ((const GAS uint32_t*)payload)[sub * 64 + lane];
    else if (type != 3) {   // wave-uniform
      wscratch[lane] = 0;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      container_scatter(payload, n, type, sub, wscratch, lane);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
      S = *(volatile uint32_t*)&wscratch[lane];
    }
    le_hi = ((L.hi >> s) & 1ULL) ? (le_hi | S) : (le_hi & S);
    le_lo = ((L.lo_m1 >> s) & 1ULL) ? (le_lo | S) : (le_lo & S);
  }
  uint32_t r = L.has_hi ? le_hi : 0xFFFFFFFFu;
  if (L.has_lo) r &= ~le_lo;
  return r & valid_lin;
}

// docId ranges (sorted index / match-all), linear layout
template <class LeafT>
DEVFN uint32_t ranges_wtile(const LeafT& L, int64_t wbase, uint32_t valid_lin, int lane) {
  const int64_t wb = wbase + (int64_t)lane * 32, we = wb + 31;
  const int64_t tile_end = wbase + PG_WAVE_DOCS - 1;
  int a = 0, b = L.n;   // first range whose hi >= wbase (ranges ascending, disjoint)
  while (a < b) {
    const int m = (a + b) >> 1;
    if ((int64_t)gptr<int32_t>(L.hi)[m] < wbase) a = m + 1; else b = m;
  }
  uint32_t acc = 0;
  for (int r = a; r < L.n; r++) {
    const int64_t lo = gptr<int32_t>(L.lo)[r], hi = gptr<int32_t>(L.hi)[r];
    if (lo > tile_end) break;
    if (hi < wb || lo > we) continue;
    const int64_t s = lo > wb ? lo - wb : 0, e = hi < we ? hi - wb : 31;
    acc |= (0xFFFFFFFFu << s) & (0xFFFFFFFFu >> (31 - e));
  }
  return acc & valid_lin;
}

struct LinStack {
  uint32_t s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0, s5 = 0;
  DEVFN void push(uint32_t v) { s5 = s4; s4 = s3; s3 = s2; s2 = s1; s1 = s0; s0 = v; }
  DEVFN void drop() { s0 = s1; s1 = s2; s2 = s3; s3 = s4; s4 = s5; }
};

// index-only filter program in linear layout (one dword = 32 consecutive docs per lane)
template <bool WORDS>   // WORDS: also understands PG_F_PUSH_WORDS (interpreter kernels only: the specialised kernels sit at 128 VGPRs)
DEVFN uint32_t index_program_lin(const PgQueryPlan& p, int n_instr, int wt, int64_t wbase, uint32_t valid_l, uint32_t* wscratch, int lane) {
  LinStack st;
  for (int i = 0; i < n_instr; i++) {
    const int op = cptr(p.instrs)[i].op, arg = cptr(p.instrs)[i].arg;
    switch (op) {
      case PG_F_PUSH_POSTINGS: st.push(postings_wtile(cptr(p.postings)[arg], wt, valid_l, wscratch, lane)); break;
      case PG_F_PUSH_RANGES: st.push(ranges_wtile(cptr(p.ranges)[arg], wbase, valid_l, lane)); break;
      case PG_F_PUSH_WORDS: if (WORDS) st.push(gptr<uint32_t>(cptr(p.ranges)[arg].words)[(int64_t)wt * 64 + lane] & valid_l); break;
      case PG_F_PUSH_RANGEIDX: if (WORDS) st.push(rangeidx_wtile(cptr(p.rangeidx)[arg], wt, valid_l, wscratch, lane)); break;
      case PG_F_PUSH_ALL: st.push(valid_l); break;
      case PG_F_PUSH_NONE: st.push(0u); break;
      case PG_F_AND: { const uint32_t b = st.s0; st.drop(); st.s0 &= b; break; }
      case PG_F_OR: { const uint32_t b = st.s0; st.drop(); st.s0 |= b; break; }
      case PG_F_NOT: st.s0 = (~st.s0) & valid_l; break;
      default: break;
    }
  }
  return st.s0;
}

// Register stack of match masks; the top is always s0 (push / pop shift the others), so no dynamic register indexing.
struct MaskStack {
  uint32_t s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0, s5 = 0;
  DEVFN void push(uint32_t v) { s5 = s4; s4 = s3; s3 = s2; s2 = s1; s1 = s0; s0 = v; }
  DEVFN void drop() { s0 = s1; s1 = s2; s2 = s3; s3 = s4; s4 = s5; }
  DEVFN void pop_and() { const uint32_t b = s0; drop(); s0 &= b; }
  DEVFN void pop_or() { const uint32_t b = s0; drop(); s0 |= b; }
};

#endif  // PG_KERNEL_FILTER_H
