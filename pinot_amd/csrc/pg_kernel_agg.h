// Aggregation of the matching docs of one wave tile: accumulator updates, the auxiliary states (DISTINCTCOUNT sets, HyperLogLog
// registers), the general and the fast-path aggregator and the workgroup epilogue.
#ifndef PG_KERNEL_AGG_H
#define PG_KERNEL_AGG_H

#include "pg_kernel_filter.h"
#include "pg_fixed_point.h"

// ---- accumulator updates ------------------------------------------------------------------------------------------------
DEVFN int64_t f64_order_key(double v) {  // order-preserving map double → int64 (MIN/MAX through integer atomics)
  const int64_t b = __double_as_longlong(v);
  return b ^ ((b >> 63) & 0x7FFFFFFFFFFFFFFFLL);
}
DEVFN void acc_int(int64_t* slot, int fn, int64_t v) {
  if (fn == PG_ACC_SUM) atomicAdd(reinterpret_cast<unsigned long long*>(slot), (unsigned long long)v);
  else if (fn == PG_ACC_MIN) atomicMin(reinterpret_cast<long long*>(slot), (long long)v);
  else atomicMax(reinterpret_cast<long long*>(slot), (long long)v);
}
DEVFN int64_t fx_digit(double x, int q, int limb) { return pg_fx_digit(x, q, limb); }   // pg_fixed_point.h
DEVFN int64_t long_digit(int64_t v, int limb) { return pg_long_digit(v, limb); }
// one accumulator update from a double / an int64 value, whatever the accumulator's value kind
DEVFN void acc_float(int64_t* slot, int fn, double v);
DEVFN void acc_from_double(int64_t* slot, const PgAccOp& op, double v, int q) {
  if (op.is_float == PG_ACCV_FIXED_DIGIT) atomicAdd(reinterpret_cast<unsigned long long*>(slot), (unsigned long long)fx_digit(v, q, op.limb));
  else acc_float(slot, op.fn, v);
}
DEVFN void acc_from_int(int64_t* slot, const PgAccOp& op, int64_t v) {
  if (op.is_float == PG_ACCV_LONG_DIGIT) atomicAdd(reinterpret_cast<unsigned long long*>(slot), (unsigned long long)long_digit(v, op.limb));
  else acc_int(slot, op.fn, v);
}
DEVFN void acc_float(int64_t* slot, int fn, double v) {
  if (fn == PG_ACC_SUM) { atomicAdd(reinterpret_cast<double*>(slot), v); return; }
  if (v != v) return;   // Java: NaN > x and NaN < x are false → NaN never replaces the holder
  const int64_t k = f64_order_key(v);
  if (fn == PG_ACC_MIN) atomicMin(reinterpret_cast<long long*>(slot), (long long)k);
  else atomicMax(reinterpret_cast<long long*>(slot), (long long)k);
}

// ---- auxiliary accumulators (DISTINCTCOUNT dictId sets, HyperLogLog registers) in HBM ------------------------------------------
// Both are monotone (bits only get set, registers only grow), so an update first reads the current state and skips the
// atomic when it would change nothing — after warm-up almost every doc does (a stale read only costs a redundant atomic).
DEVFN uint32_t murmur_hash_long_dev(int64_t data) {   // stream-lib MurmurHash.hashLong
  const uint32_t m = 0x5bd1e995u;
  uint32_t h = 0;
  uint32_t k = (uint32_t)(uint64_t)data * m;
  k ^= k >> 24;
  h ^= k * m;
  k = (uint32_t)((uint64_t)data >> 32) * m;
  k ^= k >> 24;
  h *= m;
  h ^= k * m;
  h ^= h >> 13;
  h *= m;
  h ^= h >> 15;
  return h;
}
DEVFN uint32_t hll_index_rank_dev(uint32_t x, int log2m) {   // register index | rank << 16
  const uint32_t j = x >> (32 - log2m);
  const uint32_t w = (x << log2m) | ((1u << (log2m - 1)) + 1u);
  return j | ((uint32_t)(__clz((int)w) + 1) << 16);
}
DEVFN void set_add(uint32_t* words, uint32_t id) {
  uint32_t* w = words + (id >> 5);
  const uint32_t bit = 1u << (id & 31u);
  if (!(__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) atomicOr(w, bit);
}
DEVFN uint32_t bytemax4(uint32_t a, uint32_t b) {   // per-byte unsigned max (four HyperLogLog registers)
  uint32_t r = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint32_t x = (a >> (8 * k)) & 0xFFu, y = (b >> (8 * k)) & 0xFFu;
    r |= (x > y ? x : y) << (8 * k);
  }
  return r;
}
DEVFN void hll_update(uint8_t* regs, uint32_t idx, uint32_t rank) {
  uint32_t* w = reinterpret_cast<uint32_t*>(regs + (idx & ~3u));
  const uint32_t sh = (idx & 3u) * 8u;
  uint32_t cur = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  while (((cur >> sh) & 0xFFu) < rank) {
    const uint32_t nv = (cur & ~(0xFFu << sh)) | (rank << sh);
    const uint32_t prev = atomicCAS(w, cur, nv);
    if (prev == cur) break;
    cur = prev;
  }
}

// ---- auxiliary accumulators of one batch of quads (slot[u][i] = table slot of doc i of quad k0+u, mb = the batch's mask) ----
template <int B>
DEVFN void aux_update_batch(const PgQueryPlan& p, uint32_t mb, int k0, int wtile, const uint32_t (&slot_in)[B][4], int lane, uint32_t part_lo) {
  uint32_t slot[B][4];   // the auxiliary regions are indexed by the GLOBAL group (slots are range-local in PG_AGG_LDS_PART)
#pragma unroll
  for (int u = 0; u < B; u++)
#pragma unroll
    for (int i = 0; i < 4; i++) slot[u][i] = slot_in[u][i] + (part_lo << p.replica_shift);
  // ---- auxiliary accumulators: DISTINCTCOUNT dictId sets / HyperLogLog registers (HBM regions) ---------------------------
  // Dictionary sources run in three batched stages over the 4·B docs of the lane — dictIds, (index, rank) look-ups,
  // current state words — so that 4·B gathers are in flight per lane; only docs that would change the state go on to
  // the atomic.  Lanes / docs outside the mask use clamped (valid) addresses and are masked at the atomic.
  for (int xa = 0; xa < p.n_aux; xa++) {
    PgAuxOp A = p.aux[xa];
    if (A.lds_offset >= 0) {   // this workgroup's own state in LDS (generic pointer into the LDS aperture: flat atomics)
      extern __shared__ __attribute__((aligned(16))) uint64_t smem_aux[];
      A.base = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(smem_aux) + A.lds_offset);
    } else {
      A.base = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(A.base) + (size_t)(blockIdx.x & (uint32_t)(A.n_rep - 1)) * (size_t)A.rep_bytes);
    }
    const PgValueSrc& S = p.srcs[A.src];
    if (A.kind == PG_AUX_HLL_BYTES) {
      // Serialized HyperLogLogs of a star-tree pair column (one byte per register after upload): HyperLogLog#addAll = register-wise
      // max.  One matching doc at a time, the whole wavefront on its registers: lane L merges dwords L, L+64, ... of the doc
      // into the group's registers (read first, CAS only where a register grows).
      const uint32_t n_dw = (uint32_t)A.stride >> 2;
      const GAS uint8_t* src = gptr<uint8_t>(S.data);
#pragma unroll
      for (int u = 0; u < B; u++)
#pragma unroll
        for (int i = 0; i < 4; i++) {
          unsigned long long ball = __ballot((mb >> (4 * u + i)) & 1u);
          while (ball) {
            // four docs in flight (their loads are independent); short of four, the first is repeated — max is idempotent
            const GAS uint32_t* sw[4];
            uint32_t* dst[4];
            int l0 = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
              int l = l0;
              if (j == 0 || ball) { l = __builtin_ctzll(ball); ball &= ball - 1; }
              if (j == 0) l0 = l;
              const size_t g = (size_t)((uint32_t)__builtin_amdgcn_readlane((int)slot[u][i], l) >> p.replica_shift);
              const int64_t doc = (int64_t)wtile * PG_WAVE_DOCS + 4 * ((k0 + u) * 64 + l) + i;
              sw[j] = (const GAS uint32_t*)(src + doc * (int64_t)A.stride);
              dst[j] = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(A.base) + g * (size_t)A.stride);
            }
            for (uint32_t w = (uint32_t)lane; w < n_dw; w += 64) {
              uint32_t v[4], cur[4];
#pragma unroll
              for (int j = 0; j < 4; j++) v[j] = sw[j][w];
#pragma unroll
              for (int j = 0; j < 4; j++) cur[j] = __hip_atomic_load(dst[j] + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
              for (int j = 0; j < 4; j++) {
                uint32_t c = cur[j];
                for (;;) {
                  const uint32_t nv = bytemax4(c, v[j]);
                  if (nv == c) break;
                  const uint32_t prev = atomicCAS(dst[j] + w, c, nv);
                  if (prev == c) break;
                  c = prev;
                }
              }
            }
          }
        }
    } else if (S.col_kind == PG_COL_FIXED_BIT) {
      const GAS uint32_t* tw = packed_wtile_base(S.data, wtile, S.bits);
      const uint32_t bits = (uint32_t)S.bits, mask = (1u << S.bits) - 1u;
      uint32_t d[B][4];
      if (bits <= 8) {
        uint32_t r[B][2];
#pragma unroll
        for (int u = 0; u < B; u++) load_packed_quad<true>(tw, ((mb >> (4 * u)) & 0xFu) ? (uint32_t)((k0 + u) * 64 + lane) : 0u, bits, r[u]);
#pragma unroll
        for (int u = 0; u < B; u++) decode_packed_quad<true>(r[u], ((mb >> (4 * u)) & 0xFu) ? (uint32_t)((k0 + u) * 64 + lane) : 0u, bits, mask, d[u]);
      } else {
        uint32_t r[B][8];
#pragma unroll
        for (int u = 0; u < B; u++) load_packed_quad<false>(tw, ((mb >> (4 * u)) & 0xFu) ? (uint32_t)((k0 + u) * 64 + lane) : 0u, bits, r[u]);
#pragma unroll
        for (int u = 0; u < B; u++) decode_packed_quad<false>(r[u], ((mb >> (4 * u)) & 0xFu) ? (uint32_t)((k0 + u) * 64 + lane) : 0u, bits, mask, d[u]);
      }
      uint32_t* wp[B][4];
      uint32_t want[B][4];   // DICT_SET: the bit; HLL: rank << shift-in-word, with the shift in the low 5 bits of `sh`
      uint32_t sh[B][4];
      if (A.kind == PG_AUX_DICT_SET) {
#pragma unroll
        for (int u = 0; u < B; u++)
#pragma unroll
          for (int i = 0; i < 4; i++) {
            const size_t g = (size_t)(slot[u][i] >> p.replica_shift);
            wp[u][i] = A.base + g * (size_t)A.stride + (d[u][i] >> 5);
            want[u][i] = 1u << (d[u][i] & 31u);
            sh[u][i] = 0;
          }
      } else {
        uint32_t e[B][4];
#pragma unroll
        for (int u = 0; u < B; u++)
#pragma unroll
          for (int i = 0; i < 4; i++) e[u][i] = gptr<uint32_t>(A.lut)[d[u][i]];
#pragma unroll
        for (int u = 0; u < B; u++)
#pragma unroll
          for (int i = 0; i < 4; i++) {
            const size_t g = (size_t)(slot[u][i] >> p.replica_shift);
            const uint32_t idx = e[u][i] & 0xFFFFu;
            wp[u][i] = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(A.base) + g * (size_t)A.stride + (idx & ~3u));
            sh[u][i] = (idx & 3u) * 8u;
            want[u][i] = e[u][i] >> 16;
          }
      }
      uint32_t cur[B][4];
#pragma unroll
      for (int u = 0; u < B; u++)
#pragma unroll
        for (int i = 0; i < 4; i++) cur[u][i] = __hip_atomic_load(wp[u][i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
      for (int u = 0; u < B; u++)
#pragma unroll
        for (int i = 0; i < 4; i++) {
          if ((mb >> (4 * u + i)) & 1u) {
            if (A.kind == PG_AUX_DICT_SET) {
              if (!(cur[u][i] & want[u][i])) atomicOr(wp[u][i], want[u][i]);
            } else {
              uint32_t c = cur[u][i];
              while (((c >> sh[u][i]) & 0xFFu) < want[u][i]) {
                const uint32_t nv = (c & ~(0xFFu << sh[u][i])) | (want[u][i] << sh[u][i]);
                const uint32_t prev = atomicCAS(wp[u][i], c, nv);
                if (prev == c) break;
                c = prev;
              }
            }
          }
        }
    } else {   // raw column: DISTINCTCOUNTHLL hashes the value on the fly
#pragma unroll
      for (int u = 0; u < B; u++) {
        const uint32_t nib = (mb >> (4 * u)) & 0xFu;
        if (nib) {
          const uint32_t q = (uint32_t)((k0 + u) * 64 + lane);
          int64_t v[4];   // the long the value hashes as (Integer/Long value, Float raw int bits, Double raw long bits)
          if (S.col_kind == PG_COL_RAW32) {
            const u32x4 x = *gptr<u32x4>(S.data + (size_t)wtile * (PG_WAVE_DOCS * 4) + q * 16u);
            v[0] = (int64_t)(int32_t)bswap32(x.x); v[1] = (int64_t)(int32_t)bswap32(x.y);
            v[2] = (int64_t)(int32_t)bswap32(x.z); v[3] = (int64_t)(int32_t)bswap32(x.w);
          } else {
            const GAS u32x4* pp = gptr<u32x4>(S.data + (size_t)wtile * (PG_WAVE_DOCS * 8) + q * 32u);
            const u32x4 a = pp[0], b = pp[1];
            v[0] = (int64_t)(((uint64_t)bswap32(a.x) << 32) | bswap32(a.y)); v[1] = (int64_t)(((uint64_t)bswap32(a.z) << 32) | bswap32(a.w));
            v[2] = (int64_t)(((uint64_t)bswap32(b.x) << 32) | bswap32(b.y)); v[3] = (int64_t)(((uint64_t)bswap32(b.z) << 32) | bswap32(b.w));
          }
#pragma unroll
          for (int i = 0; i < 4; i++) {
            if ((nib >> i) & 1u) {
              const size_t g = (size_t)(slot[u][i] >> p.replica_shift);
              const uint32_t e = hll_index_rank_dev(murmur_hash_long_dev(v[i]), A.log2m);
              hll_update(reinterpret_cast<uint8_t*>(A.base) + g * (size_t)A.stride, e & 0xFFFFu, e >> 16);
            }
          }
        }
      }
    }
  }

}

// Aggregates the matching docs (quad-layout mask m) of one wave tile into `table` ([n_ops][G*R] int64 slots, LDS or HBM):
// group columns of any width, raw 32/64-bit and dictionary-encoded sources.  B quads per lane are in flight at a time; like
// the filter stage, every load of a stage is issued unconditionally (lanes whose quad has no match re-read quad 0 of the
// tile) before the first is used — a load under a per-lane branch is waited for inside the branch.
// DIG: the plan has digit accumulators (exact SUMs of FLOAT / DOUBLE / wide LONG sources, PgAccValueKind); kernels without them are
// compiled without that code (it costs the others ~40 spilled VGPRs).
template <int B, bool AUX = true, bool DIG = false>
DEVFN void aggregate_wtile(const PgQueryPlan& p, uint32_t m, int wtile, int64_t* table, int lane, uint32_t rep, uint32_t part_lo = 0) {
  const uint32_t R = (uint32_t)p.replicas;
  const bool part = p.agg_mode == PG_AGG_LDS_PART;
  const uint32_t stride = part ? (uint32_t)p.part_groups : (uint32_t)p.n_groups * R;   // slots per op
#pragma unroll
  for (int k0 = 0; k0 < 8; k0 += B) {
    uint32_t mb = B == 8 ? m : ((m >> (4 * k0)) & ((1u << (4 * (B & 7))) - 1u));
    if (__ballot(mb != 0) == 0) continue;   // wave-uniform: the HLL-bytes merge needs every lane of the wavefront
    uint32_t qi[B];                         // quad index of each in-flight quad, clamped to 0 where the lane has no match
#pragma unroll
    for (int u = 0; u < B; u++) qi[u] = ((mb >> (4 * u)) & 0xFu) ? (uint32_t)((k0 + u) * 64 + lane) : 0u;
    uint32_t slot[B][4];
#pragma unroll
    for (int u = 0; u < B; u++)
#pragma unroll
      for (int i = 0; i < 4; i++) slot[u][i] = rep;
    // Up to PG_BATCH_GCOLS narrow group columns are requested together (one memory round trip for the whole key instead of one
    // per column: with few bytes per load this stage is latency-, not bandwidth-bound), together with the first raw 32-bit
    // source.  Wider / further columns follow one at a time.
    constexpr int PG_BATCH_GCOLS = 4;
    int n_batched = 0;
    while (n_batched < p.n_group_cols && n_batched < PG_BATCH_GCOLS && p.gcols[n_batched].bits <= 8) n_batched++;
    int o_first = 0;
    while (o_first < p.n_ops && p.ops[o_first].src < 0) o_first++;
    const bool prefetch0 = o_first < p.n_ops && p.srcs[p.ops[o_first].src].col_kind == PG_COL_RAW32;
    uint32_t x0[B][4];
    {
      uint32_t rg[PG_BATCH_GCOLS][B][2];
#pragma unroll
      for (int g = 0; g < PG_BATCH_GCOLS; g++)
        if (g < n_batched) {
          const GAS uint32_t* tw = packed_wtile_base(p.gcols[g].data, wtile, p.gcols[g].bits);
#pragma unroll
          for (int u = 0; u < B; u++) load_packed_quad<true>(tw, qi[u], (uint32_t)p.gcols[g].bits, rg[g][u]);
        }
      if (prefetch0) {
        const GAS uint8_t* tb = gptr<uint8_t>(p.srcs[p.ops[o_first].src].data + (size_t)wtile * (PG_WAVE_DOCS * 4));
#pragma unroll
        for (int u = 0; u < B; u++) {
          const u32x4 v = ldnt((const GAS u32x4*)(tb + qi[u] * 16u));
          x0[u][0] = v.x; x0[u][1] = v.y; x0[u][2] = v.z; x0[u][3] = v.w;
        }
      }
#pragma unroll
      for (int g = 0; g < PG_BATCH_GCOLS; g++)
        if (g < n_batched) {
          const uint32_t bits = (uint32_t)p.gcols[g].bits, mask = (1u << bits) - 1u, mult = (uint32_t)p.gcols[g].mult * R;
#pragma unroll
          for (int u = 0; u < B; u++) {
            uint32_t d[4];
            decode_packed_quad<true>(rg[g][u], qi[u], bits, mask, d);
#pragma unroll
            for (int i = 0; i < 4; i++) slot[u][i] += d[i] * mult;
          }
        }
    }
    for (int g = n_batched; g < p.n_group_cols; g++) {
      const PgGroupCol& gc = p.gcols[g];
      const GAS uint32_t* tw = packed_wtile_base(gc.data, wtile, gc.bits);
      const uint32_t bits = (uint32_t)gc.bits, mask = (1u << gc.bits) - 1u;
      const uint32_t mult = (uint32_t)gc.mult * R;
      if (bits <= 8) {
        uint32_t r[B][2];
#pragma unroll
        for (int u = 0; u < B; u++) load_packed_quad<true>(tw, qi[u], bits, r[u]);
#pragma unroll
        for (int u = 0; u < B; u++) {
          uint32_t d[4];
          decode_packed_quad<true>(r[u], qi[u], bits, mask, d);
#pragma unroll
          for (int i = 0; i < 4; i++) slot[u][i] += d[i] * mult;
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
          for (int i = 0; i < 4; i++) slot[u][i] += d[i] * mult;
        }
      }
    }
    if (part) {   // keep only the docs whose key falls in this workgroup's range; slots become range-local
      uint32_t keep = 0;
#pragma unroll
      for (int u = 0; u < B; u++)
#pragma unroll
        for (int i = 0; i < 4; i++) {
          slot[u][i] -= part_lo;
          keep |= (uint32_t)(slot[u][i] < (uint32_t)p.part_groups) << (4 * u + i);
        }
      mb &= keep;
      if (__ballot(mb != 0) == 0) continue;
#pragma unroll
      for (int u = 0; u < B; u++) qi[u] = ((mb >> (4 * u)) & 0xFu) ? (uint32_t)((k0 + u) * 64 + lane) : 0u;
    }
    int o = 0;
    // ops without a source column (src < 0) come first: COUNT, and MIN(docId) when numGroupsLimit can bite
    for (; o < p.n_ops && p.ops[o].src < 0; o++) {
      int64_t* base = table + (size_t)o * stride;
      if (p.ops[o].fn == PG_ACC_COUNT) {
#pragma unroll
        for (int u = 0; u < B; u++)
#pragma unroll
          for (int i = 0; i < 4; i++)
            if ((mb >> (4 * u + i)) & 1u) atomicAdd(reinterpret_cast<unsigned long long*>(base + slot[u][i]), 1ULL);
      } else {
#pragma unroll
        for (int u = 0; u < B; u++)
#pragma unroll
          for (int i = 0; i < 4; i++)
            if ((mb >> (4 * u + i)) & 1u)
              atomicMin(reinterpret_cast<long long*>(base + slot[u][i]),
                        (long long)wtile * PG_WAVE_DOCS + 4 * ((k0 + u) * 64 + lane) + i);
      }
    }
    while (o < p.n_ops) {
      const int src = p.ops[o].src;
      const PgValueSrc& S = p.srcs[src];
      int o_end = o;
      while (o_end < p.n_ops && p.ops[o_end].src == src) o_end++;
      const bool wide_val = S.val_type == PG_V_I64 || S.val_type == PG_V_F64;
      if (!wide_val) {
        // ---- 32-bit values: raw big-endian INT / FLOAT, or dictionary-encoded ------------------------------------------------
        uint32_t x[B][4];
        if (S.col_kind == PG_COL_RAW32) {
          if (prefetch0 && o == o_first) {   // requested together with the group columns (docs later found out of range included)
#pragma unroll
            for (int u = 0; u < B; u++)
#pragma unroll
              for (int i = 0; i < 4; i++) x[u][i] = x0[u][i];
          } else {
            const GAS uint8_t* tb = gptr<uint8_t>(S.data + (size_t)wtile * (PG_WAVE_DOCS * 4));
#pragma unroll
            for (int u = 0; u < B; u++) {
              const u32x4 v = ldnt((const GAS u32x4*)(tb + qi[u] * 16u));
              x[u][0] = v.x; x[u][1] = v.y; x[u][2] = v.z; x[u][3] = v.w;
            }
          }
#pragma unroll
          for (int u = 0; u < B; u++)
#pragma unroll
            for (int i = 0; i < 4; i++) x[u][i] = bswap32(x[u][i]);
        } else {
          const GAS uint32_t* tw = packed_wtile_base(S.data, wtile, S.bits);
          const uint32_t bits = (uint32_t)S.bits, mask = (1u << S.bits) - 1u;
          uint32_t d[B][4];
          if (bits <= 8) {
            uint32_t r[B][2];
#pragma unroll
            for (int u = 0; u < B; u++) load_packed_quad<true>(tw, qi[u], bits, r[u]);
#pragma unroll
            for (int u = 0; u < B; u++) decode_packed_quad<true>(r[u], qi[u], bits, mask, d[u]);
          } else {
            uint32_t r[B][8];
#pragma unroll
            for (int u = 0; u < B; u++) load_packed_quad<false>(tw, qi[u], bits, r[u]);
#pragma unroll
            for (int u = 0; u < B; u++) decode_packed_quad<false>(r[u], qi[u], bits, mask, d[u]);
          }
#pragma unroll
          for (int u = 0; u < B; u++)
#pragma unroll
            for (int i = 0; i < 4; i++) x[u][i] = gptr<uint32_t>(S.dict)[d[u][i]];   // every dictId read is a valid one
        }
        for (int k = o; k < o_end; k++) {
          const PgAccOp opk = p.ops[k];
          const int fn = opk.fn;
          int64_t* base = table + (size_t)k * stride;
          if (S.val_type == PG_V_I32) {
#pragma unroll
            for (int u = 0; u < B; u++)
#pragma unroll
              for (int i = 0; i < 4; i++)
                if ((mb >> (4 * u + i)) & 1u) acc_int(base + slot[u][i], fn, (int64_t)(int32_t)x[u][i]);
          } else if (DIG && opk.is_float == PG_ACCV_FIXED_DIGIT) {   // wave-uniform: the branch stays outside the unrolled loops
            const int q = S.fx_q, limb = opk.limb;
#pragma unroll
            for (int u = 0; u < B; u++)
#pragma unroll
              for (int i = 0; i < 4; i++)
                if ((mb >> (4 * u + i)) & 1u)
                  atomicAdd(reinterpret_cast<unsigned long long*>(base + slot[u][i]), (unsigned long long)fx_digit((double)__uint_as_float(x[u][i]), q, limb));
          } else {
#pragma unroll
            for (int u = 0; u < B; u++)
#pragma unroll
              for (int i = 0; i < 4; i++)
                if ((mb >> (4 * u + i)) & 1u) acc_float(base + slot[u][i], fn, (double)__uint_as_float(x[u][i]));
          }
        }
      } else {
        // ---- 64-bit values: raw big-endian LONG / DOUBLE (32 B per quad), or dictionary-encoded; four quads at a time -------------
        constexpr int WB = B < 4 ? B : 4;
#pragma unroll
        for (int h = 0; h < B; h += WB) {
          if (__ballot(((mb >> (4 * h)) & ((1u << (4 * WB)) - 1u)) != 0) == 0) continue;
          uint64_t x[WB][4];
          if (S.col_kind == PG_COL_RAW64) {
            const GAS uint8_t* tb = gptr<uint8_t>(S.data + (size_t)wtile * (PG_WAVE_DOCS * 8));
            u32x4 a[WB], b[WB];
#pragma unroll
            for (int u = 0; u < WB; u++) {
              const GAS u32x4* pp = (const GAS u32x4*)(tb + qi[h + u] * 32u);
              a[u] = ldnt(pp);
              b[u] = ldnt(pp + 1);
            }
#pragma unroll
            for (int u = 0; u < WB; u++) {
              x[u][0] = ((uint64_t)bswap32(a[u].x) << 32) | bswap32(a[u].y); x[u][1] = ((uint64_t)bswap32(a[u].z) << 32) | bswap32(a[u].w);
              x[u][2] = ((uint64_t)bswap32(b[u].x) << 32) | bswap32(b[u].y); x[u][3] = ((uint64_t)bswap32(b[u].z) << 32) | bswap32(b[u].w);
            }
          } else {
            const GAS uint32_t* tw = packed_wtile_base(S.data, wtile, S.bits);
            const uint32_t bits = (uint32_t)S.bits, mask = (1u << S.bits) - 1u;
            uint32_t d[WB][4];
            if (bits <= 8) {
              uint32_t r[WB][2];
#pragma unroll
              for (int u = 0; u < WB; u++) load_packed_quad<true>(tw, qi[h + u], bits, r[u]);
#pragma unroll
              for (int u = 0; u < WB; u++) decode_packed_quad<true>(r[u], qi[h + u], bits, mask, d[u]);
            } else {
              uint32_t r[WB][8];
#pragma unroll
              for (int u = 0; u < WB; u++) load_packed_quad<false>(tw, qi[h + u], bits, r[u]);
#pragma unroll
              for (int u = 0; u < WB; u++) decode_packed_quad<false>(r[u], qi[h + u], bits, mask, d[u]);
            }
#pragma unroll
            for (int u = 0; u < WB; u++)
#pragma unroll
              for (int i = 0; i < 4; i++) x[u][i] = gptr<uint64_t>(S.dict)[d[u][i]];
          }
          for (int k = o; k < o_end; k++) {
            const PgAccOp opk = p.ops[k];
            int64_t* base = table + (size_t)k * stride;
            if (DIG && opk.is_float == PG_ACCV_LONG_DIGIT) {   // the value-kind branches are wave-uniform and stay outside the unrolled loops
              const int limb = opk.limb;
#pragma unroll
              for (int u = 0; u < WB; u++)
#pragma unroll
                for (int i = 0; i < 4; i++)
                  if ((mb >> (4 * (h + u) + i)) & 1u)
                    atomicAdd(reinterpret_cast<unsigned long long*>(base + slot[h + u][i]), (unsigned long long)long_digit((int64_t)x[u][i], limb));
            } else if (DIG && opk.is_float == PG_ACCV_FIXED_DIGIT) {
              const int q = S.fx_q, limb = opk.limb;
#pragma unroll
              for (int u = 0; u < WB; u++)
#pragma unroll
                for (int i = 0; i < 4; i++)
                  if ((mb >> (4 * (h + u) + i)) & 1u)
                    atomicAdd(reinterpret_cast<unsigned long long*>(base + slot[h + u][i]), (unsigned long long)fx_digit(__longlong_as_double((int64_t)x[u][i]), q, limb));
            } else if (S.val_type == PG_V_I64) {
#pragma unroll
              for (int u = 0; u < WB; u++)
#pragma unroll
                for (int i = 0; i < 4; i++)
                  if ((mb >> (4 * (h + u) + i)) & 1u) acc_int(base + slot[h + u][i], opk.fn, (int64_t)x[u][i]);
            } else {
#pragma unroll
              for (int u = 0; u < WB; u++)
#pragma unroll
                for (int i = 0; i < 4; i++)
                  if ((mb >> (4 * (h + u) + i)) & 1u) acc_float(base + slot[h + u][i], opk.fn, __longlong_as_double((int64_t)x[u][i]));
            }
          }
        }
      }
      o = o_end;
    }
    if (AUX && p.n_aux > 0) {   // four quads at a time: the three-stage gathers keep 16 addresses + states per lane in registers
      constexpr int AB = B < 4 ? B : 4;
#pragma unroll
      for (int h = 0; h < B; h += AB)
        aux_update_batch<AB>(p, (mb >> (4 * h)) & ((1u << (4 * AB)) - 1u), k0 + h, wtile, reinterpret_cast<const uint32_t(&)[AB][4]>(slot[h]), lane, part_lo);
    }
  }
}

#ifndef PG_FAST_AGG_B
#define PG_FAST_AGG_B 4
#endif
// LDS-table aggregation of one wave tile for the fast path: group columns of <= 8 bits, 32-bit value sources, slots
// < 65 536 (two packed per register).  B quads per lane are in flight at a time; the first source's quads are requested
// before the group columns are decoded.
template <int B>
DEVFN void fast_aggregate_wtile(const PgQueryPlan& p, uint32_t mask_all, int wtile, int64_t* __restrict__ table, int lane, uint32_t rep) {
  const uint32_t R = (uint32_t)p.replicas;
  const uint32_t stride = (uint32_t)p.n_groups * R;   // slots per op
  int o_first = 0;
  while (o_first < p.n_ops && p.ops[o_first].src < 0) o_first++;
  const bool prefetch0 = o_first < p.n_ops && p.srcs[p.ops[o_first].src].col_kind == PG_COL_RAW32;
#pragma unroll
  for (int k0 = 0; k0 < 8; k0 += B) {
    const uint32_t m = B == 8 ? mask_all : ((mask_all >> (4 * k0)) & ((1u << (4 * (B & 7))) - 1u));
    if (__ballot(m != 0) == 0) continue;   // wave-uniform
    uint32_t x[B][4];
    if (prefetch0) {
      const GAS uint8_t* tb = gptr<uint8_t>(p.srcs[p.ops[o_first].src].data + (size_t)wtile * (PG_WAVE_DOCS * 4));
#pragma unroll
      for (int k = 0; k < B; k++) {
        const uint32_t q = ((m >> (4 * k)) & 0xFu) ? (uint32_t)((k0 + k) * 64 + lane) : 0u;
        const u32x4 v = ldnt((const GAS u32x4*)(tb + q * 16u));
        x[k][0] = v.x; x[k][1] = v.y; x[k][2] = v.z; x[k][3] = v.w;
      }
    }
    uint32_t sp[B][2];   // packed slots: docs (0,1) and (2,3) of quad k
#pragma unroll
    for (int k = 0; k < B; k++) sp[k][0] = sp[k][1] = rep | (rep << 16);
    for (int g = 0; g < p.n_group_cols; g++) {
      const PgGroupCol& gc = p.gcols[g];
      const GAS uint32_t* tw = packed_wtile_base(gc.data, wtile, gc.bits);
      const uint32_t bits = (uint32_t)gc.bits, mask = (1u << gc.bits) - 1u;
      const uint32_t mult = (uint32_t)gc.mult * R;
      uint32_t r[B][2];
#pragma unroll
      for (int k = 0; k < B; k++) {
        const uint32_t q = ((m >> (4 * k)) & 0xFu) ? (uint32_t)((k0 + k) * 64 + lane) : 0u;
        load_packed_quad<true>(tw, q, bits, r[k]);
      }
#pragma unroll
      for (int k = 0; k < B; k++) {
        uint32_t d[4];
        const uint32_t q = ((m >> (4 * k)) & 0xFu) ? (uint32_t)((k0 + k) * 64 + lane) : 0u;
        decode_packed_quad<true>(r[k], q, bits, mask, d);
        sp[k][0] += __umul24(d[0], mult) + (__umul24(d[1], mult) << 16);   // dictIds < 256, mult x replicas < 65 536
        sp[k][1] += __umul24(d[2], mult) + (__umul24(d[3], mult) << 16);
      }
    }
#define PG_SLOT(k, i) ((sp[k][(i) >> 1] >> (((i) & 1) * 16)) & 0xFFFFu)
    for (int o = 0; o < p.n_ops; o++) {
      const PgAccOp op = p.ops[o];
      int64_t* base = table + (size_t)o * stride;
      if (op.src < 0) {
#pragma unroll
        for (int k = 0; k < B; k++)
#pragma unroll
          for (int i = 0; i < 4; i++)
            if ((m >> (4 * k + i)) & 1u) atomicAdd(reinterpret_cast<unsigned long long*>(base + PG_SLOT(k, i)), 1ULL);
        continue;
      }
      const bool new_src = (o == 0 || p.ops[o - 1].src != op.src);
      if (new_src) {
        const PgValueSrc& S = p.srcs[op.src];
        if (S.col_kind == PG_COL_RAW32) {
          if (!(prefetch0 && o == o_first)) {
            const GAS uint8_t* tb = gptr<uint8_t>(S.data + (size_t)wtile * (PG_WAVE_DOCS * 4));
#pragma unroll
            for (int k = 0; k < B; k++) {
              const uint32_t q = ((m >> (4 * k)) & 0xFu) ? (uint32_t)((k0 + k) * 64 + lane) : 0u;
              const u32x4 v = ldnt((const GAS u32x4*)(tb + q * 16u));
              x[k][0] = v.x; x[k][1] = v.y; x[k][2] = v.z; x[k][3] = v.w;
            }
          }
#pragma unroll
          for (int k = 0; k < B; k++)
#pragma unroll
            for (int i = 0; i < 4; i++) x[k][i] = bswap32(x[k][i]);
        } else {   // dictionary-encoded 32-bit values
          const GAS uint32_t* tw = packed_wtile_base(S.data, wtile, S.bits);
          const uint32_t bits = (uint32_t)S.bits, mask = (1u << S.bits) - 1u;
#pragma unroll
          for (int k = 0; k < B; k++) {
#pragma unroll
            for (int i = 0; i < 4; i++) x[k][i] = 0;
            if ((m >> (4 * k)) & 0xFu) {
              uint32_t r[8], d[4];
              const uint32_t q = (uint32_t)((k0 + k) * 64 + lane);
              if (bits <= 8) { load_packed_quad<true>(tw, q, bits, r); decode_packed_quad<true>(r, q, bits, mask, d); }
              else { load_packed_quad<false>(tw, q, bits, r); decode_packed_quad<false>(r, q, bits, mask, d); }
#pragma unroll
              for (int i = 0; i < 4; i++) x[k][i] = ((m >> (4 * k + i)) & 1u) ? gptr<uint32_t>(S.dict)[d[i]] : 0u;
            }
          }
        }
      }
      if (!op.is_float) {
        if (op.fn == PG_ACC_SUM) {
#pragma unroll
          for (int k = 0; k < B; k++)
#pragma unroll
            for (int i = 0; i < 4; i++)
              if ((m >> (4 * k + i)) & 1u)
                atomicAdd(reinterpret_cast<unsigned long long*>(base + PG_SLOT(k, i)), (unsigned long long)(int64_t)(int32_t)x[k][i]);
        } else if (op.fn == PG_ACC_MIN) {
#pragma unroll
          for (int k = 0; k < B; k++)
#pragma unroll
            for (int i = 0; i < 4; i++)
              if ((m >> (4 * k + i)) & 1u) atomicMin(reinterpret_cast<long long*>(base + PG_SLOT(k, i)), (long long)(int32_t)x[k][i]);
        } else {
#pragma unroll
          for (int k = 0; k < B; k++)
#pragma unroll
            for (int i = 0; i < 4; i++)
              if ((m >> (4 * k + i)) & 1u) atomicMax(reinterpret_cast<long long*>(base + PG_SLOT(k, i)), (long long)(int32_t)x[k][i]);
        }
      } else {
#pragma unroll
        for (int k = 0; k < B; k++)
#pragma unroll
          for (int i = 0; i < 4; i++)
            if ((m >> (4 * k + i)) & 1u) acc_float(base + PG_SLOT(k, i), op.fn, (double)__uint_as_float(x[k][i]));
      }
    }
#undef PG_SLOT
  }
}

// Shared epilogue: statistics and the flush of the LDS accumulator table into this workgroup's partial table.
DEVFN void flush_workgroup(const PgQueryPlan& p, const int64_t* lds_table, const uint32_t* s_stat, bool lds_agg, int t) {
  if (t < PG_MAX_STATS && s_stat[t]) atomicAdd(&p.stats[t], (unsigned long long)s_stat[t]);
  if (lds_agg) {
    const int R = p.replicas;
    const int groups = p.agg_mode == PG_AGG_LDS_PART ? p.part_groups : p.n_groups;   // this workgroup's table: [n_ops][groups]
    const int64_t n_out = (int64_t)p.n_ops * groups;
    int64_t* out = p.partials + (int64_t)blockIdx.x * n_out;
    // Many replicas per slot (no GROUP BY — a replica per lane, PG_AGG_SINGLE —, or a handful of groups): one lane per slot walking R replicas is
    // a chain of ~70-cycle LDS round trips, 30-60 us at the end of the kernel for R = 1 024.  A WAVEFRONT per slot instead: its lanes fold
    // replicas lane, lane + 64, ... and the wavefront folds the 64 partial results (integer folds commute; floating sums keep their one order).
    if (R >= 64) {
      const int lane = t & 63, wave = t >> 6;
      for (int64_t i = wave; i < n_out; i += PG_BLOCK / 64) {
        const PgAccOp op = p.ops[(int)(i / groups)];
        const int64_t* src = lds_table + i * R;
        if (op.fn == PG_ACC_SUM && op.is_float == PG_ACCV_DOUBLE) {
          if (lane == 0) {
            double d = __longlong_as_double(src[0]);
            for (int r = 1; r < R; r++) d += __longlong_as_double(src[r]);
            out[i] = __double_as_longlong(d);
          }
          continue;
        }
        int64_t acc = src[lane];
        if (op.fn == PG_ACC_COUNT || op.fn == PG_ACC_SUM) { for (int r = lane + 64; r < R; r += 64) acc += src[r]; }
        else if (op.fn == PG_ACC_MIN) { for (int r = lane + 64; r < R; r += 64) acc = src[r] < acc ? src[r] : acc; }
        else { for (int r = lane + 64; r < R; r += 64) acc = src[r] > acc ? src[r] : acc; }
        acc = wave_fold_i64(acc, op.fn);
        if (lane == 0) out[i] = acc;
      }
      return;
    }
    for (int64_t i = t; i < n_out; i += PG_BLOCK) {
      const int o = (int)(i / groups);
      const PgAccOp op = p.ops[o];
      const int64_t* src = lds_table + i * R;   // (o * G + g) * R
      int64_t acc = src[0];
      if (op.fn == PG_ACC_SUM && op.is_float == PG_ACCV_DOUBLE) {
        double d = __longlong_as_double(acc);
        for (int r = 1; r < R; r++) d += __longlong_as_double(src[r]);
        acc = __double_as_longlong(d);
      } else if (op.fn == PG_ACC_COUNT || op.fn == PG_ACC_SUM) {
        for (int r = 1; r < R; r++) acc += src[r];
      } else if (op.fn == PG_ACC_MIN) {
        for (int r = 1; r < R; r++) acc = src[r] < acc ? src[r] : acc;
      } else {
        for (int r = 1; r < R; r++) acc = src[r] > acc ? src[r] : acc;
      }
      out[i] = acc;
    }
  }
}

#endif  // PG_KERNEL_AGG_H
