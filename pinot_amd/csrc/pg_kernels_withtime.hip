// FIRSTWITHTIME / LASTWITHTIME on the device (FirstWithTimeAggregationFunction / LastWithTimeAggregationFunction under
// pinot-core/.../aggregation/function/, their intermediate ValueLongPair(value, time)).  The reference walks the matching docs in docId order
// and keeps the pair of the last doc with time >= best (LAST) / time <= best (FIRST): the greatest docId among the docs at the extreme time.
// Here that winner is the maximum of one unsigned order (pg_with_time.h): every matching doc issues ONE 64-bit atomic max per slot — a
// distinct (time column, direction) of the query — of the packed (time, doc), or in wide mode of the time's order key (pass 0) and then, where
// its key equals the slot's maximum, of doc + 1 (pass 1).  A maximum does not depend on the tier, the grid or the order of the atomics.
//   pg_wt_reg    no GROUP BY: the best key per slot stays in registers per lane, one maximum across the wavefront and one global atomic per
//                slot at the end
//   pg_wt_lds    up to PG_WT_LDS_SLOTS slots: persistent workgroups — as many per CU as their tables fit its LDS, four at the most —, 64-bit
//                LDS atomic max, one flush of the non-empty slots
//   pg_wt_hbm    beyond that: global 64-bit atomic max
//   pg_wt_gather per admitted row the winner doc of every slot, its time and the value columns read at it
// All three passes walk the filter's match words (none: every doc) with side_scan_walk of pg_side_scan.h, which also holds the table tiers'
// skeleton, the wavefront maximum and the launcher.  The time columns' kinds and the slots' modes are kernel arguments: wave-uniform, scalar
// branches; the register tier indexes its keys statically — no scratch (the resource log of this file is checked by
// tests/test_gpu_with_time.py).  Both planes are zeroed by a memset.  Kernel names are stable; the executor reports the tier's
// (pg_exec_withtime.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pg_internal.hpp"
#include "pg_with_time.h"
#include "pg_side_scan.h"

#define DEVFN __device__ __forceinline__

namespace {

// a time column's value as getLongValuesSV gives it: INT sign-extended, LONG as it is; raw big-endian, or through the dictionary
DEVFN int64_t wt_load_time(const PgValueSrc& S, uint32_t doc) {
  if (S.col_kind == PG_COL_FIXED_BIT) {   // wave-uniform
    const uint32_t id = pg_fixed_bit_id(S.data, S.bits, doc);
    return S.val_type == PG_V_I32 ? (int64_t)reinterpret_cast<const int32_t*>(S.dict)[id] : (int64_t)reinterpret_cast<const long long*>(S.dict)[id];
  }
  if (S.col_kind == PG_COL_RAW32) return (int64_t)(int32_t)__builtin_bswap32(reinterpret_cast<const uint32_t*>(S.data)[doc]);
  return (int64_t)__builtin_bswap64(reinterpret_cast<const unsigned long long*>(S.data)[doc]);
}

// a value column's 64 bits: INT sign-extended, LONG as it is, FLOAT / DOUBLE the raw IEEE bits (a FLOAT's 32 zero-extended)
DEVFN int64_t wt_load_value(const PgValueSrc& S, uint32_t doc) {
  if (S.col_kind == PG_COL_FIXED_BIT) {
    const uint32_t id = pg_fixed_bit_id(S.data, S.bits, doc);
    switch (S.val_type) {
      case PG_V_I32: return (int64_t)reinterpret_cast<const int32_t*>(S.dict)[id];
      case PG_V_F32: return (int64_t)(uint64_t)reinterpret_cast<const uint32_t*>(S.dict)[id];
      default: return (int64_t)reinterpret_cast<const long long*>(S.dict)[id];   // LONG, or a DOUBLE's bits
    }
  }
  if (S.col_kind == PG_COL_RAW32) {
    const uint32_t u = __builtin_bswap32(reinterpret_cast<const uint32_t*>(S.data)[doc]);
    return S.val_type == PG_V_F32 ? (int64_t)(uint64_t)u : (int64_t)(int32_t)u;
  }
  return (int64_t)__builtin_bswap64(reinterpret_cast<const unsigned long long*>(S.data)[doc]);
}

// what `doc` offers a slot in this pass: the packed (time, doc) or the wide order key (pass 0; a wide key of 0 needs no atomic, the zeroed
// plane already holds it), doc + 1 where its wide key is the slot's maximum `best` and else 0, nothing (pass 1)
DEVFN unsigned long long wt_offer(const PgWtArgs& a, const PgWtSlot& S, uint32_t doc, unsigned long long best) {
  const int64_t t = wt_load_time(S.time, doc);
  if (a.pass == 0) return S.packed ? pg_wt_pack(pg_wt_rel(t, S.base, S.first), doc, a.doc_bits) : pg_wt_order_key(t, S.first);
  return pg_wt_order_key(t, S.first) == best ? (unsigned long long)doc + 1ULL : 0ULL;
}

// the tiers with a table: `tab` is the plane of this pass — the workgroup's copy in LDS, or the plane in HBM
template <typename Ptr>
DEVFN void wt_update(const PgWtArgs& a, Ptr tab, uint32_t doc) {
  const uint64_t g = pg_scan_group_key(a.scan, doc);
  if (g >= a.n_groups) return;   // (ids below their cardinalities never are)
  const uint64_t row = g * (uint64_t)a.slots;
#pragma unroll 1
  for (int s = 0; s < a.slots; s++) {   // wave-uniform
    const PgWtSlot& S = a.slot[s];
    if (a.pass == 1 && S.packed) continue;
    const unsigned long long best = a.pass == 1 ? a.keys[row + s] : 0ULL;
    const unsigned long long v = wt_offer(a, S, doc, best);
    if (v) atomicMax(&tab[row + s], v);
  }
}

template <bool LDS>
DEVFN void wt_table_body(const PgWtArgs& a) {
  unsigned long long* plane = a.pass == 0 ? a.keys : a.docs;
  side_table_pass<LDS>(
      a.scan, a.n_slots, plane, [](uint32_t) PG_SIDE_INLINE { return 0ULL; }, [&](unsigned long long* tab, uint32_t doc) PG_SIDE_INLINE { wt_update(a, tab, doc); },
      [&](uint32_t i, unsigned long long v) PG_SIDE_INLINE {   // only the non-empty slots
        if (v) atomicMax(&plane[i], v);
      });
}

}  // namespace

extern "C" __global__ void __launch_bounds__(512) pg_wt_lds(const PgWtArgs a) { wt_table_body<true>(a); }
extern "C" __global__ void __launch_bounds__(256) pg_wt_hbm(const PgWtArgs a) { wt_table_body<false>(a); }

// No GROUP BY: one row.  Every lane keeps the best offer per slot in registers over all its docs; one maximum across the wavefront and one
// global atomic per slot at the end.
extern "C" __global__ void __launch_bounds__(256) pg_wt_reg(const PgWtArgs a) {
  const int lane = threadIdx.x & 63;
  unsigned long long* plane = a.pass == 0 ? a.keys : a.docs;
  unsigned long long best[PG_WT_MAX_SLOTS], top[PG_WT_MAX_SLOTS];
#pragma unroll
  for (int s = 0; s < PG_WT_MAX_SLOTS; s++) {
    best[s] = 0;
    top[s] = (a.pass == 1 && s < a.slots) ? a.keys[s] : 0ULL;   // wave-uniform
  }
  side_scan_walk(a.scan, [&](uint32_t doc) PG_SIDE_INLINE {
#pragma unroll
    for (int s = 0; s < PG_WT_MAX_SLOTS; s++) {
      if (s < a.slots && !(a.pass == 1 && a.slot[s].packed)) {   // wave-uniform
        const unsigned long long v = wt_offer(a, a.slot[s], doc, top[s]);
        best[s] = v > best[s] ? v : best[s];
      }
    }
  });
#pragma unroll
  for (int s = 0; s < PG_WT_MAX_SLOTS; s++) {
    if (s < a.slots && !(a.pass == 1 && a.slot[s].packed)) {
      const unsigned long long v = wave_max_u64(best[s]);
      if (lane == 0 && v) atomicMax(&plane[s], v);
    }
  }
}

// The admitted rows: per row and slot the winner doc and its time, per row and aggregation the value at the winner doc of its slot.  A slot
// without a doc gives doc -1; a doc at or beyond n_docs is reported as it is and nothing is read at it (the host fails on either).
extern "C" __global__ void __launch_bounds__(256) pg_wt_gather(const PgWtGatherArgs a) {
  const int32_t per_row = a.slots + a.n_aggs;
  const int64_t n = (int64_t)a.n_rows * per_row;
  const int32_t width = 2 * a.slots + a.n_aggs;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int32_t r = (int32_t)(i / per_row), j = (int32_t)(i % per_row);
    const int32_t s = j < a.slots ? j : a.value_slot[j - a.slots];
    const uint64_t at = (uint64_t)a.rows[r] * (uint64_t)a.slots + (uint64_t)s;
    int64_t doc = -1;
    if (a.slot[s].packed) {
      const unsigned long long v = a.keys[at];
      if (v) doc = (int64_t)pg_wt_packed_doc(v, a.doc_bits);
    } else {
      const unsigned long long d = a.docs[at];
      if (d) doc = (int64_t)(d - 1ULL);
    }
    const bool readable = doc >= 0 && doc < a.n_docs;
    int64_t* out = a.out + (int64_t)r * width;
    if (j < a.slots) {
      out[2 * j] = doc;
      out[2 * j + 1] = readable ? wt_load_time(a.slot[s].time, (uint32_t)doc) : 0;
    } else {
      out[2 * a.slots + (j - a.slots)] = readable ? wt_load_value(a.value[j - a.slots], (uint32_t)doc) : 0;
    }
  }
}

// ---- launchers (pg_exec_withtime.hip) -----------------------------------------------------------------------------------------------------------
void pg_wt_launch_pass(const PgWtArgs* args, int tier, int grid, hipStream_t stream) {
  side_launch_pass(pg_wt_reg, pg_wt_lds, pg_wt_hbm, PG_WT_LDS_SLOTS * 8, *args, (size_t)args->n_slots * 8, tier, grid, stream);
}
void pg_wt_launch_gather(const PgWtGatherArgs* args, int grid, hipStream_t stream) {
  const PgWtGatherArgs a = *args;
  hipLaunchKernelGGL(pg_wt_gather, dim3(grid), dim3(256), 0, stream, a);
}
