// COVAR_POP / COVAR_SAMP on the device (CovarianceAggregationFunction under pinot-core/.../aggregation/function/, its intermediate
// CovarianceTuple(sumX, sumY, sumXY, count)).  The reference adds x, y and the rounded product fl(x * y) to three doubles in docId order;
// here every matching doc adds the exact integer digits of x, of y and of fl(x * y) (pg_covar.h) to the int64 slots of its group, and the
// host rounds each sum once (pg_exec_covar.hip).  Integer additions commute: the result does not depend on the tier, the grid or the order
// of the atomics.  One fused pass: every distinct column is loaded once per doc, however many pairs name it; the product is ONE separately
// rounded multiply (__dmul_rn; contraction is off in this translation unit, pg_expr_device.h).
//   pg_covar_reg   no GROUP BY: the row stays in registers (a digit is below 2^32 and a segment has < 2^31 docs: no int64 overflows), one
//                  reduction across the wavefront and one global atomic per slot at the end; holds one pair of two columns
//   pg_covar_reg_wide  the same body at the full limits (8 columns, 8 pairs): 186 VGPRs against 64, so only a query with more than one pair
//                  runs it
//   pg_covar_lds   up to PG_COVAR_LDS_SLOTS slots: one persistent workgroup per CU, 64-bit LDS atomics, zero digits skipped, one flush of
//                  the touched slots
//   pg_covar_hbm   beyond that: global 64-bit atomics, zero digits skipped
// All walk the filter's match words (none: every doc) with side_scan_walk of pg_side_scan.h — a plain tile loop —, which also holds
// the table tiers' skeleton, the wavefront sum and the launcher.  The column and pair descriptors are kernel arguments: wave-uniform,
// scalar branches; the register tier indexes its accumulators statically and keeps the doc's values in a vector indexed through the
// scalar pair descriptor — no scratch (the resource log of this file is checked by tests/test_gpu_covariance.py).  The table is zeroed by
// a memset and its admitted rows are gathered by pg_expr_gather (pg_kernels_expr.hip).  Kernel names are stable; the executor reports the
// tier's (pg_exec_covar.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pg_internal.hpp"
#include "pg_fixed_point.h"
#include "pg_covar.h"
#include "pg_expr_device.h"
#include "pg_side_scan.h"

#pragma clang fp contract(off)

#define DEVFN __device__ __forceinline__

namespace {

// the first NC argument columns' values at `doc`, each loaded once (wave-uniform count; the vector is indexed through the pairs' scalar indexes)
template <int NC>
DEVFN pg_d8 covar_load_all(const PgCovarArgs& a, uint32_t doc) {
  static_assert(NC <= 8 && PG_COVAR_MAX_COLS == 8, "the doc's values live in a vector of eight doubles");
  pg_d8 v = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int c = 0; c < NC; c++)
    if (c < a.n_cols) v[c] = expr_load(a.cols[c].src, doc);
  return v;
}

// the tiers with a table: `row0` is the table's first slot — the workgroup's copy in LDS, or the table in HBM
template <typename Ptr>
DEVFN void covar_update(const PgCovarArgs& a, Ptr row0, uint32_t doc) {
  const uint64_t g = pg_scan_group_key(a.scan, doc);
  if (g >= a.n_groups) return;   // (ids below their cardinalities never are)
  Ptr row = row0 + g * (uint64_t)a.slots;
  atomicAdd(reinterpret_cast<unsigned long long*>(&row[0]), 1ULL);
  // a rolled loop over the descriptors (scalar loads as they are needed: unrolled, the LDS tier runs out of scalar registers and spills to
  // scratch); the doc's values stay in a vector indexed through the scalar column index
  pg_d8 v = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll 1
  for (int c = 0; c < a.n_cols; c++) {   // wave-uniform
    const PgCovarCol& C = a.cols[c];
    const double x = expr_load(C.src, doc);
    v[c & 7] = x;
    Ptr s = row + C.first_slot;
    if (C.is_int) {
      side_sum_add(&s[0], (int64_t)x);   // exact: an INT value
    } else {
#pragma unroll
      for (int l = 0; l < PG_COVAR_DBL_SLOTS; l++) side_sum_add(&s[l], pg_fx_digit(x, C.q1, l));
    }
  }
#pragma unroll 1
  for (int p = 0; p < a.n_pairs; p++) {   // wave-uniform
    const PgCovarPair& P = a.pairs[p];
    const double prod = __dmul_rn(v[P.x & 7], v[P.y & 7]);
    Ptr s = row + P.first_slot;
#pragma unroll
    for (int l = 0; l < PG_COVAR_PROD_LIMBS; l++) side_sum_add(&s[l], pg_covar_prod_digit(prod, P.qp, l));
  }
}

extern "C" __global__ void __launch_bounds__(512) pg_covar_lds(const PgCovarArgs a) {
  side_sum_table_pass<true>(a.scan, a.n_slots, a.table, [&](int64_t* row0, uint32_t doc) PG_SIDE_INLINE { covar_update(a, row0, doc); });
}
extern "C" __global__ void __launch_bounds__(256) pg_covar_hbm(const PgCovarArgs a) {
  side_sum_table_pass<false>(a.scan, a.n_slots, a.table, [&](int64_t* row0, uint32_t doc) PG_SIDE_INLINE { covar_update(a, row0, doc); });
}

// No GROUP BY: one row.  Every lane keeps the row in registers over all its docs; one reduction across the wavefront and one global atomic
// per slot at the end.  NC / NP: the columns and pairs the instantiation holds — the accumulators are registers whether a query uses them
// or not, and the plain loop is bound by the waves in flight, so the common small query has a kernel of its own (PG_COVAR_REG_COLS /
// PG_COVAR_REG_PAIRS, pg_device.h) and only a larger one pays for the full limits.
template <int NC, int NP>
DEVFN void covar_reg_body(const PgCovarArgs& a) {
  const int lane = threadIdx.x & 63;
  int64_t sum[NC][PG_COVAR_DBL_SLOTS], prd[NP][PG_COVAR_PROD_LIMBS], count = 0;
#pragma unroll
  for (int c = 0; c < NC; c++) {
#pragma unroll
    for (int l = 0; l < PG_COVAR_DBL_SLOTS; l++) sum[c][l] = 0;
  }
#pragma unroll
  for (int p = 0; p < NP; p++) {
#pragma unroll
    for (int l = 0; l < PG_COVAR_PROD_LIMBS; l++) prd[p][l] = 0;
  }
  side_scan_walk(a.scan, [&](uint32_t doc) PG_SIDE_INLINE {
    count++;
    const pg_d8 v = covar_load_all<NC>(a, doc);
#pragma unroll
    for (int c = 0; c < NC; c++) {
      if (c < a.n_cols) {   // wave-uniform
        const PgCovarCol& C = a.cols[c];
        // the slot both kinds of column have takes its addend as a value chosen before the addition: one addition, no pointer to the accumulator
        const int64_t d0 = C.is_int ? (int64_t)v[c] : pg_fx_digit(v[c], C.q1, 0);
        sum[c][0] += d0;
        if (!C.is_int) {
#pragma unroll
          for (int l = 1; l < PG_COVAR_DBL_SLOTS; l++) sum[c][l] += pg_fx_digit(v[c], C.q1, l);
        }
      }
    }
#pragma unroll
    for (int p = 0; p < NP; p++) {
      if (p < a.n_pairs) {   // wave-uniform
        const PgCovarPair& P = a.pairs[p];
        constexpr int kMask = NC <= 2 ? 1 : (NC <= 4 ? 3 : 7);   // (the plan's indexes are below the query's columns, which this instantiation holds)
        const double prod = __dmul_rn(v[P.x & kMask], v[P.y & kMask]);
#pragma unroll
        for (int l = 0; l < PG_COVAR_PROD_LIMBS; l++) prd[p][l] += pg_covar_prod_digit(prod, P.qp, l);
      }
    }
  });
  {
    const int64_t t = wave_sum_i64(count);
    if (lane == 0 && t) atomicAdd(reinterpret_cast<unsigned long long*>(a.table), (unsigned long long)t);
  }
#pragma unroll
  for (int c = 0; c < NC; c++) {
    if (c < a.n_cols) {
      const PgCovarCol& C = a.cols[c];
#pragma unroll
      for (int l = 0; l < PG_COVAR_DBL_SLOTS; l++) {
        if (C.is_int && l >= PG_COVAR_INT_SLOTS) break;   // wave-uniform
        const int64_t t = wave_sum_i64(sum[c][l]);
        if (lane == 0 && t) atomicAdd(reinterpret_cast<unsigned long long*>(a.table + C.first_slot + l), (unsigned long long)t);
      }
    }
  }
#pragma unroll
  for (int p = 0; p < NP; p++) {
    if (p < a.n_pairs) {
      const PgCovarPair& P = a.pairs[p];
#pragma unroll
      for (int l = 0; l < PG_COVAR_PROD_LIMBS; l++) {
        const int64_t t = wave_sum_i64(prd[p][l]);
        if (lane == 0 && t) atomicAdd(reinterpret_cast<unsigned long long*>(a.table + P.first_slot + l), (unsigned long long)t);
      }
    }
  }
}

}  // namespace

extern "C" __global__ void __launch_bounds__(256) pg_covar_reg(const PgCovarArgs a) { covar_reg_body<PG_COVAR_REG_COLS, PG_COVAR_REG_PAIRS>(a); }
extern "C" __global__ void __launch_bounds__(256) pg_covar_reg_wide(const PgCovarArgs a) { covar_reg_body<PG_COVAR_MAX_COLS, PG_COVAR_MAX_PAIRS>(a); }

// ---- launcher (pg_exec_covar.hip) -------------------------------------------------------------------------------------------------------------
void pg_covar_launch_pass(const PgCovarArgs* args, int tier, int grid, hipStream_t stream) {
  const bool wide = args->n_cols > PG_COVAR_REG_COLS || args->n_pairs > PG_COVAR_REG_PAIRS;
  side_launch_pass(wide ? pg_covar_reg_wide : pg_covar_reg, pg_covar_lds, pg_covar_hbm, PG_COVAR_LDS_SLOTS * 8, *args, (size_t)args->n_slots * 8, tier, grid, stream);
}
