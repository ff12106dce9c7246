// VAR_POP / VAR_SAMP / STDDEV_POP / STDDEV_SAMP on the device (VarianceAggregationFunction under pinot-core/.../aggregation/function/, its
// intermediate VarianceTuple(count, sum, m2)).  The reference updates m2 doc by doc in docId order; here every matching doc adds the exact
// integer digits of x and of x^2 (pg_moments.h) to the int64 slots of its group, and the host forms m2 = sum x^2 - (sum x)^2 / n in exact
// integer arithmetic, rounded once (pg_exec_var.hip).  Integer additions commute: the result does not depend on the tier, the grid or the
// order of the atomics.
//   pg_var_reg   no GROUP BY: the row stays in registers (a digit is below 2^32 and a segment has < 2^31 docs: no int64 overflows), one
//                reduction across the wavefront and one global atomic per slot at the end
//   pg_var_lds   up to PG_VAR_LDS_SLOTS slots: one persistent workgroup per CU, 64-bit LDS atomics, zero digits skipped, one flush of the
//                touched slots
//   pg_var_hbm   beyond that: global 64-bit atomics
// All three walk the filter's match words (none: every doc) with side_scan_walk of pg_side_scan.h, which also holds the table tiers'
// skeleton, the wavefront sum and the launcher.  The columns and their type split (integer path or digits of a double) are kernel
// arguments: wave-uniform, scalar branches; the register tier indexes its accumulators statically — no scratch (the resource log of this
// file is checked by tests/test_gpu_variance.py).  The table is zeroed by a memset and its admitted rows are gathered by pg_expr_gather
// (pg_kernels_expr.hip).  Kernel names are stable; the executor reports the tier's (pg_exec_var.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pg_internal.hpp"
#include "pg_fixed_point.h"
#include "pg_moments.h"
#include "pg_expr_device.h"
#include "pg_side_scan.h"

#define DEVFN __device__ __forceinline__

namespace {

// the tiers with a table: `row0` is the table's first slot — the workgroup's copy in LDS, or the table in HBM
template <typename Ptr>
DEVFN void var_update(const PgVarArgs& a, Ptr row0, uint32_t doc) {
  const uint64_t g = pg_scan_group_key(a.scan, doc);
  if (g >= a.n_groups) return;   // (ids below their cardinalities never are)
  Ptr row = row0 + g * (uint64_t)a.slots;
  atomicAdd(reinterpret_cast<unsigned long long*>(&row[0]), 1ULL);
#pragma unroll 1
  for (int c = 0; c < a.n_cols; c++) {   // wave-uniform
    const PgVarCol& C = a.cols[c];
    Ptr s = row + C.first_slot;
    if (C.is_int) {
      const int64_t x = side_load_int(C.src, doc);
      const int64_t sq = x * x;   // <= 2^62
      side_sum_add(&s[0], x);
      side_sum_add(&s[1], pg_long_digit(sq, 0));
      side_sum_add(&s[2], pg_long_digit(sq, 1));
    } else {
      const double v = expr_load(C.src, doc);
#pragma unroll
      for (int l = 0; l < PG_VAR_SUM_LIMBS; l++) side_sum_add(&s[l], pg_fx_digit(v, C.q1, l));
#pragma unroll
      for (int l = 0; l < PG_VAR_SQ_LIMBS; l++) side_sum_add(&s[PG_VAR_SUM_LIMBS + l], (int64_t)pg_sq_digit(v, C.q2, l));
    }
  }
}

}  // namespace

extern "C" __global__ void __launch_bounds__(512) pg_var_lds(const PgVarArgs a) {
  side_sum_table_pass<true>(a.scan, a.n_slots, a.table, [&](int64_t* row0, uint32_t doc) PG_SIDE_INLINE { var_update(a, row0, doc); });
}
extern "C" __global__ void __launch_bounds__(256) pg_var_hbm(const PgVarArgs a) {
  side_sum_table_pass<false>(a.scan, a.n_slots, a.table, [&](int64_t* row0, uint32_t doc) PG_SIDE_INLINE { var_update(a, row0, doc); });
}

// No GROUP BY: one row.  Every lane keeps the row in registers over all its docs; one reduction across the wavefront and one global atomic
// per slot at the end.
extern "C" __global__ void __launch_bounds__(256) pg_var_reg(const PgVarArgs a) {
  const int lane = threadIdx.x & 63;
  int64_t acc[PG_VAR_MAX_COLS][PG_VAR_DBL_SLOTS], count = 0;
#pragma unroll
  for (int c = 0; c < PG_VAR_MAX_COLS; c++) {
#pragma unroll
    for (int l = 0; l < PG_VAR_DBL_SLOTS; l++) acc[c][l] = 0;
  }
  side_scan_walk(a.scan, [&](uint32_t doc) PG_SIDE_INLINE {
    count++;
#pragma unroll
    for (int c = 0; c < PG_VAR_MAX_COLS; c++) {
      if (c < a.n_cols) {   // wave-uniform
        const PgVarCol& C = a.cols[c];
        // What the doc adds to the slots both paths have is added after the branch that tells the paths apart, as values: additions at
        // the end of both of its arms would be merged into one through a pointer, and the accumulator behind it would leave its register
        // (seen as scratch in the resource log).
        static_assert(PG_VAR_INT_SLOTS <= PG_VAR_SUM_LIMBS, "the double path's first digits are digits of the sum");
        int64_t d[PG_VAR_INT_SLOTS];
        if (C.is_int) {
          const int64_t x = side_load_int(C.src, doc);
          const int64_t sq = x * x;
          d[0] = x;
          d[1] = pg_long_digit(sq, 0);
          d[2] = pg_long_digit(sq, 1);
        } else {
          const double v = expr_load(C.src, doc);
#pragma unroll
          for (int l = 0; l < PG_VAR_INT_SLOTS; l++) d[l] = pg_fx_digit(v, C.q1, l);
#pragma unroll
          for (int l = PG_VAR_INT_SLOTS; l < PG_VAR_SUM_LIMBS; l++) acc[c][l] += pg_fx_digit(v, C.q1, l);
#pragma unroll
          for (int l = 0; l < PG_VAR_SQ_LIMBS; l++) acc[c][PG_VAR_SUM_LIMBS + l] += (int64_t)pg_sq_digit(v, C.q2, l);
        }
#pragma unroll
        for (int l = 0; l < PG_VAR_INT_SLOTS; l++) acc[c][l] += d[l];
      }
    }
  });
  {
    const int64_t v = wave_sum_i64(count);
    if (lane == 0 && v) atomicAdd(reinterpret_cast<unsigned long long*>(a.table), (unsigned long long)v);
  }
#pragma unroll
  for (int c = 0; c < PG_VAR_MAX_COLS; c++) {
    if (c < a.n_cols) {
      const PgVarCol& C = a.cols[c];
#pragma unroll
      for (int l = 0; l < PG_VAR_DBL_SLOTS; l++) {
        if (C.is_int && l >= PG_VAR_INT_SLOTS) break;   // wave-uniform
        const int64_t v = wave_sum_i64(acc[c][l]);
        if (lane == 0 && v) atomicAdd(reinterpret_cast<unsigned long long*>(a.table + C.first_slot + l), (unsigned long long)v);
      }
    }
  }
}

// ---- launcher (pg_exec_var.hip) ---------------------------------------------------------------------------------------------------------------
void pg_var_launch_pass(const PgVarArgs* args, int tier, int grid, hipStream_t stream) {
  side_launch_pass(pg_var_reg, pg_var_lds, pg_var_hbm, PG_VAR_LDS_SLOTS * 8, *args, (size_t)args->n_slots * 8, tier, grid, stream);
}
