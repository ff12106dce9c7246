// SKEWNESS / KURTOSIS on the device (FourthMomentAggregationFunction under pinot-core/.../aggregation/function/, its intermediate
// PinotFourthMoment(n, m1, m2, m3, m4)).  The reference updates the mean and the central sums doc by doc in docId order; here every matching
// doc adds the exact integer digits of x, x^2, x^3 and x^4 (pg_moment4.h) to the int64 slots of its group, and the host forms the central
// moments in exact integer arithmetic, each rounded once (pg_exec_moment.hip).  Integer additions commute: the result does not depend on the
// tier, the grid or the order of the atomics.
//   pg_moment_reg   no GROUP BY: the row stays in registers (a digit is below 2^32 and a segment has < 2^31 docs: no int64 overflows), one
//                   reduction across the wavefront and one global atomic per slot at the end
//   pg_moment_lds   up to PG_MOMENT_LDS_SLOTS slots: one persistent workgroup per CU, 64-bit LDS atomics, zero digits skipped, one flush of
//                   the touched slots
//   pg_moment_hbm   beyond that: global 64-bit atomics
// All three walk the filter's match words (none: every doc) with side_scan_walk of pg_side_scan.h, which also holds the table tiers'
// skeleton, the wavefront sum and the launcher.  The columns and their type split (integer path or digits of a double) are kernel
// arguments: wave-uniform, scalar branches.  The powers of a double are formed once per doc (pg_m4_powers_of: seven 64 x 64 -> 128
// multiplies) and their words are picked by comparisons, never by an address; the register tier indexes its accumulators statically — no
// scratch (the resource log of this file is checked by tests/test_gpu_moments.py).  The table is zeroed by a memset and its admitted rows are
// gathered by pg_expr_gather (pg_kernels_expr.hip).  Kernel names are stable; the executor reports the tier's (pg_exec_moment.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pg_internal.hpp"
#include "pg_fixed_point.h"
#include "pg_moments.h"
#include "pg_moment4.h"
#include "pg_expr_device.h"
#include "pg_side_scan.h"

#define DEVFN __device__ __forceinline__

namespace {

constexpr int kSq = PG_VAR_SUM_LIMBS, kCube = kSq + PG_VAR_SQ_LIMBS, kQuad = kCube + PG_M4_CUBE_LIMBS;   // where the double path's sums start

// the tiers with a table: `row0` is the table's first slot — the workgroup's copy in LDS, or the table in HBM
template <typename Ptr>
DEVFN void moment_update(const PgMomentArgs& a, Ptr row0, uint32_t doc) {
  const uint64_t g = pg_scan_group_key(a.scan, doc);
  if (g >= a.n_groups) return;   // (ids below their cardinalities never are)
  Ptr row = row0 + g * (uint64_t)a.slots;
  atomicAdd(reinterpret_cast<unsigned long long*>(&row[0]), 1ULL);
#pragma unroll 1
  for (int c = 0; c < a.n_cols; c++) {   // wave-uniform
    const PgMomentCol& C = a.cols[c];
    Ptr s = row + C.first_slot;
    if (C.is_int) {
      int64_t d[PG_M4_INT_SLOTS];
      pg_m4_int_digits(side_load_int(C.src, doc), d);
#pragma unroll
      for (int l = 0; l < PG_M4_INT_SLOTS; l++) side_sum_add(&s[l], d[l]);
    } else {
      const double v = expr_load(C.src, doc);
      const pg_m4_powers P = pg_m4_powers_of(v);
#pragma unroll
      for (int l = 0; l < PG_VAR_SUM_LIMBS; l++) side_sum_add(&s[l], pg_fx_digit(v, C.q1, l));
#pragma unroll
      for (int l = 0; l < PG_VAR_SQ_LIMBS; l++) side_sum_add(&s[kSq + l], (int64_t)pg_sq_digit(v, C.q2, l));
#pragma unroll
      for (int l = 0; l < PG_M4_CUBE_LIMBS; l++) side_sum_add(&s[kCube + l], pg_m4_cube_digit(P, C.q3, l));
#pragma unroll
      for (int l = 0; l < PG_M4_QUAD_LIMBS; l++) side_sum_add(&s[kQuad + l], pg_m4_quad_digit(P, C.q4, l));
    }
  }
}

}  // namespace

extern "C" __global__ void __launch_bounds__(512) pg_moment_lds(const PgMomentArgs a) {
  side_sum_table_pass<true>(a.scan, a.n_slots, a.table, [&](int64_t* row0, uint32_t doc) PG_SIDE_INLINE { moment_update(a, row0, doc); });
}
extern "C" __global__ void __launch_bounds__(256) pg_moment_hbm(const PgMomentArgs a) {
  side_sum_table_pass<false>(a.scan, a.n_slots, a.table, [&](int64_t* row0, uint32_t doc) PG_SIDE_INLINE { moment_update(a, row0, doc); });
}

// No GROUP BY: one row.  Every lane keeps the row in registers over all its docs; one reduction across the wavefront and one global atomic
// per slot at the end.
extern "C" __global__ void __launch_bounds__(256) pg_moment_reg(const PgMomentArgs a) {
  const int lane = threadIdx.x & 63;
  int64_t acc[PG_MOMENT_MAX_COLS][PG_M4_DBL_SLOTS], count = 0;
#pragma unroll
  for (int c = 0; c < PG_MOMENT_MAX_COLS; c++) {
#pragma unroll
    for (int l = 0; l < PG_M4_DBL_SLOTS; l++) acc[c][l] = 0;
  }
  side_scan_walk(a.scan, [&](uint32_t doc) PG_SIDE_INLINE {
    count++;
#pragma unroll
    for (int c = 0; c < PG_MOMENT_MAX_COLS; c++) {
      if (c < a.n_cols) {   // wave-uniform
        const PgMomentCol& C = a.cols[c];
        // What the doc adds to the slots both paths have is added after the branch that tells the paths apart, as values (see pg_var_reg:
        // additions at the end of both arms would be merged into one through a pointer, and the accumulator would leave its register).
        static_assert(PG_M4_INT_SLOTS == PG_VAR_SUM_LIMBS + PG_VAR_SQ_LIMBS, "the integer path's slots are the double path's digits of x and x^2");
        int64_t d[PG_M4_INT_SLOTS];
        if (C.is_int) {
          pg_m4_int_digits(side_load_int(C.src, doc), d);
        } else {
          const double v = expr_load(C.src, doc);
          const pg_m4_powers P = pg_m4_powers_of(v);
#pragma unroll
          for (int l = 0; l < PG_VAR_SUM_LIMBS; l++) d[l] = pg_fx_digit(v, C.q1, l);
#pragma unroll
          for (int l = 0; l < PG_VAR_SQ_LIMBS; l++) d[kSq + l] = (int64_t)pg_sq_digit(v, C.q2, l);
#pragma unroll
          for (int l = 0; l < PG_M4_CUBE_LIMBS; l++) acc[c][kCube + l] += pg_m4_cube_digit(P, C.q3, l);
#pragma unroll
          for (int l = 0; l < PG_M4_QUAD_LIMBS; l++) acc[c][kQuad + l] += pg_m4_quad_digit(P, C.q4, l);
        }
#pragma unroll
        for (int l = 0; l < PG_M4_INT_SLOTS; l++) acc[c][l] += d[l];
      }
    }
  });
  {
    const int64_t v = wave_sum_i64(count);
    if (lane == 0 && v) atomicAdd(reinterpret_cast<unsigned long long*>(a.table), (unsigned long long)v);
  }
#pragma unroll
  for (int c = 0; c < PG_MOMENT_MAX_COLS; c++) {
    if (c < a.n_cols) {
      const PgMomentCol& C = a.cols[c];
#pragma unroll
      for (int l = 0; l < PG_M4_DBL_SLOTS; l++) {
        if (C.is_int && l >= PG_M4_INT_SLOTS) break;   // wave-uniform
        const int64_t v = wave_sum_i64(acc[c][l]);
        if (lane == 0 && v) atomicAdd(reinterpret_cast<unsigned long long*>(a.table + C.first_slot + l), (unsigned long long)v);
      }
    }
  }
}

// ---- launcher (pg_exec_moment.hip) ------------------------------------------------------------------------------------------------------------
void pg_moment_launch_pass(const PgMomentArgs* args, int tier, int grid, hipStream_t stream) {
  side_launch_pass(pg_moment_reg, pg_moment_lds, pg_moment_hbm, PG_MOMENT_LDS_SLOTS * 8, *args, (size_t)args->n_slots * 8, tier, grid, stream);
}
