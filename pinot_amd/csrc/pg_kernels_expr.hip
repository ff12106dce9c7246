// Arithmetic expressions inside aggregations on the device: SUM / MIN / MAX / AVG / MINMAXRANGE over add / sub / mult / div of columns and
// literals (AdditionTransformFunction, SubtractionTransformFunction, MultiplicationTransformFunction, DivisionTransformFunction under
// pinot-core/.../operator/transform/function/).  The reference computes in IEEE double, one operation at a time, in a fixed argument order;
// the programs of pg_expr.h restate that order and every step here is one separately rounded operation — contraction is switched off for
// this translation unit (hipcc would fuse a * b + c into an FMA, which rounds once where Java rounds twice).
//   pg_expr_bounds  one pass per (segment, expression) over ALL docs: the largest finite |value| and whether a NaN / Inf occurs — the scale of
//                   the exact fixed-point SUM (pg_fixed_point.h), as the registration pass of pg_segment.cpp finds it for DOUBLE columns
//   pg_expr_reg     no GROUP BY: the accumulators stay in registers, are reduced across the wavefront and cost one global atomic per
//                   wavefront and slot at the end
//   pg_expr_lds     up to PG_EXPR_LDS_SLOTS slots: one persistent workgroup per CU, 64-bit LDS atomics, one flush of the touched slots
//   pg_expr_hbm     beyond that: global 64-bit atomics
// All three walk the filter's match words (none: every doc) with side_scan_walk of pg_side_scan.h, which also holds the table tiers'
// skeleton, the wavefront reductions and the launcher.  The program is wave-uniform (kernel arguments): its branches are scalar, the
// operands and intermediate results live in vector registers indexed through the scalar index — no scratch (the resource log of this file
// is checked by tests/test_gpu_expressions.py).  Kernel names are stable; the executor reports the tier's (pg_exec_expr.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pg_internal.hpp"
#include "pg_fixed_point.h"
#include "pg_expr_device.h"

#pragma clang fp contract(off)

#include "pg_side_scan.h"   // after the pragma: what is instantiated from it is not contracted either

#define DEVFN __device__ __forceinline__

namespace {

typedef pg_d4 d4;
typedef pg_d8 d8;

// expr_load / expr_load_all / expr_eval: pg_expr_device.h (shared with the filter leaves of pg_kernels_exprpred.hip)
DEVFN int64_t expr_order_key(double v) {   // order-preserving map double -> int64 (f64_order_key of pg_kernel_agg.h)
  const int64_t b = __double_as_longlong(v);
  return b ^ ((b >> 63) & 0x7FFFFFFFFFFFFFFFLL);
}

// the tiers with a table: `row0` is the table's first slot — the workgroup's copy in LDS, or the table in HBM
template <typename Ptr>
DEVFN void expr_update(const PgExprArgs& a, Ptr row0, uint32_t doc) {
  const uint64_t g = pg_scan_group_key(a.scan, doc);
  if (g >= a.n_groups) return;   // (ids below their cardinalities never are)
  Ptr row = row0 + g * (uint64_t)a.slots;
  const d8 s = expr_load_all(a, doc);
#pragma unroll 1
  for (int e = 0; e < a.n_exprs; e++) {   // wave-uniform
    const PgExprDesc& X = a.exprs[e];
    const double v = expr_eval(a, e, s);
    if (X.acc & PG_EXPR_ACC_SUM) {
#pragma unroll
      for (int l = 0; l < PG_EXPR_SUM_LIMBS; l++) {
        const int64_t d = pg_fx_digit(v, X.q, l);
        if (d) atomicAdd(reinterpret_cast<unsigned long long*>(&row[X.sum_slot + l]), (unsigned long long)d);
      }
    }
    if (X.acc & (PG_EXPR_ACC_MIN | PG_EXPR_ACC_MAX)) {
      const long long key = expr_order_key(v);
      if (X.acc & PG_EXPR_ACC_MIN) atomicMin(reinterpret_cast<long long*>(&row[X.min_slot]), key);
      if (X.acc & PG_EXPR_ACC_MAX) atomicMax(reinterpret_cast<long long*>(&row[X.max_slot]), key);
    }
  }
  if (a.count_slot >= 0) atomicAdd(reinterpret_cast<unsigned long long*>(&row[a.count_slot]), 1ULL);
}

template <bool LDS>
DEVFN void expr_table_body(const PgExprArgs& a) {
  side_table_pass<LDS>(
      a.scan, a.n_slots, a.table, [&](uint32_t i) PG_SIDE_INLINE { return a.ident[i % (uint32_t)a.slots]; },
      [&](int64_t* tab, uint32_t doc) PG_SIDE_INLINE { expr_update(a, tab, doc); },
      [&](uint32_t i, int64_t v) PG_SIDE_INLINE {   // only the touched slots
        const int64_t id = a.ident[i % (uint32_t)a.slots];
        if (v == id) return;
        if (id == 0) atomicAdd(reinterpret_cast<unsigned long long*>(a.table + i), (unsigned long long)v);
        else if (id > 0) atomicMin(reinterpret_cast<long long*>(a.table + i), (long long)v);
        else atomicMax(reinterpret_cast<long long*>(a.table + i), (long long)v);
      });
}

}  // namespace

extern "C" __global__ void __launch_bounds__(512) pg_expr_lds(const PgExprArgs a) { expr_table_body<true>(a); }
extern "C" __global__ void __launch_bounds__(256) pg_expr_hbm(const PgExprArgs a) { expr_table_body<false>(a); }

// No GROUP BY: one row.  Every lane keeps the row in registers over all its docs (a limb takes < 2^32 per doc and a segment has < 2^31
// docs: no int64 overflows); one reduction across the wavefront and one global atomic per slot at the end.
extern "C" __global__ void __launch_bounds__(256) pg_expr_reg(const PgExprArgs a) {
  const int lane = threadIdx.x & 63;
  int64_t sum[PG_EXPR_MAX_EXPRS][PG_EXPR_SUM_LIMBS], mn[PG_EXPR_MAX_EXPRS], mx[PG_EXPR_MAX_EXPRS], count = 0;
#pragma unroll
  for (int e = 0; e < PG_EXPR_MAX_EXPRS; e++) {
    mn[e] = INT64_MAX;
    mx[e] = INT64_MIN;
#pragma unroll
    for (int l = 0; l < PG_EXPR_SUM_LIMBS; l++) sum[e][l] = 0;
  }
  side_scan_walk(a.scan, [&](uint32_t doc) PG_SIDE_INLINE {
    const d8 s = expr_load_all(a, doc);
    count++;
    d4 vals = {0, 0, 0, 0};
#pragma unroll 1
    for (int e = 0; e < a.n_exprs; e++) vals[e & 3] = expr_eval(a, e, s);   // wave-uniform; the accumulators below are indexed statically
#pragma unroll
    for (int e = 0; e < PG_EXPR_MAX_EXPRS; e++) {
      if (e < a.n_exprs) {
        const PgExprDesc& X = a.exprs[e];
        const double v = vals[e];
        if (X.acc & PG_EXPR_ACC_SUM) {
#pragma unroll
          for (int l = 0; l < PG_EXPR_SUM_LIMBS; l++) sum[e][l] += pg_fx_digit(v, X.q, l);
        }
        const int64_t key = expr_order_key(v);
        mn[e] = key < mn[e] ? key : mn[e];
        mx[e] = key > mx[e] ? key : mx[e];
      }
    }
  });
#pragma unroll
  for (int e = 0; e < PG_EXPR_MAX_EXPRS; e++) {
    if (e < a.n_exprs) {
      const PgExprDesc& X = a.exprs[e];
      if (X.acc & PG_EXPR_ACC_SUM) {
#pragma unroll
        for (int l = 0; l < PG_EXPR_SUM_LIMBS; l++) {
          const int64_t v = wave_sum_i64(sum[e][l]);
          if (lane == 0 && v) atomicAdd(reinterpret_cast<unsigned long long*>(a.table + X.sum_slot + l), (unsigned long long)v);
        }
      }
      if (X.acc & PG_EXPR_ACC_MIN) {
        const int64_t v = wave_min_i64(mn[e]);
        if (lane == 0 && v != INT64_MAX) atomicMin(reinterpret_cast<long long*>(a.table + X.min_slot), (long long)v);
      }
      if (X.acc & PG_EXPR_ACC_MAX) {
        const int64_t v = wave_max_i64(mx[e]);
        if (lane == 0 && v != INT64_MIN) atomicMax(reinterpret_cast<long long*>(a.table + X.max_slot), (long long)v);
      }
    }
  }
  if (a.count_slot >= 0) {
    const int64_t v = wave_sum_i64(count);
    if (lane == 0 && v) atomicAdd(reinterpret_cast<unsigned long long*>(a.table + a.count_slot), (unsigned long long)v);
  }
}

// Expression 0 of `a` over ALL docs: out[0] = the bits of the largest finite |value|, out[1] = 1 when a NaN / Inf occurs
extern "C" __global__ void __launch_bounds__(256) pg_expr_bounds(const PgExprArgs a, unsigned long long* __restrict__ out) {
  unsigned long long mx = 0, bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.scan.n_docs; i += (int64_t)gridDim.x * blockDim.x) {
    const d8 s = expr_load_all(a, (uint32_t)i);
    const double v = expr_eval(a, 0, s);
    unsigned long long b = (unsigned long long)__double_as_longlong(v) & 0x7FFFFFFFFFFFFFFFULL;
    if (b >= 0x7FF0000000000000ULL) { bad = 1; b = 0; }
    mx = b > mx ? b : mx;
  }
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(mx, off, 64);
    mx = o > mx ? o : mx;
    bad |= __shfl_xor(bad, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    if (mx) atomicMax(&out[0], mx);
    if (bad) atomicOr(&out[1], 1ULL);
  }
}

// every slot of the table at its identity
extern "C" __global__ void __launch_bounds__(256) pg_expr_init(const PgExprArgs a) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n_slots; i += (uint64_t)gridDim.x * blockDim.x) a.table[i] = a.ident[i % (uint32_t)a.slots];
}

// the rows of the admitted groups, compacted: out[r][slot] = table[rows[r]][slot]
extern "C" __global__ void __launch_bounds__(256) pg_expr_gather(const int64_t* __restrict__ table, const uint32_t* __restrict__ rows, int32_t n_rows,
                                                                 int32_t slots, uint64_t n_groups, int64_t* __restrict__ out) {
  const int64_t n = (int64_t)n_rows * slots;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t g = rows[i / slots];
    if (g < n_groups) out[i] = table[g * (uint64_t)slots + (uint64_t)(i % slots)];
  }
}

// ---- launchers (pg_exec_expr.hip) -------------------------------------------------------------------------------------------------------------------
void pg_expr_launch_bounds(const PgExprArgs* args, unsigned long long* out, int grid, hipStream_t stream) {
  const PgExprArgs a = *args;
  hipLaunchKernelGGL(pg_expr_bounds, dim3(grid), dim3(256), 0, stream, a, out);
}
void pg_expr_launch_init(const PgExprArgs* args, int grid, hipStream_t stream) {
  const PgExprArgs a = *args;
  hipLaunchKernelGGL(pg_expr_init, dim3(grid), dim3(256), 0, stream, a);
}
void pg_expr_launch_pass(const PgExprArgs* args, int tier, int grid, hipStream_t stream) {
  side_launch_pass(pg_expr_reg, pg_expr_lds, pg_expr_hbm, PG_EXPR_LDS_SLOTS * 8, *args, (size_t)args->n_slots * 8, tier, grid, stream);
}
void pg_expr_launch_gather(const int64_t* table, const uint32_t* rows, int32_t n_rows, int32_t slots, uint64_t n_groups, int64_t* out, int grid, hipStream_t stream) {
  hipLaunchKernelGGL(pg_expr_gather, dim3(grid), dim3(256), 0, stream, table, rows, n_rows, slots, n_groups, out);
}
