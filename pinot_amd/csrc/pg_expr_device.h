// The device half of arithmetic expressions, shared by the kernels that evaluate them (pg_kernels_expr.hip: aggregations;
// pg_kernels_exprpred.hip: filter leaves): an operand column's value as a double, and the programs of pg_expr.h run one separately rounded
// IEEE operation at a time.  Contraction is off from here to the end of the including translation unit (hipcc would fuse a * b + c into an
// FMA, which rounds once where Java rounds twice).  The program is wave-uniform (kernel arguments): its branches are scalar, the operands
// and intermediate results live in vector registers indexed through the scalar index — no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pg_device.h"

#pragma clang fp contract(off)

#define PG_EXPR_DEVFN static __device__ __forceinline__

typedef double pg_d4 __attribute__((ext_vector_type(4)));
typedef double pg_d8 __attribute__((ext_vector_type(8)));
typedef double pg_d16 __attribute__((ext_vector_type(16)));

// the operand's value as the reference's getDoubleValuesSV gives it: INT exact, LONG (double) round-to-nearest, FLOAT widened exactly
PG_EXPR_DEVFN double expr_load(const PgValueSrc& S, uint32_t doc) {
  if (S.col_kind == PG_COL_FIXED_BIT) {   // wave-uniform
    const uint32_t id = pg_fixed_bit_id(S.data, S.bits, doc);
    switch (S.val_type) {
      case PG_V_I32: return (double)reinterpret_cast<const int32_t*>(S.dict)[id];
      case PG_V_I64: return __ll2double_rn(reinterpret_cast<const long long*>(S.dict)[id]);
      case PG_V_F32: return (double)reinterpret_cast<const float*>(S.dict)[id];
      default: return reinterpret_cast<const double*>(S.dict)[id];
    }
  }
  if (S.col_kind == PG_COL_RAW32) {
    const uint32_t u = __builtin_bswap32(reinterpret_cast<const uint32_t*>(S.data)[doc]);
    return S.val_type == PG_V_F32 ? (double)__uint_as_float(u) : (double)(int32_t)u;
  }
  const unsigned long long u = __builtin_bswap64(reinterpret_cast<const unsigned long long*>(S.data)[doc]);
  return S.val_type == PG_V_F64 ? __longlong_as_double((long long)u) : __ll2double_rn((long long)u);
}

PG_EXPR_DEVFN pg_d8 expr_load_all(const PgExprArgs& a, uint32_t doc) {
  pg_d8 s = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < PG_EXPR_MAX_SRCS; i++)
    if (i < a.n_srcs) s[i] = expr_load(a.srcs[i], doc);
  return s;
}

// the value of expression `e` over the operands `s`: its steps in order, each one IEEE operation
PG_EXPR_DEVFN double expr_eval(const PgExprArgs& a, int e, const pg_d8& s) {
  const PgExprDesc& X = a.exprs[e];
  pg_d16 t = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  double r = 0.0;
  for (int k = 0; k < X.n_steps; k++) {   // wave-uniform
    const pg_expr_step& st = a.steps[X.first_step + k];
    const int ia = st.a, ib = st.b;
    const double x = ia < 0 ? st.lit : (ia < PG_EXPR_MAX_SRCS ? s[ia & 7] : t[(ia - PG_EXPR_MAX_SRCS) & 15]);
    const double y = ib < 0 ? st.lit : (ib < PG_EXPR_MAX_SRCS ? s[ib & 7] : t[(ib - PG_EXPR_MAX_SRCS) & 15]);
    switch (st.op) {
      case PG_EXPR_ADD: r = __dadd_rn(x, y); break;
      case PG_EXPR_SUB: r = __dsub_rn(x, y); break;
      case PG_EXPR_MULT: r = __dmul_rn(x, y); break;
      default: r = __ddiv_rn(x, y); break;
    }
    t[st.dst & 15] = r;
  }
  return r;
}
