// The device half of arithmetic expressions, shared by the kernels that evaluate them (pg_kernels_expr.hip: aggregations;
// pg_kernels_exprpred.hip: filter leaves; pg_kernels_exprkey.hip: keys): an operand column's value as a double, and the programs of
// pg_expr.h run one separately rounded IEEE operation at a time; a CASE's comparisons, logical operations and selects are steps of the
// same program (only the aggregations' planner hands such a program over).  Contraction is off from here to the end of the including translation unit (hipcc would fuse a * b + c into an
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
      case PG_V_DICTID: return (double)id;   // a STRING column under equals / not_equals: compared with the literal's dictId
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

// Double.compare's total order as an int64 key: -0.0 below 0.0, every NaN the one NaN above +Infinity
PG_EXPR_DEVFN long long expr_compare_key(double v) {
  const long long b = v != v ? 0x7FF8000000000000LL : __double_as_longlong(v);
  return b ^ ((b >> 63) & 0x7FFFFFFFFFFFFFFFLL);
}

// the value of expression `e` over the operands `s`: its steps in order, each one IEEE operation, comparison, logical operation or select
// (pg_expr_program.h).  Every branch of a CASE is evaluated and one value is kept: a NaN / Inf on the side not taken goes nowhere.
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
      case PG_EXPR_DIV: r = __ddiv_rn(x, y); break;
      case PG_EXPR_SELECT: {
        const int ic = st.c;
        const double z = ic < 0 ? st.lit2 : (ic < PG_EXPR_MAX_SRCS ? s[ic & 7] : t[(ic - PG_EXPR_MAX_SRCS) & 15]);
        r = x == 1.0 ? y : z;
        break;
      }
      case PG_EXPR_AND: r = x != 0.0 && y != 0.0 ? 1.0 : 0.0; break;
      case PG_EXPR_OR: r = x != 0.0 || y != 0.0 ? 1.0 : 0.0; break;
      case PG_EXPR_NOT: r = x == 0.0 ? 1.0 : 0.0; break;   // (b repeats a)
      default: {   // the six comparisons
        const long long kx = expr_compare_key(x), ky = expr_compare_key(y);
        const int op = st.op;
        const bool c = op == PG_EXPR_EQ ? kx == ky : op == PG_EXPR_NE ? kx != ky : op == PG_EXPR_GT ? kx > ky : op == PG_EXPR_GE ? kx >= ky : op == PG_EXPR_LT ? kx < ky : kx <= ky;
        r = c ? 1.0 : 0.0;
        break;
      }
    }
    t[st.dst & 15] = r;
  }
  return r;
}
