// COVAR_POP / COVAR_SAMP: the exact sums of a CovarianceTuple (shared by the kernels of pg_kernels_covar.hip, the executor
// pg_exec_covar.hip and a stand-alone CPU harness, tests/covar_main.cpp; plain C++, no HIP types).
//
// The reference (CovarianceAggregationFunction / CovarianceTuple) adds, doc by doc in docId order, x, y and the ROUNDED double product
// fl(x * y) to three doubles; every other order rounds differently.  As for SUM (pg_fixed_point.h) and the variance family (pg_moments.h)
// the GPU path does not chase that order: each of the three sums is the exact sum of its per-doc double addends, kept as integer digits,
// and rounded to double ONCE (nearest-even, +0.0 for a zero sum).  The addend of sumXY is the reference's: one separately rounded multiply
// (never an FMA, never the exact product), so a product that rounds at 53 bits, underflows to a subnormal or to 0.0 is summed as the
// double the reference sums.
//
//   Sx, Sy  as in pg_moments.h: an INT column takes one int64 slot (|x| <= 2^31, < 2^31 docs); any other column takes the digits of
//           pg_fx_digit with PG_VAR_SUM_LIMBS = 4 at the scale q1 = pg_var_q1(E), every finite |x| < 2^E.  E is the column's fx_exp
//           (FLOAT / DOUBLE: a multiple of 16 at or above its largest exponent), PG_COVAR_INT_EXP for an INT and PG_VAR_LONG_EXP for a
//           LONG column: the types' bounds — no pass over the segment looks for a tighter one.
//   Sxy     the digits of pg_fx_digit(fl(x * y)) with L = PG_COVAR_PROD_LIMBS = 5 at the scale qp = Ep - 32 L + 1, Ep = Ex + Ey:
//           |x| < 2^Ex and |y| < 2^Ey give |fl(x y)| < 2^Ep, so the integer stays below 2^(32 L - 1); a digit is below 2^32 and a segment
//           has < 2^31 docs, so no int64 limb overflows.
//
// The window of Sxy.  A product p is held exactly when it is a multiple of 2^qp; every double with |p| >= 2^(qp + 52) is one (its lowest
// mantissa bit weighs at least 2^qp), so every product within 32 L - 53 binary orders below the bound 2^Ep is exact: 75 orders for L = 4,
// 107 for L = 5, 139 for L = 6.  The bound is fixed at plan time and may sit high: each fx_exp can sit 16 above its column's top
// exponent, so 2^Ep can sit 32 orders above the largest product the segment holds.  SUM(mult(x, y)) measures its bound and keeps 75
// orders below it with four limbs (pg_fixed_point.h); to keep no fewer below the largest possible product here takes 75 + 32 = 107 orders
// below 2^Ep: L = 5, the smallest count that does.  Integer-valued products (INT and LONG columns) are always exact: qp <= 0 there
// (Ep <= 128).  A product below the window is truncated toward zero, so before the final rounding
//        |Sxy - exact| < n * 2^qp = n * 2^(Ep - 159)
// for n docs, and where the window holds every addend the result is the correctly rounded exact sum.  Underflowing products are ordinary
// addends: a subnormal is a multiple of 2^-1074 like every double, 0.0 adds nothing.
//
// Overflow.  If Ep reaches 1024 the bound cannot exclude a product that rounds to an infinity: the plan refuses (pg_covar_overflows).
#pragma once
#include <stdint.h>

#include "pg_fixed_point.h"
#include "pg_moments.h"

#define PG_COVAR_PROD_LIMBS 5
#define PG_COVAR_INT_EXP 32          // E of an INT column: |x| <= 2^31 < 2^32
#define PG_COVAR_MAX_COLS 8          // distinct argument columns of one query
#define PG_COVAR_MAX_PAIRS 8         // distinct ordered pairs of one query
#define PG_COVAR_INT_SLOTS 1         // an INT column's sum
#define PG_COVAR_DBL_SLOTS PG_VAR_SUM_LIMBS
#define PG_COVAR_MAX_SLOTS (1 + PG_COVAR_MAX_COLS * PG_COVAR_DBL_SLOTS + PG_COVAR_MAX_PAIRS * PG_COVAR_PROD_LIMBS)
#define PG_COVAR_WINDOW (32 * PG_COVAR_PROD_LIMBS - 53)   // binary orders below 2^Ep in which every product is exact

// Ep of a pair from the two columns' bounds
PG_FX_HD int pg_covar_prod_exp(int Ex, int Ey) { return Ex + Ey; }
// can a product of the pair round to an infinity, as far as the bounds tell?
PG_FX_HD int pg_covar_overflows(int Ex, int Ey) { return Ex + Ey >= 1024; }
// the scale of the product's digits
PG_FX_HD int pg_covar_qp(int Ep) { return Ep - 32 * PG_COVAR_PROD_LIMBS + 1; }
// digit `limb` of the doc's addend to Sxy; `p` is the rounded product fl(x * y), formed by the caller with ONE multiply (__dmul_rn on the
// device, a translation unit without contraction on the host)
PG_FX_HD int64_t pg_covar_prod_digit(double p, int qp, int limb) { return pg_fx_digit(p, qp, limb); }
// slots a column's sum takes in a group's row
PG_FX_HD int pg_covar_col_slots(int is_int) { return is_int ? PG_COVAR_INT_SLOTS : PG_COVAR_DBL_SLOTS; }

// ---- host finalisation ----------------------------------------------------------------------------------------------------------------------
struct pg_covar_tuple {
  double sum_x, sum_y, sum_xy;
  int64_t count;
};
// a column's sum from its slots: the integer slot, or the limbs at q1 (what SUM returns)
static inline double pg_covar_col_sum(const int64_t* s, int is_int, int E) {
  return is_int ? pg_limbs_to_double(s, 1, 0) : pg_limbs_to_double(s, PG_VAR_SUM_LIMBS, pg_var_q1(E));
}
// the tuple of one pair from a gathered row: `sx` / `sy` the columns' first slots, `sp` the pair's
static inline pg_covar_tuple pg_covar_tuple_of(int64_t count, const int64_t* sx, int x_is_int, int Ex, const int64_t* sy, int y_is_int, int Ey,
                                               const int64_t* sp, int Ep) {
  pg_covar_tuple t;
  t.count = count;
  t.sum_x = pg_covar_col_sum(sx, x_is_int, Ex);
  t.sum_y = pg_covar_col_sum(sy, y_is_int, Ey);
  t.sum_xy = pg_limbs_to_double(sp, PG_COVAR_PROD_LIMBS, pg_covar_qp(Ep));
  return t;
}
