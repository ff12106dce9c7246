// Exact second moments (VAR_POP / VAR_SAMP / STDDEV_POP / STDDEV_SAMP; shared by the kernels of pg_kernels_var.hip, the executor and a
// stand-alone CPU harness, tests/moments_main.cpp; plain C++, no HIP types).
//
// The reference (VarianceAggregationFunction / VarianceTuple) updates m2 doc by doc in docId order; every other order rounds differently.
// As for SUM (pg_fixed_point.h) the GPU path does not chase that order: it accumulates the power sums  Sx = sum x  and  Sq = sum x^2  EXACTLY
// as integers and forms  m2 = Sq - Sx^2 / n  in exact integer arithmetic on the host, rounding to double ONCE (nearest-even).
//
//   Sx   the digits of pg_fx_digit with L = PG_VAR_SUM_LIMBS = 4 at the scale q1 = E - 127, every finite |x| < 2^E.
//   Sq   x = m * 2^ex with the 53-bit mantissa m; M = m * m is formed exactly from a 64 x 64 -> 128 multiply; digit j (base 2^32) of
//        trunc(M * 2^(2 ex - q2)) with q2 = 2 E - 32 L2 + 1 goes into limb j.  No FMA, no double-double, no overflow or underflow case:
//        every finite double has an exact 106-bit square.  x^2 < 2^(2 E), so the integer stays below 2^(32 L2 - 1); a digit is below 2^32
//        and a segment has < 2^31 docs, so no int64 limb overflows.
//   L2 = PG_VAR_SQ_LIMBS = 6 (192 bits).  A value with |x| >= 2^(E - s - 1) has ex >= E - s - 53, so its square is held exactly when
//        2 s <= 32 L2 - 107: s <= 10 for L2 = 4, s <= 42 for 6, s <= 74 for 8 (where it meets the window of Sx).  E is a multiple of 16 at or
//        above the largest exponent (pg_segment.cpp), which alone can cost s = 16; L2 = 4 would then truncate columns that span a factor of
//        a thousand.  L2 = 6 keeps every column exact whose magnitudes span up to 2^26, eight decimal orders, at 1 + 4 + 6 = 11 slots per
//        group and column (1 489 groups in the LDS tier instead of 1 820 for L2 = 4); a square has at most five non-zero digits whatever
//        L2 is, so the atomics per doc do not grow with it.
//   INT  columns (raw or through an INT dictionary) take an integer path: Sx in one int64 slot (|x| <= 2^31, < 2^31 docs), x^2 (<= 2^62)
//        as two pg_long_digit digits.
//   LONG columns are read as the reference's getDoubleValuesSV reads them ((double) rounded first) and take the double path with E = 64:
//        integers are always exact (x^2 <= 2^126 and q2 < 0).
//
// Values below the window are truncated toward zero, so before the final rounding
//        |m2 - exact| < n * (2^q2 + 2^(E + q1 + 1))
// (0 <= sum x^2 - Sq < n 2^q2;  |sum x - Sx| < n 2^q1 and |sum x + Sx| < 2 n 2^E, so Sx^2 / n is off by less than n 2^(E + q1 + 1)).
// Where the window holds every digit the result is the correctly rounded true value.  m2 is 0.0 for n = 1, never negative, never -0.0
// (a difference that truncation made negative is clamped, which only moves it towards the true value).
#pragma once
#include <stdint.h>

#include "pg_fixed_point.h"

#define PG_VAR_SUM_LIMBS 4
#define PG_VAR_SQ_LIMBS 6
#define PG_VAR_INT_SLOTS 3                                       // integer path: Sx, two digits of Sq
#define PG_VAR_DBL_SLOTS (PG_VAR_SUM_LIMBS + PG_VAR_SQ_LIMBS)   // double path
#define PG_VAR_LONG_EXP 64                                       // E of a LONG column: |(double)x| <= 2^63

PG_FX_HD int pg_var_q1(int E) { return E - (32 * PG_VAR_SUM_LIMBS - 1); }
PG_FX_HD int pg_var_q2(int E) { return 2 * E - 32 * PG_VAR_SQ_LIMBS + 1; }

// digit `limb` (base 2^32) of trunc(x^2 * 2^-q2); x finite
PG_FX_HD uint32_t pg_sq_digit(double x, int q2, int limb) {
  uint64_t b;
  __builtin_memcpy(&b, &x, 8);
  const int e = (int)((b >> 52) & 0x7FFu);
  uint64_t m = b & 0xFFFFFFFFFFFFFULL;
  int ex = -1074;                       // |x| = m * 2^ex with a 53-bit m
  if (e) { m |= 1ULL << 52; ex = e - 1075; }
#if defined(__HIP_DEVICE_COMPILE__)
  const uint64_t hi = __umul64hi(m, m), lo = m * m;
#else
  const unsigned __int128 M = (unsigned __int128)m * m;
  const uint64_t hi = (uint64_t)(M >> 64), lo = (uint64_t)M;
#endif
  const int sh = 2 * ex - q2 - 32 * limb;   // digit = floor(M * 2^sh) mod 2^32, M = hi:lo < 2^106
  if (sh >= 32) return 0u;
  if (sh >= 0) return (uint32_t)lo << sh;
  const int r = -sh;
  if (r >= 128) return 0u;
  if (r >= 64) return (uint32_t)(hi >> (r - 64));
  return (uint32_t)((lo >> r) | (hi << (64 - r)));
}

// ---- host finalisation ----------------------------------------------------------------------------------------------------------------------
// a 512-bit unsigned integer, base 2^32, w[0] least significant; the operations wrap modulo 2^512 (the callers' operands stay far below)
struct pg_u512 { uint32_t w[16]; };

static inline pg_u512 pg_u512_zero(void) {
  pg_u512 r;
  for (int i = 0; i < 16; i++) r.w[i] = 0;
  return r;
}
static inline int pg_u512_is_zero(const pg_u512& a) {
  for (int i = 0; i < 16; i++) if (a.w[i]) return 0;
  return 1;
}
static inline int pg_u512_cmp(const pg_u512& a, const pg_u512& b) {
  for (int i = 15; i >= 0; i--) if (a.w[i] != b.w[i]) return a.w[i] < b.w[i] ? -1 : 1;
  return 0;
}
static inline pg_u512 pg_u512_sub(const pg_u512& a, const pg_u512& b) {   // a - b
  pg_u512 r;
  uint64_t borrow = 0;
  for (int i = 0; i < 16; i++) {
    const uint64_t t = (uint64_t)a.w[i] - b.w[i] - borrow;
    r.w[i] = (uint32_t)t;
    borrow = (t >> 32) & 1u;
  }
  return r;
}
static inline pg_u512 pg_u512_mul(const pg_u512& a, const pg_u512& b) {
  pg_u512 r = pg_u512_zero();
  for (int i = 0; i < 16; i++) {
    if (!a.w[i]) continue;
    uint64_t carry = 0;
    for (int j = 0; i + j < 16; j++) {
      const uint64_t t = (uint64_t)a.w[i] * b.w[j] + r.w[i + j] + carry;   // < 2^64
      r.w[i + j] = (uint32_t)t;
      carry = t >> 32;
    }
  }
  return r;
}
static inline pg_u512 pg_u512_mul_u32(const pg_u512& a, uint32_t n) {
  pg_u512 r;
  uint64_t carry = 0;
  for (int i = 0; i < 16; i++) {
    const uint64_t t = (uint64_t)a.w[i] * n + carry;
    r.w[i] = (uint32_t)t;
    carry = t >> 32;
  }
  return r;
}
static inline pg_u512 pg_u512_shl(const pg_u512& a, int k) {   // 0 <= k < 512
  pg_u512 r = pg_u512_zero();
  const int ws = k >> 5, bs = k & 31;
  for (int i = 15; i >= ws; i--) {
    uint64_t v = (uint64_t)a.w[i - ws] << bs;
    if (bs && i - ws - 1 >= 0) v |= (uint64_t)a.w[i - ws - 1] >> (32 - bs);
    r.w[i] = (uint32_t)v;
  }
  return r;
}
static inline pg_u512 pg_u512_div_u32(const pg_u512& a, uint32_t n, uint32_t* rem) {   // n > 0
  pg_u512 q;
  uint64_t r = 0;
  for (int i = 15; i >= 0; i--) {
    const uint64_t t = (r << 32) | a.w[i];
    q.w[i] = (uint32_t)(t / n);
    r = t % n;
  }
  *rem = (uint32_t)r;
  return q;
}
static inline int pg_u512_top_bit(const pg_u512& a) {   // index of the highest set bit, -1 for zero
  for (int j = 15; j >= 0; j--) if (a.w[j]) return 32 * j + 31 - __builtin_clz(a.w[j]);
  return -1;
}
// |sum_j limbs[j] * 2^(32 j)| of signed int64 limbs (n_limbs <= 12); *neg: its sign
static inline pg_u512 pg_u512_from_limbs(const int64_t* limbs, int n_limbs, int* neg) {
  pg_u512 r;
  __int128 carry = 0;
  for (int j = 0; j < 16; j++) {
    const __int128 t = carry + (j < n_limbs ? (__int128)limbs[j] : 0);
    r.w[j] = (uint32_t)(t & 0xFFFFFFFF);
    carry = t >> 32;   // arithmetic shift: floor
  }
  *neg = (r.w[15] >> 31) != 0;
  if (*neg) {
    uint64_t c = 1;
    for (int j = 0; j < 16; j++) { const uint64_t t = (uint64_t)(uint32_t)~r.w[j] + c; r.w[j] = (uint32_t)t; c = t >> 32; }
  }
  return r;
}
// a * 2^scale (a with at least 54 significant bits, or zero) rounded to nearest-even; `sticky`: non-zero digits exist below a's lowest bit
static inline double pg_u512_round(const pg_u512& a, int scale, int sticky) {
  const int top = pg_u512_top_bit(a);
  if (top < 0) return 0.0;
  // the lowest bit kept: 53 bits from the top, or the lowest bit a double has (2^-1074) where the result is subnormal — rounding happens
  // once, at that bit
  int lsb = top - 52;
  if (lsb + scale < -1074) lsb = -1074 - scale;
  if (lsb > top + 1) return 0.0;   // below half of the smallest subnormal
#define PG_U512_BIT(i) ((i) < 0 ? 0ULL : (uint64_t)((a.w[(i) >> 5] >> ((i) & 31)) & 1u))
  uint64_t mant = 0;
  for (int i = top; i >= lsb; i--) mant = (mant << 1) | PG_U512_BIT(i);
  if (lsb > 0) {
    const uint64_t round = PG_U512_BIT(lsb - 1);
    for (int i = lsb - 2; i >= 0 && !sticky; i--) sticky = PG_U512_BIT(i) != 0;
    if (round && (sticky || (mant & 1))) mant++;
  }
#undef PG_U512_BIT
  return ldexp((double)mant, lsb + scale);   // exact: mant <= 2^53 and lsb + scale >= -1074 (beyond the largest double: infinity)
}

// m2 = Sq - Sx^2 / n of  Sx = sum_j sx[j] 2^(32 j + q1)  and  Sq = sum_j sq[j] 2^(32 j + q2),  rounded once; n >= 1.
// |Sx| 2^-q1 < 2^159 and Sq 2^-q2 < 2^223, |q2 - 2 q1| <= 64: n Sq and Sx^2 on the common scale stay below 2^320, and the 96 bits the
// numerator is shifted up before the division (so that the quotient carries a round bit and a sticky bit whatever n is) below 2^416.
static inline double pg_var_m2(int64_t n, const int64_t* sx, int n_sx, int q1, const int64_t* sq, int n_sq, int q2) {
  if (n <= 1) return 0.0;
  int neg_x = 0, neg_q = 0;
  pg_u512 X = pg_u512_from_limbs(sx, n_sx, &neg_x);
  pg_u512 Q = pg_u512_from_limbs(sq, n_sq, &neg_q);
  if (neg_q) return 0.0;   // (never: the digits of squares are not negative)
  pg_u512 A = pg_u512_mul_u32(Q, (uint32_t)n);   // n < 2^31
  pg_u512 B = pg_u512_mul(X, X);
  const int d = q2 - 2 * q1;
  int scale = 2 * q1;
  if (d >= 0) A = pg_u512_shl(A, d);
  else { B = pg_u512_shl(B, -d); scale = q2; }
  if (pg_u512_cmp(A, B) <= 0) return 0.0;   // equal values (or truncation below the window): exactly 0.0, never negative
  pg_u512 D = pg_u512_shl(pg_u512_sub(A, B), 96);
  uint32_t rem = 0;
  const pg_u512 quot = pg_u512_div_u32(D, (uint32_t)n, &rem);   // >= 2^65
  return pg_u512_round(quot, scale - 96, rem != 0);   // the remainder is the sticky bit below the quotient
}
