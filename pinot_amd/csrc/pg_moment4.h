// Exact third and fourth moments (SKEWNESS / KURTOSIS; shared by the kernels of pg_kernels_moment.hip, the executor pg_exec_moment.hip and a
// stand-alone CPU harness, tests/moment4_main.cpp; plain C++, no HIP types).
//
// The reference (FourthMomentAggregationFunction / PinotFourthMoment(n, m1, m2, m3, m4)) updates the mean and the central sums doc by doc in
// docId order and merges with combine(); every other order rounds differently.  As for the variance family (pg_moments.h, one step further)
// the GPU path accumulates n and the power sums  S1 = sum x, S2 = sum x^2, S3 = sum x^3, S4 = sum x^4  EXACTLY as integers and forms
//     m1 = S1 / n
//     m2 = S2 - S1^2 / n
//     m3 = S3 - 3 S1 S2 / n + 2 S1^3 / n^2
//     m4 = S4 - 4 S1 S3 / n + 6 S1^2 S2 / n^2 - 3 S1^4 / n^3
// in exact integer arithmetic on the host, rounding each of the four doubles ONCE (nearest-even).
//
//   S1, S2   exactly pg_moments.h's: pg_fx_digit with L1 = 4 at q1 = E - 127, pg_sq_digit with L2 = 6 at q2 = 2 E - 191; every finite |x| < 2^E.
//   S3, S4   x = +-m * 2^ex with the 53-bit mantissa m.  m^2 (< 2^106) is one 64 x 64 -> 128 multiply, m^3 = m^2 * m (< 2^159, three 64-bit
//            words) and m^4 = (m^2)^2 (< 2^212, four words) are schoolbook products of such multiplies (__umul64hi on the device, __int128 on
//            the host).  No FMA, no double-double, no overflow or underflow case: every finite double has an exact k-th power as an integer
//            times 2^(k ex).  Digit j (base 2^32) of trunc(m^k * 2^(k ex - q_k)) with q_k = k E - 32 L_k + 1 goes into limb j; the digits of x^3
//            carry the sign of x.  |x|^k < 2^(k E), so the integer stays below 2^(32 L_k - 1).
//   L_k      A value with |x| >= 2^(E - s - 1) has ex >= E - s - 53; its k-th power has no bit below 2^(k ex) and is held exactly when
//            k ex >= q_k, that is  k (s + 53) <= 32 L_k - 1.  L2 = 6 gives s <= 42 (pg_moments.h).  The same window needs 3 * 95 = 285 <= 32 L3 - 1
//            and 4 * 95 = 380 <= 32 L4 - 1: L3 = PG_M4_CUBE_LIMBS = 9 (287: s <= 42, 8 would give s <= 32) and L4 = PG_M4_QUAD_LIMBS = 12 (383:
//            s <= 42, 11 would give s <= 34).  E is a multiple of 16 at or above the largest exponent, which alone can cost s = 16: all four
//            sums are exact for every column whose magnitudes span up to 2^26.
//   slots    1 (the doc count, shared by the columns) + 4 + 6 + 9 + 12 = 32 per group for one column on the double path: 512 groups in the
//            LDS tier of PG_MOMENT_LDS_SLOTS = 16 384 slots.  A run of b bits touches at most floor((b + 30) / 32) + 1 digits: 3 of x, 5 of
//            x^2, 6 of x^3 and 8 of x^4 — at most 1 + 22 = 23 non-zero slot updates per doc whatever the L_k are.
//   INT      columns (raw or through an INT dictionary) take an integer path, all scales 0: S1 in one int64 slot (|x| <= 2^31, < 2^31 docs),
//            x^2 (<= 2^62) as two digits, x^3 (|x^3| <= 2^93) as three signed digits and x^4 (<= 2^124) as four: 1 + 1 + 2 + 3 + 4 = 11 slots
//            and as many updates per doc, 1 489 groups in the LDS tier.  Integers are always exact.
//   LONG     columns are read as the reference's getDoubleValuesSV reads them ((double) rounded first) and take the double path with E = 64:
//            q1 = -63, q2 = -63, q3 = 192 - 287 = -95 and q4 = 256 - 383 = -127 are all negative, and the powers of an integer have no bit below
//            2^0: integer values are always exact.
//   overflow A digit is below 2^32 in magnitude and a segment has fewer than 2^31 docs: every int64 limb stays below 2^63.
//            A FLOAT / DOUBLE column with 4 E >= 1024 (pg_m4_overflows) admits an x^4 beyond the largest double; the plan refuses it.
//
// Truncation.  Values below a window are truncated toward zero: |sum x - S1| < n 2^q1 and |sum x^k - Sk| < n 2^qk, with |S1| < n 2^E,
// S2 < n 2^(2E), |S3| < n 2^(3E).  From |ab - a'b'| <= |a||b - b'| + |b'||a - a'| and |a^k - a'^k| <= k max(|a|,|a'|)^(k-1) |a - a'|, before the
// final rounding
//     |m2 - exact| < n (2^q2 + 2 * 2^(E + q1))                                                    (pg_moments.h's two terms)
//     |m3 - exact| < n (2^q3 + 3 * 2^(E + q2) + 9 * 2^(2E + q1))
//         (S3; 3 S1 S2 / n: 3 n (2^(E + q2) + 2^(2E + q1)); 2 S1^3 / n^2: 6 n 2^(2E + q1))
//     |m4 - exact| < n (2^q4 + 4 * 2^(E + q3) + 6 * 2^(2E + q2) + 28 * 2^(3E + q1))
//         (S4; 4 S1 S3 / n: 4 n (2^(E + q3) + 2^(3E + q1)); 6 S1^2 S2 / n^2: 6 n (2^(2E + q2) + 2 * 2^(3E + q1)); 3 S1^4 / n^3: 12 n 2^(3E + q1))
// and |m1 - exact| < 2^q1.  With the scales above the last term of each line dominates: 2^(2E - 126), 9 * 2^(3E - 127), 28 * 2^(4E - 127), times n.
// Where the windows hold every digit the four doubles are the correctly rounded true values.  m2 and m4 are never negative and never -0.0 (a
// difference that truncation made negative is clamped to 0.0); m3 keeps its sign, an exact zero is +0.0; for n = 1 the tuple is
// (1, x, 0.0, 0.0, 0.0); over no doc it is the reference's fresh PinotFourthMoment, (0, NaN, NaN, NaN, NaN).
#pragma once
#include <stdint.h>

#include "pg_fixed_point.h"
#include "pg_moments.h"

#define PG_M4_CUBE_LIMBS 9
#define PG_M4_QUAD_LIMBS 12
#define PG_M4_INT_SLOTS 10                                                                            // integer path: 1 + 2 + 3 + 4
#define PG_M4_DBL_SLOTS (PG_VAR_SUM_LIMBS + PG_VAR_SQ_LIMBS + PG_M4_CUBE_LIMBS + PG_M4_QUAD_LIMBS)   // double path: 31
#define PG_MOMENT_LDS_SLOTS 16384   // 64-bit slots of the LDS tier: 128 KiB of the CU's 160 KiB, one persistent workgroup per CU (as pg_var_lds)
#define PG_MOMENT_MAX_COLS 3        // distinct argument columns of one query: what pg_moment_reg holds in registers without scratch (pg_kernels_moment.hip)

PG_FX_HD int pg_m4_q3(int E) { return 3 * E - 32 * PG_M4_CUBE_LIMBS + 1; }
PG_FX_HD int pg_m4_q4(int E) { return 4 * E - 32 * PG_M4_QUAD_LIMBS + 1; }
PG_FX_HD int pg_m4_overflows(int E) { return 4 * E >= 1024; }   // x^4 may pass the largest double

PG_FX_HD void pg_m4_mul64(uint64_t a, uint64_t b, uint64_t* hi, uint64_t* lo) {
#if defined(__HIP_DEVICE_COMPILE__)
  *hi = __umul64hi(a, b);
  *lo = a * b;
#else
  const unsigned __int128 p = (unsigned __int128)a * b;
  *hi = (uint64_t)(p >> 64);
  *lo = (uint64_t)p;
#endif
}

// The powers of one finite double: |x| = m * 2^ex with the 53-bit m; p3 = m^3 (three 64-bit words, least significant first), p4 = m^4 (four).
struct pg_m4_powers {
  int ex, neg;
  uint64_t p3[3], p4[4];
};
PG_FX_HD pg_m4_powers pg_m4_powers_of(double x) {
  pg_m4_powers P;
  uint64_t b;
  __builtin_memcpy(&b, &x, 8);
  const int e = (int)((b >> 52) & 0x7FFu);
  uint64_t m = b & 0xFFFFFFFFFFFFFULL;
  P.ex = -1074;
  if (e) { m |= 1ULL << 52; P.ex = e - 1075; }
  P.neg = (int)(b >> 63);
  uint64_t h2, l2;
  pg_m4_mul64(m, m, &h2, &l2);   // m^2 = h2:l2 < 2^106, h2 < 2^42
  // m^3 = l2 m + h2 m 2^64
  uint64_t ah, al;
  pg_m4_mul64(l2, m, &ah, &al);
  uint64_t bh, bl;
  pg_m4_mul64(h2, m, &bh, &bl);   // < 2^95
  P.p3[0] = al;
  P.p3[1] = ah + bl;
  P.p3[2] = bh + (P.p3[1] < ah ? 1u : 0u);
  // m^4 = l2^2 + 2 l2 h2 2^64 + h2^2 2^128
  uint64_t ch, cl, dh, dl;
  pg_m4_mul64(l2, l2, &ch, &cl);
  pg_m4_mul64(l2, h2, &dh, &dl);   // l2 h2 < 2^106: dh < 2^42, so 2 l2 h2 = (dh << 1 | dl >> 63) : (dl << 1) does not lose a bit
  const uint64_t d0 = dl << 1, d1 = (dh << 1) | (dl >> 63);
  uint64_t sh, sl;
  pg_m4_mul64(h2, h2, &sh, &sl);   // < 2^84
  P.p4[0] = cl;
  P.p4[1] = ch + d0;
  const uint64_t c1 = P.p4[1] < ch ? 1u : 0u;
  const uint64_t t2 = d1 + sl;     // d1 < 2^43, sl < 2^64: may carry
  const uint64_t c2 = t2 < sl ? 1u : 0u;
  P.p4[2] = t2 + c1;
  const uint64_t c3 = P.p4[2] < t2 ? 1u : 0u;
  P.p4[3] = sh + c2 + c3;
  return P;
}

// digit = floor(P * 2^sh) mod 2^32 of P = sum_i w[i] 2^(64 i); the words are picked by comparisons, never by an address: registers on the device
template <int W>
PG_FX_HD uint32_t pg_m4_words_digit(const uint64_t (&w)[W], int sh) {
  if (sh >= 32) return 0u;
  if (sh >= 0) return (uint32_t)w[0] << sh;
  const int r = -sh, wi = r >> 6, bit = r & 63;
  uint64_t lo = 0, hi = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int i = 0; i < W; i++) {
    if (wi == i) lo = w[i];
    if (wi + 1 == i) hi = w[i];
  }
  return bit ? (uint32_t)((lo >> bit) | (hi << (64 - bit))) : (uint32_t)lo;
}
// digit `limb` of trunc(|x|^3 * 2^-q3), carrying x's sign, and of trunc(x^4 * 2^-q4)
PG_FX_HD int64_t pg_m4_cube_digit(const pg_m4_powers& P, int q3, int limb) {
  const int64_t d = (int64_t)pg_m4_words_digit<3>(P.p3, 3 * P.ex - q3 - 32 * limb);
  return P.neg ? -d : d;
}
PG_FX_HD int64_t pg_m4_quad_digit(const pg_m4_powers& P, int q4, int limb) { return (int64_t)pg_m4_words_digit<4>(P.p4, 4 * P.ex - q4 - 32 * limb); }

// the integer path: the PG_M4_INT_SLOTS digits of an INT value's x, x^2, x^3 and x^4
PG_FX_HD void pg_m4_int_digits(int64_t x, int64_t* d) {
  const uint64_t a = (uint64_t)(x < 0 ? -x : x);   // <= 2^31
  const uint64_t a2 = a * a;                       // <= 2^62
  uint64_t h3, l3, h4, l4;
  pg_m4_mul64(a2, a, &h3, &l3);                    // <= 2^93
  pg_m4_mul64(a2, a2, &h4, &l4);                   // <= 2^124
  d[0] = x;
  d[1] = (int64_t)(uint32_t)a2;
  d[2] = (int64_t)(a2 >> 32);
  const int64_t c0 = (int64_t)(uint32_t)l3, c1 = (int64_t)(l3 >> 32), c2 = (int64_t)(uint32_t)h3;
  d[3] = x < 0 ? -c0 : c0;
  d[4] = x < 0 ? -c1 : c1;
  d[5] = x < 0 ? -c2 : c2;
  d[6] = (int64_t)(uint32_t)l4;
  d[7] = (int64_t)(l4 >> 32);
  d[8] = (int64_t)(uint32_t)h4;
  d[9] = (int64_t)(h4 >> 32);
}

// ---- host finalisation ----------------------------------------------------------------------------------------------------------------------
// The numerators over n, n^2, n^3 on their common scale 4 q1 (the smallest of q4, q1 + q3, 2 q1 + q2, 4 q1 = 4 E - 508): every term of m4's is
// below c n^4 2^(4E) 2^(508 - 4E) < c 2^(124 + 508) with c = 1, 4, 6, 3, their sum below 14 * 2^632 < 2^636.  The numerator is shifted up by
// PG_WIDE_GUARD = 160 bits before the divisions (n^3 < 2^93: a non-zero quotient keeps at least 67 bits, a round bit and sticky bits among
// them): 796 bits, rounded up to a multiple of 64: PG_WIDE_WORDS = 26 words of 32 bits, 832 bits.  (pg_u512 of pg_moments.h holds m2's 416.)
// w[0] is least significant; the operations wrap modulo 2^832 (the callers' operands stay below, as derived above).
#define PG_WIDE_WORDS 26
#define PG_WIDE_GUARD 160
struct pg_wide { uint32_t w[PG_WIDE_WORDS]; };

static inline pg_wide pg_wide_zero(void) {
  pg_wide r;
  for (int i = 0; i < PG_WIDE_WORDS; i++) r.w[i] = 0;
  return r;
}
static inline int pg_wide_cmp(const pg_wide& a, const pg_wide& b) {
  for (int i = PG_WIDE_WORDS - 1; i >= 0; i--) if (a.w[i] != b.w[i]) return a.w[i] < b.w[i] ? -1 : 1;
  return 0;
}
static inline pg_wide pg_wide_add(const pg_wide& a, const pg_wide& b) {
  pg_wide r;
  uint64_t carry = 0;
  for (int i = 0; i < PG_WIDE_WORDS; i++) {
    const uint64_t t = (uint64_t)a.w[i] + b.w[i] + carry;
    r.w[i] = (uint32_t)t;
    carry = t >> 32;
  }
  return r;
}
static inline pg_wide pg_wide_sub(const pg_wide& a, const pg_wide& b) {   // a - b
  pg_wide r;
  uint64_t borrow = 0;
  for (int i = 0; i < PG_WIDE_WORDS; i++) {
    const uint64_t t = (uint64_t)a.w[i] - b.w[i] - borrow;
    r.w[i] = (uint32_t)t;
    borrow = (t >> 32) & 1u;
  }
  return r;
}
static inline pg_wide pg_wide_mul(const pg_wide& a, const pg_wide& b) {
  pg_wide r = pg_wide_zero();
  for (int i = 0; i < PG_WIDE_WORDS; i++) {
    if (!a.w[i]) continue;
    uint64_t carry = 0;
    for (int j = 0; i + j < PG_WIDE_WORDS; j++) {
      const uint64_t t = (uint64_t)a.w[i] * b.w[j] + r.w[i + j] + carry;   // < 2^64
      r.w[i + j] = (uint32_t)t;
      carry = t >> 32;
    }
  }
  return r;
}
static inline pg_wide pg_wide_mul_u32(const pg_wide& a, uint32_t n) {
  pg_wide r;
  uint64_t carry = 0;
  for (int i = 0; i < PG_WIDE_WORDS; i++) {
    const uint64_t t = (uint64_t)a.w[i] * n + carry;
    r.w[i] = (uint32_t)t;
    carry = t >> 32;
  }
  return r;
}
static inline pg_wide pg_wide_shl(const pg_wide& a, int k) {   // 0 <= k < 32 PG_WIDE_WORDS
  pg_wide r = pg_wide_zero();
  const int ws = k >> 5, bs = k & 31;
  for (int i = PG_WIDE_WORDS - 1; i >= ws; i--) {
    uint64_t v = (uint64_t)a.w[i - ws] << bs;
    if (bs && i - ws - 1 >= 0) v |= (uint64_t)a.w[i - ws - 1] >> (32 - bs);
    r.w[i] = (uint32_t)v;
  }
  return r;
}
static inline pg_wide pg_wide_div_u32(const pg_wide& a, uint32_t n, uint32_t* rem) {   // n > 0
  pg_wide q;
  uint64_t r = 0;
  for (int i = PG_WIDE_WORDS - 1; i >= 0; i--) {
    const uint64_t t = (r << 32) | a.w[i];
    q.w[i] = (uint32_t)(t / n);
    r = t % n;
  }
  *rem = (uint32_t)r;
  return q;
}
static inline int pg_wide_top_bit(const pg_wide& a) {   // index of the highest set bit, -1 for zero
  for (int j = PG_WIDE_WORDS - 1; j >= 0; j--) if (a.w[j]) return 32 * j + 31 - __builtin_clz(a.w[j]);
  return -1;
}
// a * 2^scale (a with at least 54 significant bits, or zero) rounded to nearest-even; `sticky`: non-zero digits exist below a's lowest bit
static inline double pg_wide_round(const pg_wide& a, int scale, int sticky) {
  const int top = pg_wide_top_bit(a);
  if (top < 0) return 0.0;
  // the lowest bit kept: 53 bits from the top, or the lowest bit a double has (2^-1074) where the result is subnormal — one rounding, at that bit
  int lsb = top - 52;
  if (lsb + scale < -1074) lsb = -1074 - scale;
  if (lsb > top + 1) return 0.0;   // below half of the smallest subnormal
#define PG_WIDE_BIT(i) ((i) < 0 ? 0ULL : (uint64_t)((a.w[(i) >> 5] >> ((i) & 31)) & 1u))
  uint64_t mant = 0;
  for (int i = top; i >= lsb; i--) mant = (mant << 1) | PG_WIDE_BIT(i);
  if (lsb > 0) {
    const uint64_t round = PG_WIDE_BIT(lsb - 1);
    for (int i = lsb - 2; i >= 0 && !sticky; i--) sticky = PG_WIDE_BIT(i) != 0;
    if (round && (sticky || (mant & 1))) mant++;
  }
#undef PG_WIDE_BIT
  return ldexp((double)mant, lsb + scale);   // exact: mant <= 2^53 and lsb + scale >= -1074
}

// a signed wide integer: magnitude and sign (zero is never negative)
struct pg_swide { pg_wide m; int neg; };
// sum_j limbs[j] * 2^(32 j) of signed int64 limbs (n_limbs <= PG_M4_QUAD_LIMBS)
static inline pg_swide pg_swide_from_limbs(const int64_t* limbs, int n_limbs) {
  pg_swide r;
  __int128 carry = 0;
  for (int j = 0; j < PG_WIDE_WORDS; j++) {
    const __int128 t = carry + (j < n_limbs ? (__int128)limbs[j] : 0);
    r.m.w[j] = (uint32_t)(t & 0xFFFFFFFF);
    carry = t >> 32;   // arithmetic shift: floor
  }
  r.neg = (r.m.w[PG_WIDE_WORDS - 1] >> 31) != 0;
  if (r.neg) {
    uint64_t c = 1;
    for (int j = 0; j < PG_WIDE_WORDS; j++) { const uint64_t t = (uint64_t)(uint32_t)~r.m.w[j] + c; r.m.w[j] = (uint32_t)t; c = t >> 32; }
  }
  return r;
}
static inline pg_swide pg_swide_mul(const pg_swide& a, const pg_swide& b) {
  pg_swide r;
  r.m = pg_wide_mul(a.m, b.m);
  r.neg = (a.neg != b.neg) && pg_wide_top_bit(r.m) >= 0;
  return r;
}
// a * c * 2^k with the sign flipped if `negate`
static inline pg_swide pg_swide_scale(const pg_swide& a, uint32_t c, int k, int negate) {
  pg_swide r;
  r.m = pg_wide_shl(pg_wide_mul_u32(a.m, c), k);
  r.neg = (a.neg != (negate != 0)) && pg_wide_top_bit(r.m) >= 0;
  return r;
}
static inline pg_swide pg_swide_add(const pg_swide& a, const pg_swide& b) {
  pg_swide r;
  if (a.neg == b.neg) {
    r.m = pg_wide_add(a.m, b.m);
    r.neg = a.neg;
    return r;
  }
  const int c = pg_wide_cmp(a.m, b.m);
  if (c == 0) { r.m = pg_wide_zero(); r.neg = 0; return r; }
  r.m = c > 0 ? pg_wide_sub(a.m, b.m) : pg_wide_sub(b.m, a.m);
  r.neg = c > 0 ? a.neg : b.neg;
  return r;
}
// num * 2^scale / n^divs rounded once, the sign kept: the remainders of the divisions are the sticky bit
static inline double pg_swide_quotient(const pg_swide& num, int scale, uint32_t n, int divs) {
  pg_wide q = pg_wide_shl(num.m, PG_WIDE_GUARD);
  int sticky = 0;
  for (int i = 0; i < divs; i++) {
    uint32_t rem = 0;
    q = pg_wide_div_u32(q, n, &rem);
    sticky |= rem != 0;
  }
  const double v = pg_wide_round(q, scale - PG_WIDE_GUARD, sticky);
  return num.neg ? -v : v;
}

// PinotFourthMoment(n, m1, m2, m3, m4): serialize() is the long and the four doubles, big-endian
struct pg_m4_tuple {
  int64_t n;
  double m1, m2, m3, m4;
};
// The tuple of  Sk = sum_j sk[j] 2^(32 j + qk)  (n1 .. n4 limbs; the integer path: 1, 2, 3, 4 limbs at scale 0), each double rounded once.
static inline pg_m4_tuple pg_m4_tuple_of(int64_t n, const int64_t* s1, int n1, int q1, const int64_t* s2, int n2, int q2, const int64_t* s3, int n3, int q3,
                                         const int64_t* s4, int n4, int q4) {
  pg_m4_tuple t;
  t.n = n;
  if (n <= 0) {   // a fresh PinotFourthMoment
    t.m1 = t.m2 = t.m3 = t.m4 = __builtin_nan("");
    return t;
  }
  const uint32_t N = (uint32_t)n;   // < 2^31
  const pg_swide X1 = pg_swide_from_limbs(s1, n1);
  t.m1 = pg_swide_quotient(X1, q1, N, 1);
  t.m2 = t.m3 = t.m4 = 0.0;
  if (n == 1) return t;
  const pg_swide X2 = pg_swide_from_limbs(s2, n2), X3 = pg_swide_from_limbs(s3, n3), X4 = pg_swide_from_limbs(s4, n4);
  const pg_swide X11 = pg_swide_mul(X1, X1), X111 = pg_swide_mul(X11, X1);
  // m2 n = n S2 - S1^2
  {
    const int sa = q2, sb = 2 * q1, sc = sa < sb ? sa : sb;
    const pg_swide num = pg_swide_add(pg_swide_scale(X2, N, sa - sc, 0), pg_swide_scale(X11, 1, sb - sc, 1));
    const double v = pg_swide_quotient(num, sc, N, 1);
    t.m2 = v > 0.0 ? v : 0.0;   // equal values (or truncation below the window): exactly 0.0, never negative
  }
  // m3 n^2 = n^2 S3 - 3 n S1 S2 + 2 S1^3
  {
    const int sa = q3, sb = q1 + q2, sd = 3 * q1;
    int sc = sa < sb ? sa : sb;
    if (sd < sc) sc = sd;
    pg_swide num = pg_swide_scale(pg_swide_scale(X3, N, 0, 0), N, sa - sc, 0);
    num = pg_swide_add(num, pg_swide_scale(pg_swide_scale(pg_swide_mul(X1, X2), N, 0, 0), 3, sb - sc, 1));
    num = pg_swide_add(num, pg_swide_scale(X111, 2, sd - sc, 0));
    const double v = pg_swide_quotient(num, sc, N, 2);
    t.m3 = v == 0.0 ? 0.0 : v;   // an exact zero is +0.0
  }
  // m4 n^3 = n^3 S4 - 4 n^2 S1 S3 + 6 n S1^2 S2 - 3 S1^4
  {
    const int sa = q4, sb = q1 + q3, sd = 2 * q1 + q2, se = 4 * q1;
    int sc = sa < sb ? sa : sb;
    if (sd < sc) sc = sd;
    if (se < sc) sc = se;
    pg_swide num = pg_swide_scale(pg_swide_scale(pg_swide_scale(X4, N, 0, 0), N, 0, 0), N, sa - sc, 0);
    num = pg_swide_add(num, pg_swide_scale(pg_swide_scale(pg_swide_scale(pg_swide_mul(X1, X3), N, 0, 0), N, 0, 0), 4, sb - sc, 1));
    num = pg_swide_add(num, pg_swide_scale(pg_swide_scale(pg_swide_mul(X11, X2), N, 0, 0), 6, sd - sc, 0));
    num = pg_swide_add(num, pg_swide_scale(pg_swide_mul(X111, X1), 3, se - sc, 1));
    const double v = pg_swide_quotient(num, sc, N, 3);
    t.m4 = v > 0.0 ? v : 0.0;
  }
  return t;
}
