// Time-bucket transforms as GROUP BY / DISTINCT keys: the NORMAL FORM every function of the family is reduced to by the parser
// (pg_time_expr.h), and its evaluation for one value.  Plain declarations and one `__host__ __device__` function: pg_time_keys
// (pg_kernels_timekey.hip) and the stand-alone host program of tests/time_expr_main.cpp run the same code.
//
//   x  → x * pre_mul (wrapping)  → conv `in` (to milliseconds)  → bucket step  → conv `out` (from milliseconds)  → post step
//
// conv is java.util.concurrent.TimeUnit#convert: to a finer unit a SATURATING multiply, to a coarser one a division that truncates toward
// zero.  Plain `*`, `+`, `-` wrap as Java's do (computed in uint64_t: signed overflow is undefined in C++).  Every divisor is a literal of the
// query, so no division instruction is executed per value: the host precomputes a signed multiply-high reciprocal per divisor
// (pg_time_divisor; Warren, Hacker's Delight, 10-1 "signed division by divisors >= 2") and the calendar floors divide by compile-time
// constants only, which the compiler turns into the same multiply-high sequences.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PG_TIME_HD __host__ __device__ static inline
#else
#define PG_TIME_HD static inline
#endif

enum pg_time_conv_kind { PG_TIME_CONV_SAME = 0, PG_TIME_CONV_UP = 1, PG_TIME_CONV_DOWN = 2 };
enum pg_time_bucket_kind {
  PG_TIME_BUCKET_NONE = 0,
  PG_TIME_BUCKET_TRUNC = 1,     // ms / g * g, truncating (datetimeconvert's granularity)
  PG_TIME_BUCKET_FLOOR = 2,     // floor((ms + offset - phase) / g) * g + phase - offset: second .. week of datetrunc
  PG_TIME_BUCKET_MONTH = 3,     // floor to the first instant of the month / quarter / year of ms + offset (ISO chronology), minus offset
  PG_TIME_BUCKET_QUARTER = 4,
  PG_TIME_BUCKET_YEAR = 5
};
enum pg_time_post_kind { PG_TIME_POST_NONE = 0, PG_TIME_POST_DIV = 1 /* v / n */, PG_TIME_POST_ROUND = 2 /* v / n * n */ };

#define PG_TIME_DIV_ONE (-1)   // pg_time_divisor.shift: |d| == 1
#define PG_TIME_DIV_MIN (-2)   //                        d == Long.MIN_VALUE

// Java's n / d for a divisor d != 0 known on the host: q = mulhi(magic, n) (+ n when magic < 0) >> shift, plus one when negative; negated
// when d < 0 (magic and shift are those of |d|)
struct pg_time_divisor {
  int64_t d;
  int64_t magic;
  int32_t shift;
  int32_t neg;
};
struct pg_time_conv {
  int32_t kind;      // pg_time_conv_kind
  int32_t pad;
  int64_t mul;       // UP: the factor m ...
  int64_t limit;     // ... and Long.MAX_VALUE / m: beyond +-limit the result saturates
  pg_time_divisor div;   // DOWN
};
struct pg_time_program {
  int64_t pre_mul;   // 1: none (datetimeconvert: the input format's size)
  pg_time_conv in, out;
  int32_t bucket;    // pg_time_bucket_kind
  int32_t post;      // pg_time_post_kind
  pg_time_divisor bucket_div;   // TRUNC / FLOOR: g
  int64_t offset;    // FLOOR and the calendar floors: the zone's fixed offset in milliseconds
  int64_t phase;     // FLOOR: weeks begin on Monday, 1970-01-01 is a Thursday: 4 days; else 0
  pg_time_divisor post_div;     // n
};

PG_TIME_HD int64_t pg_time_mulhi(int64_t a, int64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __mul64hi(a, b);
#else
  return (int64_t)(((__int128)a * (__int128)b) >> 64);
#endif
}

PG_TIME_HD int64_t pg_time_div(int64_t n, const pg_time_divisor& D) {
  if (D.shift == PG_TIME_DIV_MIN) return n == INT64_MIN ? 1 : 0;
  uint64_t q = (uint64_t)n;
  if (D.shift != PG_TIME_DIV_ONE) {
    int64_t h = pg_time_mulhi(D.magic, n);
    if (D.magic < 0) h = (int64_t)((uint64_t)h + (uint64_t)n);
    h >>= D.shift;
    q = (uint64_t)h + ((uint64_t)h >> 63);
  }
  return (int64_t)(D.neg ? 0 - q : q);   // (Long.MIN_VALUE / -1 is Long.MIN_VALUE: the negation wraps, no division runs)
}

PG_TIME_HD int64_t pg_time_conv_apply(int64_t d, const pg_time_conv& C) {
  if (C.kind == PG_TIME_CONV_SAME) return d;
  if (C.kind == PG_TIME_CONV_UP) {
    if (d > C.limit) return INT64_MAX;
    if (d < -C.limit) return INT64_MIN;
    return d * C.mul;
  }
  return pg_time_div(d, C.div);
}

// floor(a / b) for a compile-time constant b > 0
#define PG_TIME_FLOOR_DIV(a, b) ((a) / (b) - (((a) % (b)) < 0 ? 1 : 0))

// The first day (days since 1970-01-01) of the month / quarter / year holding day `z`, proleptic Gregorian: the era / year-of-era / day-of-year
// decomposition over 400-year eras of 146 097 days that start on March 1st (public domain: H. Hinnant, "chrono-compatible low-level date
// algorithms")
PG_TIME_HD int64_t pg_time_calendar_floor_days(int64_t z, int32_t bucket) {
  z += 719468;
  const int64_t era = PG_TIME_FLOOR_DIV(z, (int64_t)146097);
  const int64_t doe = z - era * 146097;                                         // [0, 146096]
  const int64_t yoe = (doe - doe / 1460 + doe / 36524 - doe / 146096) / 365;    // [0, 399]
  const int64_t doy = doe - (365 * yoe + yoe / 4 - yoe / 100);                  // [0, 365], March 1st = 0
  const int64_t mp = (5 * doy + 2) / 153;                                       // [0, 11], March = 0
  int64_t m = mp < 10 ? mp + 3 : mp - 9;                                        // [1, 12]
  int64_t y = yoe + era * 400 + (m <= 2 ? 1 : 0);
  if (bucket == PG_TIME_BUCKET_YEAR) m = 1;
  else if (bucket == PG_TIME_BUCKET_QUARTER) m = (m - 1) / 3 * 3 + 1;
  // days_from_civil(y, m, 1)
  y -= m <= 2 ? 1 : 0;
  const int64_t era2 = PG_TIME_FLOOR_DIV(y, (int64_t)400);
  const int64_t yoe2 = y - era2 * 400;
  const int64_t doy2 = (153 * (m > 2 ? m - 3 : m + 9) + 2) / 5;
  const int64_t doe2 = yoe2 * 365 + yoe2 / 4 - yoe2 / 100 + doy2;
  return era2 * 146097 + doe2 - 719468;
}

PG_TIME_HD int64_t pg_time_eval(const pg_time_program& P, int64_t x) {
  int64_t ms = pg_time_conv_apply((int64_t)((uint64_t)x * (uint64_t)P.pre_mul), P.in);
  switch (P.bucket) {   // wave-uniform
    case PG_TIME_BUCKET_NONE: break;
    case PG_TIME_BUCKET_TRUNC:
      ms = (int64_t)((uint64_t)pg_time_div(ms, P.bucket_div) * (uint64_t)P.bucket_div.d);
      break;
    case PG_TIME_BUCKET_FLOOR: {
      const uint64_t g = (uint64_t)P.bucket_div.d;
      const uint64_t v = (uint64_t)ms + (uint64_t)P.offset - (uint64_t)P.phase;
      uint64_t q = (uint64_t)pg_time_div((int64_t)v, P.bucket_div);
      if ((int64_t)(v - q * g) < 0) q -= 1;
      ms = (int64_t)(q * g + (uint64_t)P.phase - (uint64_t)P.offset);
      break;
    }
    default: {
      const int64_t v = (int64_t)((uint64_t)ms + (uint64_t)P.offset);
      const int64_t day = PG_TIME_FLOOR_DIV(v, (int64_t)86400000);
      ms = (int64_t)((uint64_t)pg_time_calendar_floor_days(day, P.bucket) * (uint64_t)86400000 - (uint64_t)P.offset);
      break;
    }
  }
  int64_t o = pg_time_conv_apply(ms, P.out);
  if (P.post != PG_TIME_POST_NONE) {
    o = pg_time_div(o, P.post_div);
    if (P.post == PG_TIME_POST_ROUND) o = (int64_t)((uint64_t)o * (uint64_t)P.post_div.d);
  }
  return o;
}
