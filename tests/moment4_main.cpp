// CPU harness of tests/test_moment4_host.py: feeds pinot_amd/csrc/pg_moment4.h the vectors it reads from stdin, exactly as the kernels of
// pg_kernels_moment.hip and the host of pg_exec_moment.hip do (digits -> int64 limbs -> one rounding per double), and prints limbs and
// result bits.  Built with -fsanitize=address,undefined and run as a program of its own.  One record per line:
//   K                        -> "K <sum limbs> <square limbs> <cube limbs> <quad limbs> <int slots> <long exponent> <wide words> <guard bits>"
//   D <E> <n> <hex64 ...>    doubles as bit patterns, every finite |x| < 2^E: the double path
//   I <n> <int ...>          INT values: the integer path
//   U <op> <hexA> <hexB>     the wide integer: op = mul | add | sub | cmp | shl (B: the bit count, decimal) | mulu (B: a u32, decimal) |
//                            div (B: a u32, decimal)
// D / I answer  "Q <q1> <q2> <q3> <q4>", "L <S1 limbs ...> | <S2 ...> | <S3 ...> | <S4 ...>", "R <n> <m1 bits> <m2 bits> <m3 bits> <m4 bits>";
// U answers "U <hex>" (div: + " <rem>").
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../pinot_amd/csrc/pg_moment4.h"

static pg_wide parse_hex(const std::string& s) {
  pg_wide r = pg_wide_zero();
  int bit = 0;
  for (size_t i = s.size(); i-- > 0 && bit < 32 * PG_WIDE_WORDS; bit += 4) {
    const char c = s[i];
    const uint32_t v = (uint32_t)(c >= '0' && c <= '9' ? c - '0' : (c >= 'a' && c <= 'f' ? c - 'a' + 10 : 0));
    r.w[bit >> 5] |= v << (bit & 31);
  }
  return r;
}
static void print_hex(const pg_wide& a) {
  for (int i = PG_WIDE_WORDS - 1; i >= 0; i--) printf("%08" PRIx32, a.w[i]);
}

static void finish(int64_t n, const int64_t* s, const int* len, const int* q) {
  printf("Q %d %d %d %d\nL", q[0], q[1], q[2], q[3]);
  const int64_t* p = s;
  for (int k = 0; k < 4; k++) {
    if (k) printf(" |");
    for (int j = 0; j < len[k]; j++) printf(" %" PRId64, p[j]);
    p += len[k];
  }
  const int64_t* s1 = s;
  const int64_t* s2 = s1 + len[0];
  const int64_t* s3 = s2 + len[1];
  const int64_t* s4 = s3 + len[2];
  const pg_m4_tuple t = pg_m4_tuple_of(n, s1, len[0], q[0], s2, len[1], q[1], s3, len[2], q[2], s4, len[3], q[3]);
  const double m[4] = {t.m1, t.m2, t.m3, t.m4};
  printf("\nR %" PRId64, t.n);
  for (int k = 0; k < 4; k++) {
    uint64_t b;
    memcpy(&b, &m[k], 8);
    printf(" %016" PRIx64, b);
  }
  printf("\n");
}

int main() {
  char kind[8];
  while (scanf("%7s", kind) == 1) {
    if (kind[0] == 'K') {
      printf("K %d %d %d %d %d %d %d %d\n", PG_VAR_SUM_LIMBS, PG_VAR_SQ_LIMBS, PG_M4_CUBE_LIMBS, PG_M4_QUAD_LIMBS, PG_M4_INT_SLOTS, PG_VAR_LONG_EXP, PG_WIDE_WORDS,
             PG_WIDE_GUARD);
    } else if (kind[0] == 'D') {
      int E;
      long n;
      if (scanf("%d %ld", &E, &n) != 2) return 2;
      const int q[4] = {pg_var_q1(E), pg_var_q2(E), pg_m4_q3(E), pg_m4_q4(E)};
      const int len[4] = {PG_VAR_SUM_LIMBS, PG_VAR_SQ_LIMBS, PG_M4_CUBE_LIMBS, PG_M4_QUAD_LIMBS};
      int64_t s[PG_M4_DBL_SLOTS] = {0};
      for (long i = 0; i < n; i++) {
        uint64_t b;
        if (scanf("%" SCNx64, &b) != 1) return 2;
        double x;
        memcpy(&x, &b, 8);
        const pg_m4_powers P = pg_m4_powers_of(x);
        int64_t* p = s;
        for (int j = 0; j < len[0]; j++) *p++ += pg_fx_digit(x, q[0], j);
        for (int j = 0; j < len[1]; j++) *p++ += (int64_t)pg_sq_digit(x, q[1], j);
        for (int j = 0; j < len[2]; j++) *p++ += pg_m4_cube_digit(P, q[2], j);
        for (int j = 0; j < len[3]; j++) *p++ += pg_m4_quad_digit(P, q[3], j);
      }
      finish(n, s, len, q);
    } else if (kind[0] == 'I') {
      long n;
      if (scanf("%ld", &n) != 1) return 2;
      const int q[4] = {0, 0, 0, 0}, len[4] = {1, 2, 3, 4};
      int64_t s[PG_M4_INT_SLOTS] = {0};
      for (long i = 0; i < n; i++) {
        int64_t v;
        if (scanf("%" SCNd64, &v) != 1) return 2;
        if (v < INT32_MIN || v > INT32_MAX) return 3;
        int64_t d[PG_M4_INT_SLOTS];
        pg_m4_int_digits(v, d);
        for (int j = 0; j < PG_M4_INT_SLOTS; j++) s[j] += d[j];
      }
      finish(n, s, len, q);
    } else if (kind[0] == 'U') {
      char op[8], a[256], b[256];
      if (scanf("%7s %255s %255s", op, a, b) != 3) return 2;
      const pg_wide A = parse_hex(a);
      printf("U ");
      if (!strcmp(op, "mul")) print_hex(pg_wide_mul(A, parse_hex(b)));
      else if (!strcmp(op, "add")) print_hex(pg_wide_add(A, parse_hex(b)));
      else if (!strcmp(op, "sub")) print_hex(pg_wide_sub(A, parse_hex(b)));
      else if (!strcmp(op, "cmp")) printf("%d", pg_wide_cmp(A, parse_hex(b)));
      else if (!strcmp(op, "shl")) print_hex(pg_wide_shl(A, atoi(b)));
      else if (!strcmp(op, "mulu")) print_hex(pg_wide_mul_u32(A, (uint32_t)strtoul(b, nullptr, 10)));
      else if (!strcmp(op, "div")) {
        uint32_t rem = 0;
        print_hex(pg_wide_div_u32(A, (uint32_t)strtoul(b, nullptr, 10), &rem));
        printf(" %" PRIu32, rem);
      } else return 2;
      printf("\n");
    } else {
      return 2;
    }
  }
  printf("moment4 ok\n");
  return 0;
}
