// CPU harness of tests/test_moments_host.py: feeds pinot_amd/csrc/pg_moments.h the vectors it reads from stdin, exactly as the kernels of
// pg_kernels_var.hip and the host of pg_exec_var.hip do (digits -> int64 limbs -> one rounding), and prints limbs and result bits.
// Built with -fsanitize=address,undefined and run as a program of its own.  One record per line:
//   K                        -> "K <sum limbs> <square limbs> <int slots> <long exponent>"
//   D <E> <n> <hex64 ...>    doubles as bit patterns, every finite |x| < 2^E: the double path
//   I <n> <int ...>          INT values: the integer path
//   U <op> <hexA> <hexB>     the 512-bit helper: op = mul | sub | cmp | shl (B: the bit count, decimal) | mulu (B: a u32, decimal) |
//                            div (B: a u32, decimal)
// D / I answer  "Q <q1> <q2>", "L <sum limbs ...> | <square limbs ...>", "R <n> <sum bits> <m2 bits>";  U answers "U <hex>" (div: + " <rem>").
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../pinot_amd/csrc/pg_moments.h"

static pg_u512 parse_hex(const std::string& s) {
  pg_u512 r = pg_u512_zero();
  int bit = 0;
  for (size_t i = s.size(); i-- > 0 && bit < 512; bit += 4) {
    const char c = s[i];
    const uint32_t v = (uint32_t)(c >= '0' && c <= '9' ? c - '0' : (c >= 'a' && c <= 'f' ? c - 'a' + 10 : 0));
    r.w[bit >> 5] |= v << (bit & 31);
  }
  return r;
}
static void print_hex(const pg_u512& a) {
  for (int i = 15; i >= 0; i--) printf("%08" PRIx32, a.w[i]);
}

static void finish(int64_t n, const int64_t* sx, int n_sx, int q1, const int64_t* sq, int n_sq, int q2) {
  printf("Q %d %d\nL", q1, q2);
  for (int j = 0; j < n_sx; j++) printf(" %" PRId64, sx[j]);
  printf(" |");
  for (int j = 0; j < n_sq; j++) printf(" %" PRId64, sq[j]);
  const double sum = pg_limbs_to_double(sx, n_sx, q1), m2 = pg_var_m2(n, sx, n_sx, q1, sq, n_sq, q2);
  uint64_t sb, mb;
  memcpy(&sb, &sum, 8);
  memcpy(&mb, &m2, 8);
  printf("\nR %" PRId64 " %016" PRIx64 " %016" PRIx64 "\n", n, sb, mb);
}

int main() {
  char kind[8];
  while (scanf("%7s", kind) == 1) {
    if (kind[0] == 'K') {
      printf("K %d %d %d %d\n", PG_VAR_SUM_LIMBS, PG_VAR_SQ_LIMBS, PG_VAR_INT_SLOTS, PG_VAR_LONG_EXP);
    } else if (kind[0] == 'D') {
      int E;
      long n;
      if (scanf("%d %ld", &E, &n) != 2) return 2;
      const int q1 = pg_var_q1(E), q2 = pg_var_q2(E);
      int64_t sx[PG_VAR_SUM_LIMBS] = {0}, sq[PG_VAR_SQ_LIMBS] = {0};
      for (long i = 0; i < n; i++) {
        uint64_t b;
        if (scanf("%" SCNx64, &b) != 1) return 2;
        double x;
        memcpy(&x, &b, 8);
        for (int j = 0; j < PG_VAR_SUM_LIMBS; j++) sx[j] += pg_fx_digit(x, q1, j);
        for (int j = 0; j < PG_VAR_SQ_LIMBS; j++) sq[j] += (int64_t)pg_sq_digit(x, q2, j);
      }
      finish(n, sx, PG_VAR_SUM_LIMBS, q1, sq, PG_VAR_SQ_LIMBS, q2);
    } else if (kind[0] == 'I') {
      long n;
      if (scanf("%ld", &n) != 1) return 2;
      int64_t sx[1] = {0}, sq[2] = {0, 0};
      for (long i = 0; i < n; i++) {
        int64_t v;
        if (scanf("%" SCNd64, &v) != 1) return 2;
        if (v < INT32_MIN || v > INT32_MAX) return 3;
        const int64_t s = v * v;
        sx[0] += v;
        sq[0] += pg_long_digit(s, 0);
        sq[1] += pg_long_digit(s, 1);
      }
      finish(n, sx, 1, 0, sq, 2, 0);
    } else if (kind[0] == 'U') {
      char op[8], a[160], b[160];
      if (scanf("%7s %159s %159s", op, a, b) != 3) return 2;
      const pg_u512 A = parse_hex(a);
      printf("U ");
      if (!strcmp(op, "mul")) print_hex(pg_u512_mul(A, parse_hex(b)));
      else if (!strcmp(op, "sub")) print_hex(pg_u512_sub(A, parse_hex(b)));
      else if (!strcmp(op, "cmp")) printf("%d", pg_u512_cmp(A, parse_hex(b)));
      else if (!strcmp(op, "shl")) print_hex(pg_u512_shl(A, atoi(b)));
      else if (!strcmp(op, "mulu")) print_hex(pg_u512_mul_u32(A, (uint32_t)strtoul(b, nullptr, 10)));
      else if (!strcmp(op, "div")) {
        uint32_t rem = 0;
        print_hex(pg_u512_div_u32(A, (uint32_t)strtoul(b, nullptr, 10), &rem));
        printf(" %" PRIu32, rem);
      } else return 2;
      printf("\n");
    } else {
      return 2;
    }
  }
  printf("moments ok\n");
  return 0;
}
