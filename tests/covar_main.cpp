// CPU harness of tests/test_covar_host.py: feeds pinot_amd/csrc/pg_covar.h the vectors it reads from stdin, exactly as the kernels of
// pg_kernels_covar.hip and the host of pg_exec_covar.hip do (one rounded multiply -> digits -> int64 limbs -> one rounding per sum), and
// prints limbs and result bits.  Built with -fsanitize=address,undefined and -ffp-contract=off, run as a program of its own.  One record
// per line:
//   K                                              -> "K <product limbs> <int exponent> <max cols> <max pairs> <window>"
//   O <Ex> <Ey>                                    -> "O <0|1>": does the plan refuse the pair for overflow?
//   P <I|D> <Ex> <I|D> <Ey> <n> <hex64 x ...> <hex64 y ...>   the two columns as doubles (bit patterns), I: an INT column (one slot)
// P answers "Q <q1x> <q1y> <qp>", "L <x limbs ...> | <y limbs ...> | <product limbs ...>", "R <sumX bits> <sumY bits> <sumXY bits> <n>".
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../pinot_amd/csrc/pg_covar.h"

static double from_bits(uint64_t b) {
  double d;
  memcpy(&d, &b, 8);
  return d;
}
static uint64_t to_bits(double d) {
  uint64_t b;
  memcpy(&b, &d, 8);
  return b;
}

int main() {
  char kind[8];
  while (scanf("%7s", kind) == 1) {
    if (kind[0] == 'K') {
      printf("K %d %d %d %d %d\n", PG_COVAR_PROD_LIMBS, PG_COVAR_INT_EXP, PG_COVAR_MAX_COLS, PG_COVAR_MAX_PAIRS, PG_COVAR_WINDOW);
    } else if (kind[0] == 'O') {
      int Ex, Ey;
      if (scanf("%d %d", &Ex, &Ey) != 2) return 2;
      printf("O %d\n", pg_covar_overflows(Ex, Ey));
    } else if (kind[0] == 'P') {
      char tx[4], ty[4];
      int Ex, Ey;
      long n;
      if (scanf("%3s %d %3s %d %ld", tx, &Ex, ty, &Ey, &n) != 5 || n < 0) return 2;
      const int x_int = tx[0] == 'I', y_int = ty[0] == 'I';
      std::vector<double> x((size_t)n), y((size_t)n);
      for (std::vector<double>* v : {&x, &y})
        for (long i = 0; i < n; i++) {
          uint64_t b;
          if (scanf("%" SCNx64, &b) != 1) return 2;
          (*v)[(size_t)i] = from_bits(b);
        }
      const int Ep = pg_covar_prod_exp(Ex, Ey), qp = pg_covar_qp(Ep);
      const int q1x = x_int ? 0 : pg_var_q1(Ex), q1y = y_int ? 0 : pg_var_q1(Ey);
      int64_t sx[PG_COVAR_DBL_SLOTS] = {0}, sy[PG_COVAR_DBL_SLOTS] = {0}, sp[PG_COVAR_PROD_LIMBS] = {0};
      for (long i = 0; i < n; i++) {
        const double a = x[(size_t)i], b = y[(size_t)i];
        if (x_int) sx[0] += (int64_t)a;
        else for (int l = 0; l < PG_COVAR_DBL_SLOTS; l++) sx[l] += pg_fx_digit(a, q1x, l);
        if (y_int) sy[0] += (int64_t)b;
        else for (int l = 0; l < PG_COVAR_DBL_SLOTS; l++) sy[l] += pg_fx_digit(b, q1y, l);
        volatile double p = a * b;   // one rounded multiply
        for (int l = 0; l < PG_COVAR_PROD_LIMBS; l++) sp[l] += pg_covar_prod_digit(p, qp, l);
      }
      printf("Q %d %d %d\nL", q1x, q1y, qp);
      for (int l = 0; l < pg_covar_col_slots(x_int); l++) printf(" %" PRId64, sx[l]);
      printf(" |");
      for (int l = 0; l < pg_covar_col_slots(y_int); l++) printf(" %" PRId64, sy[l]);
      printf(" |");
      for (int l = 0; l < PG_COVAR_PROD_LIMBS; l++) printf(" %" PRId64, sp[l]);
      const pg_covar_tuple t = pg_covar_tuple_of((int64_t)n, sx, x_int, Ex, sy, y_int, Ey, sp, Ep);
      printf("\nR %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %" PRId64 "\n", to_bits(t.sum_x), to_bits(t.sum_y), to_bits(t.sum_xy), t.count);
    } else {
      return 2;
    }
  }
  printf("covar ok\n");
  return 0;
}
