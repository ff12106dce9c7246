// Stand-alone driver of the expression parser (pinot_amd/csrc/pg_expr.cpp), built with -fsanitize=address,undefined by
// tests/test_expr_parse.py: well-formed texts nested to the limits and every malformed one the test can think of, each handed over in a
// heap buffer of exactly its length so that a read past the text is caught.  Prints one line per case and "expr parse ok" at the end.
#include <locale.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../include/pinot_gpu.h"
#include "../pinot_amd/csrc/pg_expr.h"

static int failures = 0;

static int32_t parse(const std::string& text, pg::ExprProgram& prog, std::string& error) {
  char* exact = (char*)malloc(text.size() + 1);   // no slack behind the terminator
  memcpy(exact, text.c_str(), text.size() + 1);
  const int32_t st = pg::expr_parse(exact, prog, error);
  free(exact);
  return st;
}

static void expect(const char* what, const std::string& text, int32_t status, int n_steps = -1, int n_columns = -1) {
  pg::ExprProgram prog;
  std::string error;
  const int32_t st = parse(text, prog, error);
  bool ok = st == status;
  if (st == PG_OK) {
    ok = ok && error.empty() && prog.n_steps >= 1 && prog.n_steps <= PG_EXPR_MAX_OPS && prog.columns.size() >= 1 && prog.columns.size() <= PG_EXPR_MAX_SRCS;
    if (n_steps >= 0) ok = ok && prog.n_steps == n_steps;
    if (n_columns >= 0) ok = ok && (int)prog.columns.size() == n_columns;
    int n_dst = 0;
    for (int k = 0; k < prog.n_steps && ok; k++) {   // every reference points at a column or at an earlier result
      const pg_expr_step& s = prog.steps[k];
      ok = s.op >= PG_EXPR_ADD && s.op <= PG_EXPR_DIV && s.dst >= 0 && s.dst < PG_EXPR_MAX_OPS && s.dst <= n_dst && !(s.a < 0 && s.b < 0);
      const int32_t refs[2] = {s.a, s.b};
      for (int32_t r : refs) {
        if (r < 0) continue;
        if (r < PG_EXPR_MAX_SRCS) ok = ok && r < (int32_t)prog.columns.size();
        else ok = ok && r - PG_EXPR_MAX_SRCS <= n_dst && r - PG_EXPR_MAX_SRCS < PG_EXPR_MAX_OPS;
      }
      if (s.dst == n_dst) n_dst++;
    }
  } else {
    ok = ok && !error.empty() && error.size() < 512 && prog.n_steps == 0 && prog.columns.empty();   // every refusal carries a text
  }
  printf("%s %s: status %d (want %d), %d steps, %zu columns%s%s\n", ok ? "ok  " : "FAIL", what, st, status, prog.n_steps, prog.columns.size(), error.empty() ? "" : " — ", error.c_str());
  if (!ok) failures++;
}

static std::string nest(const char* fn, const char* leaf, int depth, bool through_first) {
  std::string t = leaf;
  for (int i = 0; i < depth; i++) t = through_first ? std::string(fn) + "(" + t + "," + leaf + ")" : std::string(fn) + "(" + leaf + "," + t + ")";
  return t;
}

// the double the program computes for given column values: the host-side restatement of the device loop
static double run(const pg::ExprProgram& p, const double* cols) {
  double t[PG_EXPR_MAX_OPS] = {0}, r = 0;
  for (int k = 0; k < p.n_steps; k++) {
    const pg_expr_step& s = p.steps[k];
    const double x = s.a < 0 ? s.lit : (s.a < PG_EXPR_MAX_SRCS ? cols[s.a] : t[s.a - PG_EXPR_MAX_SRCS]);
    const double y = s.b < 0 ? s.lit : (s.b < PG_EXPR_MAX_SRCS ? cols[s.b] : t[s.b - PG_EXPR_MAX_SRCS]);
    volatile double v = s.op == PG_EXPR_ADD ? x + y : s.op == PG_EXPR_SUB ? x - y : s.op == PG_EXPR_MULT ? x * y : x / y;
    r = v;
    t[s.dst] = r;
  }
  return r;
}

static void expect_value(const std::string& text, const double* cols, double want) {
  pg::ExprProgram prog;
  std::string error;
  const int32_t st = parse(text, prog, error);
  const double got = st == PG_OK ? run(prog, cols) : 0.0;
  const bool ok = st == PG_OK && memcmp(&got, &want, 8) == 0;
  printf("%s value of %s: %.17g (want %.17g)\n", ok ? "ok  " : "FAIL", text.c_str(), got, want);
  if (!ok) failures++;
}

int main() {
  const int32_t OK = PG_OK, INV = PG_ERR_INVALID_ARGUMENT, UNS = PG_ERR_UNSUPPORTED;
  // ---- well-formed -------------------------------------------------------------------------------------------------------------------------
  expect("two columns", "add(column1,column9)", OK, 2, 2);
  expect("a quoted literal", "mult(price,'1.5')", OK, 1, 1);
  expect("a bare literal", "mult(price,1.5)", OK, 1, 1);
  expect("aliases", "plus(minus(a,b),times(c,divide(d,e)))", OK, 6, 5);   // minus 1, divide 1, times 2, plus 2
  expect("upper case and blanks", " ADD( a , Sub( b , '2' ) ) ", OK, 3, 2);
  expect("literals between columns", "add(a,'5',b,'-2.5e3',c)", OK, 3, 3);
  expect("a literal-only call folds", "add(sub('3','1'),a)", OK, 1, 1);
  expect("nesting of the goldens", "add(div(INT_COL1,INT_COL2),div(LONG_COL1,LONG_COL2))", OK, 4, 4);
  expect("15 operations through the first argument", nest("sub", "a", 15, true), OK, 15, 1);
  expect("15 operations through the second argument", nest("div", "a", 15, false), OK, 15, 1);
  expect("15 operations in one call", "add(a,a,a,a,a,a,a,a,a,a,a,a,a,a,a)", OK, 15, 1);
  expect("8 columns", "add(c1,c2,c3,c4,c5,c6,c7,c8)", OK, 8, 8);
  expect("8 columns, each twice", "mult(add(c1,c2,c3,c4,c5,c6,c7,c8),sub(c1,div(c2,c8)))", OK, 12, 8);
  expect("a very long identifier", "add(" + std::string(100000, 'x') + ",b)", OK, 2, 2);
  expect("deep literal-only nesting within the limit", nest("add", "'1'", 14, true) + std::string(""), INV);   // folds to a literal: no column
  // ---- over the limits -----------------------------------------------------------------------------------------------------------------------
  expect("a 16th operation (nested)", nest("sub", "a", 16, true), UNS);
  expect("a 16th operation (one call)", "add(a,a,a,a,a,a,a,a,a,a,a,a,a,a,a,a)", UNS);
  expect("a 16th operation (second argument)", nest("div", "a", 16, false), UNS);
  expect("a 9th column", "add(c1,c2,c3,c4,c5,c6,c7,c8,c9)", UNS);
  expect("literal-only nesting past any useful depth", nest("add", "'1'", 4000, false), UNS);
  expect("mod", "mod(a,b)", UNS);
  expect("another function inside", "add(a,abs(b))", UNS);
  // ---- malformed -------------------------------------------------------------------------------------------------------------------------------
  expect("empty text", "", INV);
  expect("a plain column", "column1", INV);
  expect("unbalanced: no closing parenthesis", "add(a,b", INV);
  expect("unbalanced: nested", "add(a,sub(b,c)", INV);
  expect("unbalanced: one too many", "add(a,b))", INV);
  expect("only an opening parenthesis", "add(", INV);
  expect("no function name", "(a,b)", INV);
  expect("an empty argument", "add(a,)", INV);
  expect("an empty first argument", "add(,a)", INV);
  expect("two commas", "add(a,,b)", INV);
  expect("no arguments", "add()", INV);
  expect("one argument", "add(a)", INV);
  expect("three arguments to sub", "sub(a,b,c)", INV);
  expect("one argument to div", "div(a)", INV);
  expect("an unterminated quote", "add(a,'5)", INV);
  expect("an unterminated quote at the end", "add(a,'", INV);
  expect("a quote that is no number", "add(a,'five')", INV);
  expect("an empty quote", "add(a,'')", INV);
  expect("a number with a tail", "add(a,5x)", INV);
  expect("a name that starts with a digit is taken for a literal", "add(a,1st_col)", INV);
  expect("a lone sign", "add(a,-)", INV);
  expect("an exponent without digits", "add(a,1e)", INV);
  expect("a leading plus", "add(a,+2.5)", OK, 1, 1);
  expect("an infinite literal", "add(a,1e999)", INV);
  expect("a hexadecimal literal", "add(a,'0x10')", INV);
  expect("no column at all", "add('1','2')", INV);
  expect("no column in a nest", "mult(add('1','2'),sub('3','4'))", INV);
  expect("trailing text", "add(a,b) c", INV);
  expect("two operands without a comma", "add(a b)", INV);
  expect("a very long malformed text", "add(" + std::string(100000, '(') , INV);
  expect("a very long unterminated quote", "add(a,'" + std::string(100000, '9'), INV);
  // ---- the programs compute the reference's values ----------------------------------------------------------------------------------------------
  const double cols[3] = {1e16, -1e16, -0.0};
  expect_value("add(a,b,'1')", cols, 0.0);              // ((0.0 + 1) + 1e16) + -1e16: the literal first
  expect_value("add(add(a,b),'1')", cols, 1.0);
  expect_value("add(c,c)", cols + 0, 2e16);             // (first use names the column: c = cols[0])
  expect_value("sub('1',a)", cols, 1.0 - 1e16);
  expect_value("div(a,'3')", cols, 1e16 / 3.0);
  expect_value("mult(a,'2','0.25',b)", cols, ((1.0 * 2.0 * 0.25) * 1e16) * -1e16);
  expect_value("add(sub('3','1'),a)", cols, (0.0 + 2.0) + 1e16);
  // literals are read without regard to the process locale: under a decimal-comma locale (where the machine has one) 1.5 stays 1.5
  const char* loc = setlocale(LC_ALL, "de_DE.UTF-8");
  printf("locale: %s\n", loc ? loc : "(de_DE.UTF-8 not installed: the C locale stays)");
  expect_value("mult(a,'1.5')", cols, 1.5e16);
  expect_value("add(a,2.5e-1)", cols, 0.25 + 1e16);
  setlocale(LC_ALL, "C");
  const double zeros[2] = {-0.0, -0.0};
  expect_value("add(a,b)", zeros, 0.0);                 // 0.0 + -0.0 + -0.0 is +0.0
  expect_value("mult(a,'1')", zeros, -0.0);
  if (failures) { printf("%d failures\n", failures); return 1; }
  printf("expr parse ok\n");
  return 0;
}
