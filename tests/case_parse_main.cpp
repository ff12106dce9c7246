// Stand-alone driver of the expression parser's CASE half (pinot_amd/csrc/pg_expr.cpp), built with -fsanitize=address,undefined by
// tests/test_case_parse.py: the lowering of case / comparisons / and / or / not to the straight-line program, its limits reached through
// CASE, every malformed shape, and a host-side run of each accepted program against hand values.  Each text is handed over in a heap
// buffer of exactly its length.  Prints one line per case and "case parse ok" at the end.
#include <math.h>
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

static void report(bool ok, const char* what, const std::string& detail) {
  printf("%s %s%s%s\n", ok ? "ok  " : "FAIL", what, detail.empty() ? "" : ": ", detail.c_str());
  if (!ok) failures++;
}

// every reference of an accepted program points at a column, at an earlier result or at a literal; the records point at their steps
static bool well_formed(const pg::ExprProgram& p) {
  bool ok = p.n_steps >= 1 && p.n_steps <= PG_EXPR_MAX_OPS && !p.columns.empty() && p.columns.size() <= PG_EXPR_MAX_SRCS;
  int n_dst = 0;
  for (int k = 0; k < p.n_steps && ok; k++) {
    const pg_expr_step& s = p.steps[k];
    ok = s.op >= PG_EXPR_ADD && s.op <= PG_EXPR_SELECT && s.dst >= 0 && s.dst < PG_EXPR_MAX_OPS && s.dst <= n_dst;
    const bool select = s.op == PG_EXPR_SELECT;
    const int32_t refs[3] = {s.a, s.b, select ? s.c : -1};
    if (!select) ok = ok && !(s.a < 0 && s.b < 0);
    if (select || s.op >= PG_EXPR_AND) ok = ok && s.a >= PG_EXPR_MAX_SRCS;   // a condition is an earlier result
    for (int32_t r : refs) {
      if (r < 0) continue;
      if (r < PG_EXPR_MAX_SRCS) ok = ok && r < (int32_t)p.columns.size();
      else ok = ok && r - PG_EXPR_MAX_SRCS <= n_dst && r - PG_EXPR_MAX_SRCS < PG_EXPR_MAX_OPS;
    }
    if (s.dst == n_dst) n_dst++;
  }
  for (const pg::ExprComparison& c : p.comparisons) ok = ok && c.step >= 0 && c.step < p.n_steps && p.steps[c.step].op >= PG_EXPR_EQ && p.steps[c.step].op <= PG_EXPR_LE;
  for (size_t i = 0; i < p.cases.size(); i++)
    for (const pg::ExprBranch& b : p.cases[i].branches) {
      if (b.kind == pg::ExprBranch::LITERAL) ok = ok && b.step >= 0 && b.step < p.n_steps && p.steps[b.step].op == PG_EXPR_SELECT && (b.slot == 0 ? p.steps[b.step].b : p.steps[b.step].c) < 0;
      if (b.kind == pg::ExprBranch::CASE) ok = ok && b.ref >= 0 && (size_t)b.ref < i;
      if (b.kind == pg::ExprBranch::COLUMN) ok = ok && b.ref >= 0 && (size_t)b.ref < p.columns.size();
    }
  return ok;
}

static void expect(const char* what, const std::string& text, int32_t status, int n_steps = -1, int n_columns = -1, const char* in_error = nullptr) {
  pg::ExprProgram prog;
  std::string error;
  const int32_t st = parse(text, prog, error);
  bool ok = st == status;
  if (st == PG_OK) {
    ok = ok && error.empty() && well_formed(prog);
    if (n_steps >= 0) ok = ok && prog.n_steps == n_steps;
    if (n_columns >= 0) ok = ok && (int)prog.columns.size() == n_columns;
  } else {
    ok = ok && !error.empty() && error.size() < 512 && prog.n_steps == 0 && prog.columns.empty() && prog.cases.empty() && prog.comparisons.empty() && !prog.conditional;
    if (in_error) ok = ok && error.find(in_error) != std::string::npos;
  }
  char detail[700];
  snprintf(detail, sizeof(detail), "status %d (want %d), %d steps, %zu columns%s%.500s", st, status, prog.n_steps, prog.columns.size(), error.empty() ? "" : " — ", error.c_str());
  report(ok, what, detail);
}

// Double.compare's order as a key
static long long key_of(double v) {
  long long b;
  if (v != v) b = 0x7FF8000000000000LL;
  else memcpy(&b, &v, 8);
  return b ^ ((b >> 63) & 0x7FFFFFFFFFFFFFFFLL);
}
// the double the program computes for given column values: the host-side restatement of the device loop
static double run(const pg::ExprProgram& p, const double* cols) {
  double t[PG_EXPR_MAX_OPS] = {0}, r = 0;
  for (int k = 0; k < p.n_steps; k++) {
    const pg_expr_step& s = p.steps[k];
    auto val = [&](int32_t ref, double lit) { return ref < 0 ? lit : (ref < PG_EXPR_MAX_SRCS ? cols[ref] : t[ref - PG_EXPR_MAX_SRCS]); };
    const double x = val(s.a, s.lit), y = val(s.b, s.lit);
    volatile double v = 0;
    switch (s.op) {
      case PG_EXPR_ADD: v = x + y; break;
      case PG_EXPR_SUB: v = x - y; break;
      case PG_EXPR_MULT: v = x * y; break;
      case PG_EXPR_DIV: v = y == 0 ? (x == 0 || x != x ? NAN : (signbit(x) != signbit(y) ? -INFINITY : INFINITY)) : x / y; break;   // (no trap under UBSan)
      case PG_EXPR_EQ: v = key_of(x) == key_of(y); break;
      case PG_EXPR_NE: v = key_of(x) != key_of(y); break;
      case PG_EXPR_GT: v = key_of(x) > key_of(y); break;
      case PG_EXPR_GE: v = key_of(x) >= key_of(y); break;
      case PG_EXPR_LT: v = key_of(x) < key_of(y); break;
      case PG_EXPR_LE: v = key_of(x) <= key_of(y); break;
      case PG_EXPR_AND: v = x != 0 && y != 0; break;
      case PG_EXPR_OR: v = x != 0 || y != 0; break;
      case PG_EXPR_NOT: v = x == 0; break;
      default: v = x == 1.0 ? y : val(s.c, s.lit2); break;
    }
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
  const bool ok = st == PG_OK && prog.conditional && memcmp(&got, &want, 8) == 0;
  char detail[400];
  snprintf(detail, sizeof(detail), "%.200s = %.17g (want %.17g) %.100s", text.c_str(), got, want, error.c_str());
  report(ok, "value", detail);
}

static std::string whens(int n, const char* then) {   // case(gt(a,'0'),then,gt(a,'1'),then,...,'0'): n comparisons + n selects
  std::string t = "case(";
  for (int i = 0; i < n; i++) t += "greater_than(a,'" + std::to_string(i) + "')," + then + ",";
  return t + "'0')";
}

int main() {
  const int32_t OK = PG_OK, INV = PG_ERR_INVALID_ARGUMENT, UNS = PG_ERR_UNSUPPORTED;
  // ---- the lowering ------------------------------------------------------------------------------------------------------------------------
  {
    pg::ExprProgram p;
    std::string error;
    const int32_t st = parse("case(greater_than(a,'3'),'3',GREATERTHAN(a,'2'),b,Greater_Than(a,'1'),'1','-1')", p, error);
    bool ok = st == OK && well_formed(p) && p.conditional && p.n_steps == 6 && p.columns.size() == 2 && p.cases.size() == 1 && p.comparisons.size() == 3;
    // three comparisons in argument order, each a node of its own; then the selects from the last WHEN backwards, all into the CASE's dst
    for (int k = 0; ok && k < 3; k++) ok = p.steps[k].op == PG_EXPR_GT && p.steps[k].dst == k && p.steps[k].a == 0 && p.steps[k].b < 0 && p.steps[k].lit == 3.0 - k;
    ok = ok && p.steps[3].op == PG_EXPR_SELECT && p.steps[3].dst == 3 && p.steps[3].a == PG_EXPR_MAX_SRCS + 2 && p.steps[3].b < 0 && p.steps[3].lit == 1.0 && p.steps[3].c < 0 && p.steps[3].lit2 == -1.0;
    ok = ok && p.steps[4].op == PG_EXPR_SELECT && p.steps[4].dst == 3 && p.steps[4].a == PG_EXPR_MAX_SRCS + 1 && p.steps[4].b == 1 && p.steps[4].c == PG_EXPR_MAX_SRCS + 3;
    ok = ok && p.steps[5].op == PG_EXPR_SELECT && p.steps[5].dst == 3 && p.steps[5].a == PG_EXPR_MAX_SRCS + 0 && p.steps[5].lit == 3.0 && p.steps[5].c == PG_EXPR_MAX_SRCS + 3;
    if (ok) {
      const pg::ExprCase& C = p.cases[0];
      ok = C.has_else && C.branches.size() == 4 && C.branches[0].kind == pg::ExprBranch::LITERAL && C.branches[0].ref == pg::PG_EXPR_T_INT && C.branches[0].step == 5 &&
           C.branches[1].kind == pg::ExprBranch::COLUMN && C.branches[1].ref == 1 && C.branches[2].step == 3 && C.branches[2].slot == 0 && C.branches[3].step == 3 &&
           C.branches[3].slot == 1 && C.branches[3].ival == -1;
    }
    report(ok, "lowering order", error);
  }
  {
    pg::ExprProgram p;
    std::string error;
    const int32_t st = parse("mult(case(and(equals(s,'ok'),or(less_than(a,b),not(not_equals(a,'7')))),add(a,'1'),'null'),'2')", p, error);
    // equals 0, less_than 1, not_equals 2, not 3, or 4, and 5, add 6, select 7, mult 8
    bool ok = st == OK && well_formed(p) && p.n_steps == 9 && p.columns.size() == 3 && p.cases.size() == 1 && !p.cases[0].has_else && p.cases[0].branches.size() == 1 &&
              p.cases[0].branches[0].kind == pg::ExprBranch::ARITHMETIC && p.comparisons.size() == 3;
    ok = ok && p.comparisons[0].literal == 1 && p.comparisons[0].literal_type == pg::PG_EXPR_T_STRING && p.comparisons[0].text == "ok" && p.comparisons[0].column[0] == 0;
    ok = ok && p.comparisons[1].literal == -1 && p.comparisons[1].column[0] == 1 && p.comparisons[1].column[1] == 2;
    ok = ok && p.comparisons[2].literal == 1 && p.comparisons[2].literal_type == pg::PG_EXPR_T_INT && p.comparisons[2].ival == 7 && p.comparisons[2].text == "7";
    ok = ok && p.steps[3].op == PG_EXPR_NOT && p.steps[4].op == PG_EXPR_OR && p.steps[5].op == PG_EXPR_AND && p.steps[7].op == PG_EXPR_SELECT && p.steps[7].c < 0 && p.steps[7].lit2 == 0.0 &&
         p.steps[8].op == PG_EXPR_MULT;
    report(ok, "conditions, a string literal kept as text, no ELSE", error);
  }
  {
    pg::ExprProgram p;
    std::string error;
    const int32_t st = parse("case(less_than(a,'0'),case(equals(a,'-1'),'2147483648','1.5'),a)", p, error);
    const bool ok = st == OK && well_formed(p) && p.cases.size() == 2 && p.cases[0].branches[0].ref == pg::PG_EXPR_T_LONG && p.cases[0].branches[0].ival == 2147483648LL &&
                    p.cases[0].branches[1].ref == pg::PG_EXPR_T_DOUBLE && p.cases[1].branches[0].kind == pg::ExprBranch::CASE && p.cases[1].branches[0].ref == 0 &&
                    p.cases[1].branches[1].kind == pg::ExprBranch::COLUMN;
    report(ok, "a nested CASE is recorded before the one that holds it; literal types", error);
  }
  expect("and / or flattened n-ary: k - 1 steps each", "case(and(equals(a,'1'),equals(b,'2'),equals(c,'3'),equals(d,'4')),'1','0')", OK, 8, 4);
  expect("a plain expression is not conditional", "add(a,b)", OK, 2, 2);
  // ---- the limits, reached through CASE -----------------------------------------------------------------------------------------------------------
  expect("15 operations: 7 WHENs and a sub", "sub(" + whens(7, "'1'") + ",a)", OK, 15, 1);
  expect("a 16th operation through CASE", "sub(" + whens(7, "'1'") + ",sub(a,'1'))", UNS, -1, -1, "more than 15 operations");
  expect("a 16th operation: 8 WHENs", whens(8, "'1'"), UNS, -1, -1, "more than 15 operations");
  expect("8 columns, condition columns counting", "case(and(equals(c1,c2),equals(c3,c4),equals(c5,c6)),c7,c8)", OK, 6, 8);
  expect("a 9th column in a condition", "case(and(equals(c1,c2),equals(c3,c4),equals(c5,c6),equals(c7,c9)),c7,c8)", UNS, -1, -1, "more than 8 distinct columns");
  expect("a 9th column as the ELSE", "case(and(equals(c1,c2),equals(c3,c4),equals(c5,c6),equals(c7,c8)),c7,c9)", UNS, -1, -1, "more than 8 distinct columns");
  // ---- malformed and out of scope -----------------------------------------------------------------------------------------------------------------
  expect("an even argument count", "case(equals(a,'1'),'1')", INV, -1, -1, "odd number of arguments");
  expect("an even argument count (4)", "case(equals(a,'1'),'1',equals(a,'2'),'2')", INV, -1, -1, "odd number of arguments");
  expect("one argument", "case(a)", INV, -1, -1, "odd number of arguments");
  expect("no argument", "case()", INV);
  expect("a non-comparison WHEN: a column", "case(a,'1','0')", UNS, -1, -1, "a WHEN that is no comparison");
  expect("a non-comparison WHEN: a literal", "case('1','1','0')", UNS, -1, -1, "a WHEN that is no comparison");
  expect("a non-comparison WHEN: arithmetic", "case(add(a,b),'1','0')", UNS, -1, -1, "a WHEN that is no comparison");
  expect("a non-comparison WHEN: 'null'", "case('null','1','0')", UNS, -1, -1, "a WHEN that is no comparison");
  expect("a comparison outside a WHEN: the argument", "greater_than(a,'1')", UNS, -1, -1, "outside a WHEN");
  expect("a comparison outside a WHEN: an arithmetic operand", "add(a,equals(b,'1'))", UNS, -1, -1, "outside a WHEN");
  expect("a comparison outside a WHEN: a THEN", "case(equals(a,'1'),equals(b,'1'),'0')", UNS, -1, -1, "outside a WHEN");
  expect("a comparison as the ELSE", "case(equals(a,'1'),'1',equals(b,'1'))", UNS, -1, -1, "as the ELSE");
  expect("a comparison of a comparison", "case(equals(equals(a,'1'),'1'),'1','0')", UNS, -1, -1, "outside a WHEN");
  expect("a logical call outside a WHEN", "and(equals(a,'1'),equals(b,'1'))", UNS, -1, -1, "outside a WHEN");
  expect("a comparison of two literals", "case(equals('1','1'),a,'0')", UNS, -1, -1, "over two literals");
  expect("and over a bare column", "case(and(a,equals(b,'1')),'1','0')", UNS, -1, -1, "and over a column");
  expect("not over a literal", "case(not('1'),a,'0')", UNS, -1, -1, "not over a column");
  expect("and with one argument", "case(and(equals(a,'1')),'1','0')", INV, -1, -1, "and takes 2 or more");
  expect("not with two arguments", "case(not(equals(a,'1'),equals(a,'2')),'1','0')", INV, -1, -1, "not takes exactly 1");
  expect("equals with three arguments", "case(equals(a,'1','2'),'1','0')", INV, -1, -1, "equals takes exactly 2");
  expect("a CASE as a comparison's operand", "case(equals(case(equals(a,'1'),'1','0'),'1'),'1','0')", UNS, -1, -1, "a CASE as an operand");
  expect("an unterminated string literal", "case(equals(s,'ok),1,0)", INV, -1, -1, "unterminated quote");
  expect("an unterminated string literal at the end", "case(equals(s,'", INV, -1, -1, "unterminated quote");
  expect("a string literal under an ordering comparison", "case(greater_than(s,'ok'),'1','0')", INV, -1, -1, "not a decimal number");
  expect("a string literal as a THEN", "case(equals(a,'1'),'ok','0')", INV, -1, -1, "not a decimal number");
  expect("a string literal as the ELSE", "case(equals(a,'1'),'1','ok')", INV, -1, -1, "not a decimal number");
  expect("'null' as a THEN", "case(equals(a,'1'),'null','0')", INV, -1, -1, "not a decimal number");
  expect("a string literal against arithmetic", "case(equals(add(a,b),'ok'),'1','0')", INV, -1, -1, "not a decimal number");
  expect("a string literal in arithmetic inside a WHEN", "case(equals(a,add(b,'ok')),'1','0')", INV, -1, -1, "not a decimal number");
  expect("mod inside a WHEN", "case(equals(mod(a,'2'),'0'),'1','0')", UNS, -1, -1, "the function mod");
  expect("no column at all", "case(equals('1','2'),'1','0')", UNS);
  expect("unbalanced", "case(equals(a,'1'),'1','0'", INV, -1, -1, "unbalanced parentheses");
  expect("trailing text", "case(equals(a,'1'),'1','0') x", INV, -1, -1, "trailing text");
  expect("a very long string literal", "case(equals(s,'" + std::string(100000, 'x') + "'),'1','0')", OK, 2, 1);
  // ---- the programs compute the reference's values -------------------------------------------------------------------------------------------------
  const double nan = NAN, inf = INFINITY;
  {
    const std::string prio = "case(greater_than(a,'3'),'3',greater_than(a,'2'),'2',greater_than(a,'1'),'1','-1')";
    const double v4[1] = {4}, v3[1] = {3}, v2[1] = {2}, v1[1] = {1}, vn[1] = {nan};
    expect_value(prio, v4, 3.0);       // all three hold: the first wins
    expect_value(prio, v3, 2.0);
    expect_value(prio, v2, 1.0);
    expect_value(prio, v1, -1.0);
    expect_value(prio, vn, 3.0);       // NaN above everything
  }
  {
    const double z[2] = {0.0, -0.0}, m[2] = {-0.0, 7.0}, n2[2] = {nan, nan};
    expect_value("case(equals(a,b),'1','0')", z, 0.0);                 // Double.compare: 0.0 is not -0.0
    expect_value("case(greater_than(a,b),'1','0')", z, 1.0);           // ... it is above it
    expect_value("case(less_than(a,'0'),'1','0')", m, 1.0);            // -0.0 < 0
    expect_value("case(less_than_or_equal(a,'-0.0'),b,'0')", m, 7.0);
    expect_value("case(equals(a,b),'1','0')", n2, 1.0);                // NaN equals NaN
    expect_value("case(not_equals(a,b),'1','0')", n2, 0.0);
    expect_value("case(greater_than_or_equal(a,'1e308'),'1','0')", n2, 1.0);
  }
  {
    const double zero[2] = {0.0, 5.0}, two[2] = {2.0, 5.0};   // columns in order of first appearance: b, a
    expect_value("case(not_equals(b,'0'),div(a,b),'0')", zero, 0.0);   // a / b is +Inf on this doc: not selected, it goes nowhere
    expect_value("case(not_equals(b,'0'),div(a,b),'0')", two, 2.5);
  }
  {
    const double c3[3] = {3.0, 8.0, -inf};
    expect_value("case(and(greater_than(a,'2'),or(equals(b,'1'),not(less_than(b,'8')))),a,'null')", c3, 3.0);
    expect_value("case(and(greater_than(a,'2'),or(equals(b,'1'),not(less_than(b,'9')))),a,'null')", c3, 0.0);   // no ELSE: the placeholder
    expect_value("case(or(less_than(a,b),equals(a,'0'),equals(a,'1')),add(a,b),'-1')", c3, 11.0);
    expect_value("mult('2',case(less_than(a,b),case(greater_than(a,'5'),'1',c),'7'))", c3, -inf);
    expect_value("sub(case(less_than(a,b),a,b),case(less_than(a,b),b,a))", c3, -5.0);
  }
  if (failures) { printf("%d failures\n", failures); return 1; }
  printf("case parse ok\n");
  return 0;
}
