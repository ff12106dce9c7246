// Arithmetic expressions inside aggregations: the text ExpressionContext#toString prints — fn(arg,arg,...) over add / sub / mult / div and
// their aliases plus / minus / times / divide (TransformFunctionType.java:47-50), columns and numeric literals (bare or single-quoted) —
// parsed into a small straight-line program.  Plain C++ without HIP types: it compiles stand-alone (tests/expr_parse_main.cpp).
// Host only: the kernels see pg_expr_program.h.
//
// The program restates the reference's transform functions one rounded IEEE double operation at a time, in their order:
//   add(args):  sum = 0.0; sum += every literal argument, in argument order; then sum += every other argument, in argument order
//               (AdditionTransformFunction: _literalSum, then the non-literal arguments)
//   mult(args): the same with 1.0 and *=  (MultiplicationTransformFunction)
//   sub(a, b) = a - b, div(a, b) = a / b  (exactly two arguments)
// A function call over literals only is folded to a literal, as the reference's compiler does before a segment sees it.  An OPERATION is one
// such step on the device: add / mult over k non-literal arguments take k, sub / div one.
#pragma once
#include "pg_expr_program.h"

#include <string>
#include <vector>

namespace pg {
struct ExprProgram {
  std::vector<std::string> columns;   // the distinct operand columns, in order of first appearance (steps refer to them by index)
  pg_expr_step steps[PG_EXPR_MAX_OPS];
  int32_t n_steps = 0;                // >= 1; the expression's value is the dst of the last step
};
// An argument that starts with a digit, '+', '-' or '.' is a LITERAL (decimal notation, parsed without regard to the process locale): a
// column whose name starts so cannot be an operand here — such a text is PG_ERR_INVALID_ARGUMENT, and the Java plan answers.
// does an aggregation's argument spell an expression?  (A Pinot column name cannot contain '('.)
inline bool expr_is_expression(const char* text) {
  if (!text) return false;
  for (const char* p = text; *p; p++) if (*p == '(') return true;
  return false;
}
// PG_OK, or PG_ERR_INVALID_ARGUMENT (malformed text, a wrong argument count, a literal that is no number, no column in it) /
// PG_ERR_UNSUPPORTED (another function, more than PG_EXPR_MAX_SRCS columns or PG_EXPR_MAX_OPS operations) with the reason in `error`
int32_t expr_parse(const char* text, ExprProgram& out, std::string& error);
// The argument list of an aggregation with more than one argument (pg_agg_spec.column of FIRSTWITHTIME / LASTWITHTIME, "x,t,'DOUBLE'"), split
// by the lexer of the expression texts above: commas at depth 0, single-quoted literals, blanks around an argument dropped.  A nested call
// stays one argument with its parentheses (expr_is_expression tells).  PG_OK, or PG_ERR_INVALID_ARGUMENT (null or empty text, an empty
// argument, an unterminated quote, text behind a quoted literal, unbalanced parentheses) with the reason in `error`.
struct ExprArgument {
  std::string text;      // a quoted literal: without its quotes
  bool quoted = false;
};
int32_t expr_split_arguments(const char* text, std::vector<ExprArgument>& out, std::string& error);
}  // namespace pg
