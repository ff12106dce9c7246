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
// CASE (CaseTransformFunction): case(when1,then1,...,whenN,thenN,else) with 2N+1 arguments; an omitted ELSE arrives as the literal 'null'.
// A WHEN is a comparison — equals / not_equals / greater_than / greater_than_or_equal / less_than / less_than_or_equal over two operands —
// or and / or / not over such calls; the first WHEN whose value is 1 selects its THEN, no WHEN the ELSE (without one: 0.0, the null
// placeholder).  The program evaluates every WHEN, THEN and ELSE in argument order and then N selects from the last WHEN backwards, all into
// the CASE's one dst: select N keeps thenN or the ELSE, select k < N keeps thenK or what the selects behind it left — the first true WHEN
// wins.  A comparison or a logical call anywhere else (an aggregation's argument, an arithmetic operand, a THEN / ELSE, a comparison's
// operand) is PG_ERR_UNSUPPORTED, like a comparison of two literals, a CASE as a comparison's operand and a logical call over anything but
// comparisons and logical calls.  What the value depends on beside the text — the operand columns' types — is recorded for the planner:
enum ExprType : int32_t { PG_EXPR_T_INT = 0, PG_EXPR_T_LONG = 1, PG_EXPR_T_FLOAT = 2, PG_EXPR_T_DOUBLE = 3, PG_EXPR_T_STRING = 4 };   // pg_data_type's numbering
// a literal's type from its text (RequestUtils.getLiteral): integer-looking and within int INT, within long LONG, any other number DOUBLE
struct ExprBranch {   // one THEN / ELSE of a CASE
  enum Kind : int32_t { COLUMN = 0, LITERAL = 1, ARITHMETIC = 2, CASE = 3 };
  int32_t kind = COLUMN;
  int32_t ref = 0;        // COLUMN: index into `columns`; LITERAL: its ExprType; CASE: index into `cases` (an earlier one)
  int32_t step = -1;      // LITERAL: the select that holds it, in pg_expr_step::lit (slot 0) or lit2 (slot 1) ...
  int32_t slot = 0;
  int64_t ival = 0;       // ... and an INT / LONG literal's exact value (a FLOAT-typed CASE narrows it with (float))
};
struct ExprCase {
  std::vector<ExprBranch> branches;   // the THENs in order, then the ELSE when there is one
  bool has_else = false;
};
struct ExprComparison {
  int32_t step = -1;             // the comparison's step
  int32_t column[2] = {-1, -1};  // per operand: index into `columns` when it is a plain column, else -1
  int32_t literal = -1;          // the operand that is a literal (0 / 1), -1: none
  int32_t literal_type = 0;      // ExprType; PG_EXPR_T_STRING: a quoted text that is no number (directly under equals / not_equals only)
  int64_t ival = 0;              // an INT / LONG literal's exact value
  std::string text;              // the literal as written: looked up in the dictionary when the other operand is a STRING column
};
struct ExprProgram {
  std::vector<std::string> columns;   // the distinct operand columns, in order of first appearance (steps refer to them by index)
  pg_expr_step steps[PG_EXPR_MAX_OPS];
  int32_t n_steps = 0;                // >= 1; the expression's value is the dst of the last step
  bool conditional = false;           // holds a CASE, a comparison or a logical operation (aggregations only: filters and keys refuse it)
  std::vector<ExprCase> cases;        // inner CASEs before the ones that hold them
  std::vector<ExprComparison> comparisons;
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
// PG_ERR_UNSUPPORTED (another function, more than PG_EXPR_MAX_SRCS columns or PG_EXPR_MAX_OPS operations — comparisons, logical operations
// and selects count, condition columns too —, a condition where none may stand) with the reason in `error`
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
