// The straight-line programs of arithmetic expressions inside aggregations: limits, opcodes and the step record, shared by the parser
// (pg_expr.h, host only) and the kernels' argument block (pg_device.h).  Plain C declarations: no parser, no C++ library headers.
#pragma once
#include <stdint.h>

#define PG_EXPR_MAX_SRCS 8    // distinct operand columns (PG_MAX_SRCS)
#define PG_EXPR_MAX_OPS 15    // operations of one expression
#define PG_EXPR_MAX_EXPRS 4   // distinct expressions of one query

// The four arithmetic operations; the six comparisons (Double.compare's total order over the operands as doubles: -0.0 below 0.0, NaN equal
// to NaN and above +Infinity; the result is 1.0 or 0.0); the logical operations over such results (AND: both != 0, OR: either != 0, NOT:
// a == 0; 1.0 or 0.0); and SELECT, dst = a == 1.0 ? b : c — what a CASE is lowered to (pg_expr.h).
enum pg_expr_opcode {
  PG_EXPR_ADD = 0, PG_EXPR_SUB = 1, PG_EXPR_MULT = 2, PG_EXPR_DIV = 3,
  PG_EXPR_EQ = 4, PG_EXPR_NE = 5, PG_EXPR_GT = 6, PG_EXPR_GE = 7, PG_EXPR_LT = 8, PG_EXPR_LE = 9,
  PG_EXPR_AND = 10, PG_EXPR_OR = 11, PG_EXPR_NOT = 12,
  PG_EXPR_SELECT = 13
};
// dst = a <op> b.  An operand is a column (0 .. PG_EXPR_MAX_SRCS-1), the result of an earlier operation (PG_EXPR_MAX_SRCS + its dst) or,
// when negative, a literal: `lit` for a or b (at most one of the two is a literal), `lit2` for c.  Only SELECT reads c (NOT reads a alone).
// dst counts the function calls of the expression that were not folded, in the order their first step appears.
struct pg_expr_step {
  int32_t op;
  int32_t dst;
  int32_t a, b, c;
  int32_t pad;
  double lit, lit2;
};

