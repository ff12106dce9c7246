// The straight-line programs of arithmetic expressions inside aggregations: limits, opcodes and the step record, shared by the parser
// (pg_expr.h, host only) and the kernels' argument block (pg_device.h).  Plain C declarations: no parser, no C++ library headers.
#pragma once
#include <stdint.h>

#define PG_EXPR_MAX_SRCS 8    // distinct operand columns (PG_MAX_SRCS)
#define PG_EXPR_MAX_OPS 15    // operations of one expression
#define PG_EXPR_MAX_EXPRS 4   // distinct expressions of one query

enum pg_expr_opcode { PG_EXPR_ADD = 0, PG_EXPR_SUB = 1, PG_EXPR_MULT = 2, PG_EXPR_DIV = 3 };
// dst = a <op> b.  An operand is a column (0 .. PG_EXPR_MAX_SRCS-1), the result of an earlier operation (PG_EXPR_MAX_SRCS + its dst) or,
// when negative, the literal `lit` (at most one operand of a step is a literal).  dst counts the function calls of the expression that were
// not folded, in the order their first step appears.
struct pg_expr_step {
  int32_t op;
  int32_t dst;
  int32_t a, b;
  double lit;
};

