/* The NativeQuery wire format of a filter whose predicate has an arithmetic expression on its left-hand side, through the shim's C half
 * (integration/jni/pinot_gpu_shim.c): the expression travels as the text ExpressionContext#toString prints, in the predicate's column string —
 * of any length.  Compiled and run by tests/test_expression_filter_sql.py; prints one line per check and "wire format ok" at the end. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pinot_gpu.h"
#include "pinot_gpu_shim.h"

typedef struct { uint8_t b[4096]; size_t n; } record;
static void w_i32(record* r, int32_t v) { for (int i = 0; i < 4; i++) r->b[r->n++] = (uint8_t)((uint32_t)v >> (8 * i)); }
static void w_str(record* r, const char* s) {
  if (!s) { w_i32(r, -1); return; }
  const size_t len = strlen(s);
  w_i32(r, (int32_t)len);
  memcpy(r->b + r->n, s, len);
  r->n += len;
  while (r->n & 3) r->b[r->n++] = 0;
}
static void w_predicate(record* r, int32_t type, const char* column, int32_t n_values, const char* const* values, const char* lower, const char* upper,
                        int32_t lower_inclusive, int32_t upper_inclusive) {
  w_i32(r, PG_FILTER_PREDICATE); w_i32(r, 0);
  w_i32(r, type); w_i32(r, n_values);
  w_str(r, column);
  for (int32_t i = 0; i < n_values; i++) w_str(r, values[i]);
  w_str(r, lower); w_str(r, upper);
  w_i32(r, lower_inclusive); w_i32(r, upper_inclusive);
}

/* SELECT g, COUNT(*) FROM t WHERE price * quantity > 1000 AND NOT (div(a,b) IN (1, 2.5)) AND <long expression> = 0 GROUP BY g */
int main(void) {
  static char long_text[1500];
  record rec;
  char err[256];
  const char* in_values[2] = {"1", "2.5"};
  const char* eq_value[1] = {"0"};
  /* a text longer than any fixed buffer: plus(plus(...plus(c0,c1)...),cN) */
  size_t at = 0;
  for (int i = 1; i < 100; i++) at += (size_t)snprintf(long_text + at, sizeof long_text - at, "plus(");
  at += (size_t)snprintf(long_text + at, sizeof long_text - at, "c0");
  for (int i = 1; i < 100; i++) at += (size_t)snprintf(long_text + at, sizeof long_text - at, ",c%d)", i);
  rec.n = 0;
  w_i32(&rec, PGSHIM_QUERY_MAGIC); w_i32(&rec, 0); w_i32(&rec, 0); w_i32(&rec, 0);
  w_i32(&rec, 1); w_i32(&rec, 1); w_i32(&rec, 1); w_i32(&rec, 0);
  w_i32(&rec, 10); w_i32(&rec, -1);
  w_str(&rec, "g");
  w_i32(&rec, PG_AGG_COUNT); w_i32(&rec, 0); w_str(&rec, "*");
  w_i32(&rec, PG_FILTER_AND); w_i32(&rec, 3);
  w_predicate(&rec, PG_PRED_RANGE, "times(price,quantity)", 0, NULL, "1000", "*", 0, 0);
  w_i32(&rec, PG_FILTER_NOT); w_i32(&rec, 1);
  w_predicate(&rec, PG_PRED_IN, "div(a,b)", 2, in_values, NULL, NULL, 0, 0);
  w_predicate(&rec, PG_PRED_EQ, long_text, 1, eq_value, NULL, NULL, 0, 0);

  pgshim_query* nq = NULL;
  if (pgshim_query_parse(rec.b, rec.n, &nq, err, sizeof err) != PG_OK) { fprintf(stderr, "parse: %s\n", err); return 1; }
  const pg_query* q = pgshim_query_get(nq);
  const pg_filter_node* f = q->filter;
  if (!f || f->type != PG_FILTER_AND || f->n_children != 3) { fprintf(stderr, "root differs\n"); return 1; }
  const pg_filter_node* range = &f->children[0];
  if (range->type != PG_FILTER_PREDICATE || range->predicate_type != PG_PRED_RANGE || strcmp(range->column, "times(price,quantity)") != 0 ||
      strcmp(range->lower, "1000") != 0 || strcmp(range->upper, "*") != 0 || range->lower_inclusive || range->upper_inclusive || range->n_values != 0) {
    fprintf(stderr, "range leaf differs\n");
    return 1;
  }
  printf("an infix comparison round-trips as a RANGE over its canonical text\n");
  const pg_filter_node* not_node = &f->children[1];
  if (not_node->type != PG_FILTER_NOT || not_node->n_children != 1) { fprintf(stderr, "NOT differs\n"); return 1; }
  const pg_filter_node* in = &not_node->children[0];
  if (in->predicate_type != PG_PRED_IN || strcmp(in->column, "div(a,b)") != 0 || in->n_values != 2 || strcmp(in->values[0], "1") != 0 ||
      strcmp(in->values[1], "2.5") != 0 || in->lower != NULL || in->upper != NULL) {
    fprintf(stderr, "IN leaf differs\n");
    return 1;
  }
  printf("an IN list over a function call round-trips under NOT\n");
  const pg_filter_node* eq = &f->children[2];
  if (eq->predicate_type != PG_PRED_EQ || strlen(eq->column) != strlen(long_text) || strcmp(eq->column, long_text) != 0 || strlen(long_text) < 900 ||
      strcmp(eq->values[0], "0") != 0) {
    fprintf(stderr, "long text differs\n");
    return 1;
  }
  printf("a text of %d bytes round-trips whole\n", (int)strlen(long_text));
  pgshim_query_free(nq);
  /* every truncation fails cleanly */
  for (size_t cut = 40; cut < rec.n; cut++) {
    pgshim_query* bad = NULL;
    if (pgshim_query_parse(rec.b, cut, &bad, err, sizeof err) == PG_OK) { fprintf(stderr, "truncated record accepted at %zu\n", cut); return 1; }
  }
  printf("a truncated record fails cleanly\n");
  printf("wire format ok\n");
  return 0;
}
