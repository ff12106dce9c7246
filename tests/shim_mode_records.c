/* The NativeQuery wire format of MODE through the shim's C half (integration/jni/pinot_gpu_shim.c): the function id PG_AGG_MODE passes
 * through as an int — nothing range-checks it —, its argument list ("x" or "x,'MAX'") IS the column string, and it carries no parameter
 * bytes, so a record with it has no agg_params unless a PERCENTILE sits next to it; PG_QUERY_FLAG_FINAL_MODE travels in the flags word.
 * Compiled and run by tests/test_mode_query.py; prints one line per check and "wire format ok" at the end. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pinot_gpu.h"
#include "pinot_gpu_shim.h"

typedef struct { uint8_t b[1024]; size_t n; } record;
static void w_i32(record* r, int32_t v) { for (int i = 0; i < 4; i++) r->b[r->n++] = (uint8_t)((uint32_t)v >> (8 * i)); }
static void w_f64(record* r, double d) { uint64_t u; memcpy(&u, &d, 8); for (int i = 0; i < 8; i++) r->b[r->n++] = (uint8_t)(u >> (8 * i)); }
static void w_str(record* r, const char* s) {
  const size_t len = strlen(s);
  w_i32(r, (int32_t)len);
  memcpy(r->b + r->n, s, len);
  r->n += len;
  while (r->n & 3) r->b[r->n++] = 0;
}
static const char kPlain[] = "lat";
static const char kAvg[] = "lat,'AVG'";
/* SELECT g, MODE(lat), MODE(lat, 'AVG'), COUNT(*)[, PERCENTILE(lat, 99.9)] FROM t GROUP BY g, with PG_QUERY_FLAG_FINAL_MODE */
static void build(record* r, int with_percentile) {
  r->n = 0;
  w_i32(r, PGSHIM_QUERY_MAGIC); w_i32(r, PG_QUERY_FLAG_FINAL_MODE); w_i32(r, 0); w_i32(r, 0);
  w_i32(r, 1); w_i32(r, with_percentile ? 4 : 3); w_i32(r, 0); w_i32(r, 0);
  w_i32(r, 10); w_i32(r, -1);
  w_str(r, "g");
  w_i32(r, PG_AGG_MODE); w_i32(r, 0); w_str(r, kPlain);
  w_i32(r, PG_AGG_MODE); w_i32(r, 0); w_str(r, kAvg);
  w_i32(r, PG_AGG_COUNT); w_i32(r, 0); w_str(r, "*");
  if (with_percentile) { w_i32(r, PG_AGG_PERCENTILE); w_i32(r, 0); w_str(r, "lat"); w_f64(r, 99.9); }
}

int main(void) {
  record rec;
  char err[256];
  pgshim_query* nq = NULL;
  build(&rec, 0);
  if (pgshim_query_parse(rec.b, rec.n, &nq, err, sizeof err) != PG_OK) { fprintf(stderr, "parse: %s\n", err); return 1; }
  const pg_query* q = pgshim_query_get(nq);
  if (q->n_aggregations != 3 || q->agg_params != NULL || q->aggregations[0].function != 28 || q->aggregations[1].function != 28 ||
      q->aggregations[2].function != PG_AGG_COUNT || strcmp(q->aggregations[0].column, kPlain) != 0 || strcmp(q->aggregations[1].column, kAvg) != 0 ||
      strcmp(q->group_by_columns[0], "g") != 0 || (q->flags & PG_QUERY_FLAG_FINAL_MODE) == 0 || PG_QUERY_FLAG_FINAL_MODE != 0x400) {
    fprintf(stderr, "round trip differs\n");
    return 1;
  }
  pgshim_query_free(nq);
  printf("the function round-trips with its argument lists and without parameters\n");
  for (size_t cut = 40; cut < rec.n; cut++) {
    pgshim_query* bad = NULL;
    if (pgshim_query_parse(rec.b, cut, &bad, err, sizeof err) == PG_OK) { fprintf(stderr, "truncated record accepted at %zu\n", cut); return 1; }
  }
  printf("a truncated record fails cleanly\n");
  build(&rec, 1);
  nq = NULL;
  if (pgshim_query_parse(rec.b, rec.n, &nq, err, sizeof err) != PG_OK) { fprintf(stderr, "parse: %s\n", err); return 1; }
  q = pgshim_query_get(nq);
  if (q->n_aggregations != 4 || !q->agg_params || q->agg_params[3] != 99.9 || q->agg_params[0] != 0.0 || q->agg_params[1] != 0.0 ||
      q->aggregations[1].function != PG_AGG_MODE || q->aggregations[3].function != PG_AGG_PERCENTILE) {
    fprintf(stderr, "record with a percentile differs\n");
    return 1;
  }
  pgshim_query_free(nq);
  printf("a percentile next to it keeps its parameter\n");
  /* a trailing double behind a record whose last aggregation is a MODE is trailing bytes: it takes no parameter */
  rec.n = 0;
  w_i32(&rec, PGSHIM_QUERY_MAGIC); w_i32(&rec, 0); w_i32(&rec, 0); w_i32(&rec, 0);
  w_i32(&rec, 0); w_i32(&rec, 1); w_i32(&rec, 0); w_i32(&rec, 0);
  w_i32(&rec, 10); w_i32(&rec, -1);
  w_i32(&rec, PG_AGG_MODE); w_i32(&rec, 0); w_str(&rec, kPlain);
  w_f64(&rec, 1.0);
  nq = NULL;
  if (pgshim_query_parse(rec.b, rec.n, &nq, err, sizeof err) == PG_OK || !strstr(err, "trailing bytes")) { fprintf(stderr, "trailing bytes accepted\n"); return 1; }
  printf("a mode takes no parameter\n");
  printf("wire format ok\n");
  return 0;
}
