/* The NativeQuery wire format of an aggregation over a CASE through the shim's C half (integration/jni/pinot_gpu_shim.c): the canonical text
 * case(when1,then1,...,else) IS the column string of a plain SUM / MIN / AVG record — no new function id, no parameter bytes, no flag —, of any
 * length (the record's strings carry their own), with its quotes, commas and parentheses untouched.
 * Compiled and run by tests/test_case_query.py; prints one line per check and "wire format ok" at the end. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pinot_gpu.h"
#include "pinot_gpu_shim.h"

typedef struct { uint8_t b[8192]; size_t n; } record;
static void w_i32(record* r, int32_t v) { for (int i = 0; i < 4; i++) r->b[r->n++] = (uint8_t)((uint32_t)v >> (8 * i)); }
static void w_f64(record* r, double d) { uint64_t u; memcpy(&u, &d, 8); for (int i = 0; i < 8; i++) r->b[r->n++] = (uint8_t)(u >> (8 * i)); }
static void w_str(record* r, const char* s) {
  const size_t len = strlen(s);
  w_i32(r, (int32_t)len);
  memcpy(r->b + r->n, s, len);
  r->n += len;
  while (r->n & 3) r->b[r->n++] = 0;
}
static const char kCount[] = "case(equals(status,'ok'),'1','0')";
static const char kGuard[] = "case(and(notequals(b,'0'),or(greaterthan(a,'100'),not(lessthanorequal(a,b)))),divide(a,b),'null')";
static char kLong[4000];   /* fifteen operations' worth of text and a long string literal */
/* SELECT g, SUM(kCount), AVG(kGuard), MIN(kLong)[, PERCENTILE(lat, 99.9)] FROM t GROUP BY g */
static void build(record* r, int with_percentile) {
  r->n = 0;
  w_i32(r, PGSHIM_QUERY_MAGIC); w_i32(r, 0); w_i32(r, 0); w_i32(r, 0);
  w_i32(r, 1); w_i32(r, with_percentile ? 4 : 3); w_i32(r, 0); w_i32(r, 0);
  w_i32(r, 10); w_i32(r, -1);
  w_str(r, "g");
  w_i32(r, PG_AGG_SUM); w_i32(r, 0); w_str(r, kCount);
  w_i32(r, PG_AGG_AVG); w_i32(r, 0); w_str(r, kGuard);
  w_i32(r, PG_AGG_MIN); w_i32(r, 0); w_str(r, kLong);
  if (with_percentile) { w_i32(r, PG_AGG_PERCENTILE); w_i32(r, 0); w_str(r, "lat"); w_f64(r, 99.9); }
}

int main(void) {
  record rec;
  char err[256];
  pgshim_query* nq = NULL;
  strcpy(kLong, "case(equals(name,'");
  memset(kLong + strlen(kLong), 'x', 3000);
  strcat(kLong, "'),a,greaterthan(a,'5000'),a,'9999999')");
  build(&rec, 0);
  if (pgshim_query_parse(rec.b, rec.n, &nq, err, sizeof err) != PG_OK) { fprintf(stderr, "parse: %s\n", err); return 1; }
  const pg_query* q = pgshim_query_get(nq);
  if (q->n_aggregations != 3 || q->agg_params != NULL || q->flags != 0 || q->aggregations[0].function != PG_AGG_SUM || q->aggregations[1].function != PG_AGG_AVG ||
      q->aggregations[2].function != PG_AGG_MIN || strcmp(q->aggregations[0].column, kCount) != 0 || strcmp(q->aggregations[1].column, kGuard) != 0 ||
      strcmp(q->aggregations[2].column, kLong) != 0 || strlen(q->aggregations[2].column) < 3000 || strcmp(q->group_by_columns[0], "g") != 0) {
    fprintf(stderr, "round trip differs\n");
    return 1;
  }
  pgshim_query_free(nq);
  printf("the texts round-trip under the plain function ids, without parameters or flags\n");
  for (size_t cut = 40; cut < rec.n; cut += (cut < 400 || cut + 64 > rec.n ? 1 : 37)) {
    pgshim_query* bad = NULL;
    if (pgshim_query_parse(rec.b, cut, &bad, err, sizeof err) == PG_OK) { fprintf(stderr, "truncated record accepted at %zu\n", cut); return 1; }
  }
  printf("a truncated record fails cleanly\n");
  build(&rec, 1);
  nq = NULL;
  if (pgshim_query_parse(rec.b, rec.n, &nq, err, sizeof err) != PG_OK) { fprintf(stderr, "parse: %s\n", err); return 1; }
  q = pgshim_query_get(nq);
  if (q->n_aggregations != 4 || !q->agg_params || q->agg_params[3] != 99.9 || q->agg_params[0] != 0.0 || strcmp(q->aggregations[1].column, kGuard) != 0 ||
      q->aggregations[3].function != PG_AGG_PERCENTILE) {
    fprintf(stderr, "record with a percentile differs\n");
    return 1;
  }
  pgshim_query_free(nq);
  printf("a percentile next to them keeps its parameter\n");
  printf("wire format ok\n");
  return 0;
}
