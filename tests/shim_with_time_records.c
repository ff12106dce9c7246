/* The NativeQuery wire format of FIRSTWITHTIME / LASTWITHTIME through the shim's C half (integration/jni/pinot_gpu_shim.c): the function ids
 * PG_AGG_FIRSTWITHTIME / PG_AGG_LASTWITHTIME pass through as ints — nothing range-checks them — and the argument list "x,t,'TYPE'" passes
 * through as the aggregation's column string, commas and quotes included; the functions carry no parameter.  Compiled and run by
 * tests/test_with_time_query.py; prints one line per check and "wire format ok" at the end. */
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
/* SELECT g, FIRSTWITHTIME(m, ts, 'INT'), LASTWITHTIME(lat, ts, 'DOUBLE'), COUNT(*) FROM t GROUP BY g */
static void build(record* r) {
  r->n = 0;
  w_i32(r, PGSHIM_QUERY_MAGIC); w_i32(r, 0); w_i32(r, 0); w_i32(r, 0);
  w_i32(r, 1); w_i32(r, 3); w_i32(r, 0); w_i32(r, 0);
  w_i32(r, 10); w_i32(r, -1);
  w_str(r, "g");
  w_i32(r, PG_AGG_FIRSTWITHTIME); w_i32(r, 0); w_str(r, "m,ts,'INT'");
  w_i32(r, PG_AGG_LASTWITHTIME); w_i32(r, 0); w_str(r, "lat,ts,'DOUBLE'");
  w_i32(r, PG_AGG_COUNT); w_i32(r, 0); w_str(r, "*");
}

int main(void) {
  record rec;
  char err[256];
  pgshim_query* nq = NULL;
  build(&rec);
  if (pgshim_query_parse(rec.b, rec.n, &nq, err, sizeof err) != PG_OK) { fprintf(stderr, "parse: %s\n", err); return 1; }
  const pg_query* q = pgshim_query_get(nq);
  if (q->n_aggregations != 3 || q->agg_params != NULL || q->aggregations[0].function != 21 || q->aggregations[1].function != 22 ||
      strcmp(q->aggregations[0].column, "m,ts,'INT'") != 0 || strcmp(q->aggregations[1].column, "lat,ts,'DOUBLE'") != 0 ||
      q->aggregations[2].function != PG_AGG_COUNT || strcmp(q->group_by_columns[0], "g") != 0) {
    fprintf(stderr, "round trip differs\n");
    return 1;
  }
  pgshim_query_free(nq);
  printf("ids 21 / 22 and their argument lists arrive unchanged\n");
  for (size_t cut = 40; cut < rec.n; cut++) {
    pgshim_query* bad = NULL;
    if (pgshim_query_parse(rec.b, cut, &bad, err, sizeof err) == PG_OK) { fprintf(stderr, "truncated record accepted at %zu\n", cut); return 1; }
  }
  printf("a truncated record fails cleanly\n");
  /* a trailing double behind the record is trailing bytes: the functions take no parameter */
  build(&rec);
  w_f64(&rec, 1.0);
  nq = NULL;
  if (pgshim_query_parse(rec.b, rec.n, &nq, err, sizeof err) == PG_OK || !strstr(err, "trailing bytes")) { fprintf(stderr, "trailing bytes accepted\n"); return 1; }
  printf("the functions take no parameter\n");
  printf("wire format ok\n");
  return 0;
}
