/* The NativeQuery wire format of a PERCENTILE aggregation through the shim's C half (integration/jni/pinot_gpu_shim.c): an aggregation whose
 * function is PG_AGG_PERCENTILE carries one 8-byte little-endian double right after its column string; records without one are unchanged.
 * Compiled and run by tests/test_percentile_wire_format.py; prints one line per check and "wire format ok" at the end. */
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
/* SELECT g, COUNT(*), PERCENTILE(lat, 99.9), SUM(m), PERCENTILE(lat2, 50) FROM t GROUP BY g; with_percentiles = 0: COUNT(*) and SUM(m) only */
static size_t build(record* r, int with_percentiles, size_t* first_double_at) {
  r->n = 0;
  w_i32(r, PGSHIM_QUERY_MAGIC); w_i32(r, 0); w_i32(r, 0); w_i32(r, 0);
  w_i32(r, 1); w_i32(r, with_percentiles ? 4 : 2); w_i32(r, 0); w_i32(r, 0);
  w_i32(r, 10); w_i32(r, -1);
  w_str(r, "g");
  w_i32(r, PG_AGG_COUNT); w_i32(r, 0); w_str(r, "*");
  if (with_percentiles) { w_i32(r, PG_AGG_PERCENTILE); w_i32(r, 0); w_str(r, "lat"); *first_double_at = r->n; w_f64(r, 99.9); }
  w_i32(r, PG_AGG_SUM); w_i32(r, 0); w_str(r, "m");
  if (with_percentiles) { w_i32(r, PG_AGG_PERCENTILE); w_i32(r, 0); w_str(r, "lat2"); w_f64(r, 50.0); }
  return r->n;
}

int main(void) {
  record rec;
  char err[256];
  size_t at = 0;
  pgshim_query* nq = NULL;
  build(&rec, 1, &at);
  if (pgshim_query_parse(rec.b, rec.n, &nq, err, sizeof err) != PG_OK) { fprintf(stderr, "parse: %s\n", err); return 1; }
  const pg_query* q = pgshim_query_get(nq);
  if (q->n_aggregations != 4 || !q->agg_params || q->agg_params[1] != 99.9 || q->agg_params[3] != 50.0 || q->agg_params[0] != 0.0 ||
      q->aggregations[1].function != PG_AGG_PERCENTILE || strcmp(q->aggregations[1].column, "lat") != 0 ||
      q->aggregations[2].function != PG_AGG_SUM || strcmp(q->aggregations[3].column, "lat2") != 0 || strcmp(q->group_by_columns[0], "g") != 0) {
    fprintf(stderr, "round trip differs\n");
    return 1;
  }
  pgshim_query_free(nq);
  printf("two percentiles round-trip into agg_params\n");
  /* every truncation fails cleanly, the ones inside the first double among them */
  for (size_t cut = 40; cut < rec.n; cut++) {
    pgshim_query* bad = NULL;
    if (pgshim_query_parse(rec.b, cut, &bad, err, sizeof err) == PG_OK) { fprintf(stderr, "truncated record accepted at %zu\n", cut); return 1; }
    if (cut > at && cut < at + 8 && !strstr(err, "truncated")) { fprintf(stderr, "cut %zu: %s\n", cut, err); return 1; }
  }
  printf("a truncated double fails cleanly\n");
  /* a trailing double behind a record that has no PERCENTILE is trailing bytes */
  build(&rec, 0, &at);
  nq = NULL;
  if (pgshim_query_parse(rec.b, rec.n, &nq, err, sizeof err) != PG_OK) { fprintf(stderr, "parse: %s\n", err); return 1; }
  q = pgshim_query_get(nq);
  if (q->n_aggregations != 2 || q->agg_params != NULL || q->aggregations[1].function != PG_AGG_SUM) { fprintf(stderr, "plain record differs\n"); return 1; }
  pgshim_query_free(nq);
  w_f64(&rec, 1.0);
  nq = NULL;
  if (pgshim_query_parse(rec.b, rec.n, &nq, err, sizeof err) == PG_OK || !strstr(err, "trailing bytes")) { fprintf(stderr, "trailing bytes accepted\n"); return 1; }
  printf("a record without a percentile is unchanged\n");
  printf("wire format ok\n");
  return 0;
}
