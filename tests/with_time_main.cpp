// Stand-alone harness over pinot_amd/csrc/pg_with_time.h (plain C++, no HIP): the order keys, the packed bound and the pack / unpack round
// trip the kernels of pg_kernels_withtime.hip and the executor share.  Built with -fsanitize=address,undefined and run by
// tests/test_with_time_host.py, which compares every line with tests/with_time_model.py.  Reads commands from stdin, one per line:
//   K                                  -> K <PG_WT_MAX_SLOTS> <PG_WT_MAX_AGGS> <PG_WT_LDS_SLOTS>
//   D <n_docs>                         -> D <doc bits>
//   O <t> <first>                      -> O <order key, hex> <the time the key decodes to>
//   E <tmin> <tmax> <D>                -> E <range, hex> <largest admitted range, hex> <eligible 0/1>
//   P <tmin> <tmax> <t> <doc> <D> <first> -> P <packed, hex> <doc> <rel, hex> <time>      (eligible ranges only)
// and prints "with_time ok" at the end.
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../pinot_amd/csrc/pg_with_time.h"

int main() {
  char line[512];
  std::vector<uint64_t> seen;   // (heap use under the sanitizer: every packed value is kept and checked non-zero at the end)
  while (fgets(line, sizeof line, stdin)) {
    long long a = 0, b = 0, c = 0;
    unsigned long long doc = 0;
    int d = 0, first = 0;
    if (line[0] == 'K') {
      printf("K %d %d %d\n", PG_WT_MAX_SLOTS, PG_WT_MAX_AGGS, PG_WT_LDS_SLOTS);
    } else if (sscanf(line, "D %lld", &a) == 1) {
      printf("D %d\n", pg_wt_doc_bits((int64_t)a));
    } else if (sscanf(line, "O %lld %d", &a, &first) == 2) {
      const uint64_t key = pg_wt_order_key((int64_t)a, first);
      printf("O %016" PRIx64 " %" PRId64 "\n", key, pg_wt_time_of_key(key, first));
    } else if (sscanf(line, "E %lld %lld %d", &a, &b, &d) == 3) {
      const uint64_t range = pg_wt_range((int64_t)a, (int64_t)b);
      printf("E %016" PRIx64 " %016" PRIx64 " %d\n", range, pg_wt_packed_max_range(d), pg_wt_packed_ok(range, d));
    } else if (sscanf(line, "P %lld %lld %lld %llu %d %d", &a, &b, &c, &doc, &d, &first) == 6) {
      if (!pg_wt_packed_ok(pg_wt_range((int64_t)a, (int64_t)b), d)) { fprintf(stderr, "not eligible: %s", line); return 1; }
      const int64_t base = first ? (int64_t)b : (int64_t)a;
      const uint64_t rel = pg_wt_rel((int64_t)c, base, first);
      const uint64_t v = pg_wt_pack(rel, (uint32_t)doc, d);
      seen.push_back(v);
      printf("P %016" PRIx64 " %u %016" PRIx64 " %" PRId64 "\n", v, pg_wt_packed_doc(v, d), pg_wt_packed_rel(v, d), pg_wt_time_of_rel(pg_wt_packed_rel(v, d), base, first));
    } else {
      fprintf(stderr, "bad line: %s", line);
      return 1;
    }
  }
  for (uint64_t v : seen) if (v == 0) { fprintf(stderr, "a packed value of 0 (reserved for \"no doc\")\n"); return 1; }
  printf("with_time ok\n");
  return 0;
}
