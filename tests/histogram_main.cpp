// pinot_amd/csrc/pg_histogram.h as a stand-alone host program (built with -fsanitize=address,undefined by tests/test_histogram_host.py and run
// directly): the argument-list parser, the GPU path's own limits and pg_hist_bin, line by line from stdin.
//   P <argument list>     parses it: "ok <kind> <numBins> <lower> <upper> <binLength> <edges...>" (doubles as 16 hex digits of their bits; the
//                         first argument behind "x="), or "err <status> <message>"; the specification stays current
//   S                     the current specification under hist_spec_supported: "supported" or "unsupported <message>"
//   B <bits> <bits> ...   pg_hist_bin of every value under the current specification: the bins (-1 none, -2 / -3 the throwing inputs)
// Prints "histogram ok" at the end of the input.
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include <iostream>
#include <sstream>
#include <string>

#include "../pinot_amd/csrc/pg_histogram.h"

static std::string bits(double v) {
  uint64_t u;
  memcpy(&u, &v, 8);
  char buf[24];
  snprintf(buf, sizeof(buf), "%016" PRIx64, u);
  return buf;
}

int main() {
  pg::HistSpec spec;
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    if (line[0] == 'P') {
      std::string error;
      const int32_t st = pg::hist_parse_arguments(line.size() > 2 ? line.c_str() + 2 : "", spec, error);
      if (st != PG_OK) { printf("err %d %s\n", st, error.c_str()); continue; }
      printf("ok %d %d %s %s %s x=%s", spec.kind, spec.n_bins, bits(spec.lower).c_str(), bits(spec.upper).c_str(), bits(spec.bin_length).c_str(), spec.column.c_str());
      for (double e : spec.edges) printf(" %s", bits(e).c_str());
      printf("\n");
    } else if (line[0] == 'S') {
      std::string error;
      if (pg::hist_spec_supported(spec, error) == PG_OK) printf("supported\n");
      else printf("unsupported %s\n", error.c_str());
    } else if (line[0] == 'B') {
      const pg_hist_spec s = spec.device(spec.edges.data());
      std::istringstream in(line.substr(1));
      std::string tok;
      bool first = true;
      while (in >> tok) {
        const uint64_t u = strtoull(tok.c_str(), nullptr, 16);
        double v;
        memcpy(&v, &u, 8);
        printf(first ? "%d" : " %d", pg_hist_bin(s, v));
        first = false;
      }
      printf("\n");
    } else {
      fprintf(stderr, "bad line: %s\n", line.c_str());
      return 2;
    }
  }
  printf("histogram ok\n");
  return 0;
}
