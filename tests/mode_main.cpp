// pinot_amd/csrc/pg_mode.h as a stand-alone host program (built with -fsanitize=address,undefined by tests/test_mode_host.py and run
// directly): the argument-list parser, the selection's combine rule and AVG's exact sum, line by line from stdin.
//   P <argument list>                  parses it: "ok <reducer> x=<column>" or "err <status> <message>"
//   C <cut> <cut> ... | <count> ...    the row of counts cut into chunks at the given ids: every chunk's partial by pg_mode_of /
//                                      pg_mode_combine over its ids, then the chunks' partials combined — "<max_count> <n_tied> <lo> <hi>",
//                                      or "none" for a row without a counted id
//   S <bits> <bits> ...                mode_exact_sum of the doubles (16 hex digits of their bits each): the sum's bits
// Prints "mode ok" at the end of the input.
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../pinot_amd/csrc/pg_mode.h"

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    if (line[0] == 'P') {
      pg::ModeSpec spec;
      std::string error;
      const int32_t st = pg::mode_parse_arguments(line.size() > 2 ? line.c_str() + 2 : "", spec, error);
      if (st != PG_OK) printf("err %d %s\n", st, error.c_str());
      else printf("ok %d x=%s\n", spec.reducer, spec.column.c_str());
    } else if (line[0] == 'C') {
      std::istringstream in(line.substr(1));
      std::vector<uint32_t> cuts, counts;
      std::string tok;
      bool after = false;
      while (in >> tok) {
        if (tok == "|") { after = true; continue; }
        (after ? counts : cuts).push_back((uint32_t)strtoul(tok.c_str(), nullptr, 10));
      }
      cuts.push_back((uint32_t)counts.size());
      pg_mode_partial row = pg_mode_identity();
      uint32_t at = 0;
      for (uint32_t cut : cuts) {
        pg_mode_partial chunk = pg_mode_identity();
        for (; at < cut && at < counts.size(); at++) chunk = pg_mode_combine(chunk, pg_mode_of(at, counts[at]));
        row = pg_mode_combine(row, chunk);
      }
      if (row.n_tied == 0) printf("none\n");
      else printf("%u %u %u %u\n", row.max_count, row.n_tied, row.lo, row.hi);
    } else if (line[0] == 'S') {
      std::istringstream in(line.substr(1));
      std::vector<double> v;
      std::string tok;
      while (in >> tok) {
        const uint64_t u = strtoull(tok.c_str(), nullptr, 16);
        double d;
        memcpy(&d, &u, 8);
        v.push_back(d);
      }
      const double s = pg::mode_exact_sum(v.data(), v.size());
      uint64_t u;
      memcpy(&u, &s, 8);
      printf("%016" PRIx64 "\n", u);
    } else {
      fprintf(stderr, "bad line: %s\n", line.c_str());
      return 2;
    }
  }
  printf("mode ok\n");
  return 0;
}
