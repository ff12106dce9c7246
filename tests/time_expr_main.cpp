// Stand-alone driver of the time-bucket transform parser (pinot_amd/csrc/pg_time_expr.cpp) and of the per-value function the kernel shares
// (pg_time_eval, pinot_amd/csrc/pg_time_program.h), built with -fsanitize=address,undefined by tests/test_time_expr.py.
//   time_expr_main TEXTS INPUTS
// TEXTS holds one text per line, INPUTS one long per line.  Every text is handed to the parser in a heap buffer of exactly its length, so that a
// read past the text is caught.  Per text one line "T <status> <family?> <column>|<error>", and for an accepted text one line "V" with
// the function's value for every input.  Then the reciprocal division is checked against the division it replaces, and "time expr ok" ends
// the output.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <string>
#include <vector>

#include "../include/pinot_gpu.h"
#include "../pinot_amd/csrc/pg_time_expr.h"

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s TEXTS INPUTS\n", argv[0]); return 2; }
  std::vector<std::string> texts;
  std::vector<int64_t> inputs;
  {
    std::ifstream f(argv[1]);
    for (std::string line; std::getline(f, line);) texts.push_back(line);
    std::ifstream g(argv[2]);
    for (std::string line; std::getline(g, line);) if (!line.empty()) inputs.push_back((int64_t)strtoll(line.c_str(), nullptr, 10));
  }
  if (texts.empty() || inputs.empty()) { fprintf(stderr, "no texts or no inputs\n"); return 2; }
  for (const std::string& text : texts) {
    char* exact = (char*)malloc(text.size() + 1);   // no slack behind the terminator
    memcpy(exact, text.c_str(), text.size() + 1);
    pg::TimeProgram tp;
    std::string error;
    const int32_t st = pg::time_expr_parse(exact, tp, error);
    const bool family = pg::time_expr_is_time_function(exact);
    free(exact);
    if ((st == PG_OK) != error.empty() || (st == PG_OK && tp.column.empty()) || (st != PG_OK && !tp.column.empty()) || error.size() > 512) {
      printf("FAIL inconsistent answer for %s\n", text.c_str());
      return 1;
    }
    printf("T %d %d %s\n", st, family ? 1 : 0, st == PG_OK ? tp.column.c_str() : error.c_str());
    if (st != PG_OK) continue;
    printf("V");
    for (int64_t x : inputs) printf(" %lld", (long long)pg_time_eval(tp.prog, x));
    printf("\n");
  }
  // the reciprocals against the divisions they replace: every divisor the family can produce and awkward ones, over the inputs
  const int64_t divisors[] = {1, -1, 2, -2, 3, 5, -5, 7, 10, 60, 1000, 60000, 900000, 3600000, 86400000, 604800000, 1000000, 1000000000LL, 60000000000LL,
                              3600000000000LL, 86400000000000LL, 2147483647, -2147483647 - 1LL, 4294967297LL, (1LL << 62), (1LL << 62) + 1, INT64_MAX,
                              INT64_MAX - 1, -INT64_MAX, INT64_MIN};
  int failures = 0;
  for (int64_t d : divisors) {
    const pg_time_divisor D = pg::time_divisor_of(d);
    for (int64_t n : inputs) {
      const int64_t want = (n == INT64_MIN && d == -1) ? INT64_MIN : n / d;
      const int64_t got = pg_time_div(n, D);
      if (got != want) { printf("FAIL %lld / %lld: %lld, want %lld\n", (long long)n, (long long)d, (long long)got, (long long)want); failures++; }
    }
  }
  if (failures) { printf("%d failures\n", failures); return 1; }
  printf("time expr ok\n");
  return 0;
}
