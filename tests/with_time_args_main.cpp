// Stand-alone harness over expr_split_arguments (pinot_amd/csrc/pg_expr.cpp): the lexer behind the argument lists of aggregations with more
// than one argument (FIRSTWITHTIME / LASTWITHTIME: "x,t,'DOUBLE'").  Built with -fsanitize=address,undefined and run by
// tests/test_with_time_query.py: one text per line on stdin; per text "<status> <n>" and the arguments as [text] (bare) or <text> (quoted).
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../pinot_amd/csrc/pg_expr.h"

int main() {
  char line[1024];
  while (fgets(line, sizeof line, stdin)) {
    size_t n = strlen(line);
    if (n && line[n - 1] == '\n') line[--n] = 0;
    std::vector<pg::ExprArgument> args;
    std::string error;
    const int32_t st = pg::expr_split_arguments(line, args, error);
    printf("%d %d", (int)st, (int)args.size());
    for (const pg::ExprArgument& a : args) printf(a.quoted ? " <%s>" : " [%s]", a.text.c_str());
    if (st != 0 && error.empty()) printf(" (no reason given)");
    printf("\n");
  }
  std::vector<pg::ExprArgument> args;
  std::string error;
  printf("%d null\n", (int)pg::expr_split_arguments(nullptr, args, error));
  printf("split ok\n");
  return 0;
}
