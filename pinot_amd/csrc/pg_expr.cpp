// Parser of the expression texts of pg_expr.h (host code only; see the header for the grammar and the program's meaning).
#include "pg_expr.h"

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <charconv>
#include <cmath>

#include "../../include/pinot_gpu.h"

namespace pg {
namespace {

constexpr int kMaxDepth = PG_EXPR_MAX_OPS + 1;   // nested calls: deeper ones could only be literal-only (every other call costs an operation)

struct Value {
  bool literal = false;
  double v = 0;
  int32_t ref = 0;           // column index, or PG_EXPR_MAX_SRCS + dst
  bool cond = false;         // the result of a comparison or of a logical call (1.0 / 0.0)
  int32_t case_index = -1;   // the result of a CASE: its entry in ExprProgram::cases
  int32_t lit_type = PG_EXPR_T_DOUBLE;   // a literal's ExprType (a folded call: DOUBLE; PG_EXPR_T_STRING: a quoted text that is no number)
  int64_t ival = 0;
  bool is_null = false;      // the literal 'null' where an ELSE may stand
  std::string text;          // a literal directly under equals / not_equals, as written
};
// where an argument stands
struct Context {
  bool cond_ok = false;      // a WHEN, or an argument of and / or / not inside one: a comparison or a logical call may stand here
  bool text_ok = false;      // directly under equals / not_equals: a quoted literal keeps its text
  bool null_ok = false;      // a CASE's argument at an even position: 'null' is the omitted ELSE
};

struct Parser {
  const char* s;
  size_t n, i = 0;
  ExprProgram& out;
  std::string& error;
  int32_t status = PG_OK;
  int32_t n_nodes = 0;

  Parser(const char* text, ExprProgram& o, std::string& e) : s(text), n(strlen(text)), out(o), error(e) {}

  bool fail(int32_t st, const std::string& msg) {
    if (status == PG_OK) { status = st; error = msg; }
    return false;
  }
  std::string shown(size_t from, size_t to) const {   // a piece of the text for a message, cut to a readable length
    std::string t(s + from, to - from);
    if (t.size() > 64) t = t.substr(0, 61) + "...";
    return t;
  }
  void skip_ws() { while (i < n && (s[i] == ' ' || s[i] == '\t' || s[i] == '\n' || s[i] == '\r')) i++; }
  static bool delimiter(char c) { return c == '(' || c == ')' || c == ',' || c == '\'' || c == ' ' || c == '\t' || c == '\n' || c == '\r'; }

  // 0: a finite decimal number; 1: not decimal notation (or empty); 2: not a finite number
  static int number_kind(const std::string& t, double& v) {
    if (t.empty()) return 1;
    for (char c : t)   // decimal notation only: no "inf", "nan" or hexadecimal floats
      if (!((c >= '0' && c <= '9') || c == '+' || c == '-' || c == '.' || c == 'e' || c == 'E')) return 1;
    // std::from_chars: correctly rounded like Double.parseDouble and, unlike strtod, blind to the process locale (it takes no leading '+')
    const char* first = t.c_str() + (t[0] == '+' ? 1 : 0);
    const char* last = t.c_str() + t.size();
    v = 0;
    const std::from_chars_result r = std::from_chars(first, last, v);
    if (first == last || r.ptr != last || r.ec != std::errc() || !std::isfinite(v)) return 2;
    return 0;
  }
  bool number(const std::string& t, double& v) {
    if (t.empty()) return fail(PG_ERR_INVALID_ARGUMENT, "expression: an empty literal");
    switch (number_kind(t, v)) {
      case 0: return true;
      case 1: return fail(PG_ERR_INVALID_ARGUMENT, "expression: the literal '" + shown_text(t) + "' is not a decimal number");
      default: return fail(PG_ERR_INVALID_ARGUMENT, "expression: the literal '" + shown_text(t) + "' is not a finite number");
    }
  }
  static std::string shown_text(const std::string& t) { return t.size() > 64 ? t.substr(0, 61) + "..." : t; }
  // RequestUtils.getLiteral: an integer-looking text within int is INT, within long LONG; any other number is DOUBLE
  static void type_literal(const std::string& t, Value& v) {
    v.lit_type = PG_EXPR_T_DOUBLE;
    v.ival = 0;
    const size_t from = !t.empty() && (t[0] == '+' || t[0] == '-') ? 1 : 0;
    if (t.size() == from) return;
    for (size_t k = from; k < t.size(); k++) if (t[k] < '0' || t[k] > '9') return;
    long long x = 0;
    const std::from_chars_result r = std::from_chars(t.c_str() + (t[0] == '+' ? 1 : 0), t.c_str() + t.size(), x);
    if (r.ec != std::errc() || r.ptr != t.c_str() + t.size()) return;   // beyond long
    v.ival = x;
    v.lit_type = x >= INT32_MIN && x <= INT32_MAX ? PG_EXPR_T_INT : PG_EXPR_T_LONG;
  }
  bool literal_value(const std::string& t, Value& v) {
    v.literal = true;
    if (!number(t, v.v)) return false;
    type_literal(t, v);
    return true;
  }

  pg_expr_step* new_step(int32_t op, int32_t dst) {
    if (out.n_steps >= PG_EXPR_MAX_OPS) {
      fail(PG_ERR_UNSUPPORTED, "expression with more than " + std::to_string(PG_EXPR_MAX_OPS) + " operations");
      return nullptr;
    }
    pg_expr_step& st = out.steps[out.n_steps++];
    st.op = op;
    st.dst = dst;
    st.a = st.b = st.c = -1;
    st.pad = 0;
    st.lit = st.lit2 = 0.0;
    return &st;
  }
  bool step(int32_t op, int32_t dst, const Value& a, const Value& b) {
    pg_expr_step* st = new_step(op, dst);
    if (!st) return false;
    st->a = a.literal ? -1 : a.ref;
    st->b = b.literal ? -1 : b.ref;
    st->lit = a.literal ? a.v : (b.literal ? b.v : 0.0);
    return true;
  }

  bool argument(int depth, const Context& ctx, Value& v) {
    skip_ws();
    if (i < n && s[i] == '\'') {   // a quoted literal
      const size_t from = ++i;
      while (i < n && s[i] != '\'') i++;
      if (i >= n) return fail(PG_ERR_INVALID_ARGUMENT, "expression: unterminated quote");
      const std::string t(s + from, i - from);
      i++;
      v.literal = true;
      if (ctx.null_ok && t == "null") {   // CaseTransformFunction#init: no ELSE
        v.is_null = true;
        v.v = 0.0;
        return true;
      }
      if (ctx.text_ok) {
        v.text = t;
        if (number_kind(t, v.v) != 0) {   // kept as text: the planner looks it up in a STRING column's dictionary
          v.v = 0.0;
          v.lit_type = PG_EXPR_T_STRING;
          return true;
        }
        type_literal(t, v);
        return true;
      }
      return literal_value(t, v);
    }
    const size_t from = i;
    while (i < n && !delimiter(s[i])) i++;
    if (i == from) return fail(PG_ERR_INVALID_ARGUMENT, i < n ? "expression: an empty argument at '" + shown(i, n) + "'" : std::string("expression: the text ends inside an argument list"));
    const size_t to = i;
    skip_ws();
    if (i < n && s[i] == '(') {   // a nested call
      i = from;
      return call(depth + 1, ctx, v);
    }
    const std::string t(s + from, to - from);
    const char c = t[0];
    if ((c >= '0' && c <= '9') || c == '-' || c == '+' || c == '.') {
      if (ctx.text_ok) v.text = t;
      return literal_value(t, v);
    }
    size_t k = 0;
    while (k < out.columns.size() && out.columns[k] != t) k++;
    if (k == out.columns.size()) {
      if (k >= PG_EXPR_MAX_SRCS) return fail(PG_ERR_UNSUPPORTED, "expression over more than " + std::to_string(PG_EXPR_MAX_SRCS) + " distinct columns");
      out.columns.push_back(t);
    }
    v.literal = false;
    v.ref = (int32_t)k;
    return true;
  }

  // ',' (true, more arguments) or ')' (false, the list ends) behind an argument; anything else fails
  bool more_arguments(bool& more) {
    skip_ws();
    if (i < n && s[i] == ',') { i++; more = true; return true; }
    if (i < n && s[i] == ')') { i++; more = false; return true; }
    return fail(PG_ERR_INVALID_ARGUMENT, i < n ? "expression: ',' or ')' expected at '" + shown(i, n) + "'" : std::string("expression: unbalanced parentheses"));
  }

  static int32_t comparison_of(const std::string& name) {
    if (name == "equals") return PG_EXPR_EQ;
    if (name == "notequals") return PG_EXPR_NE;
    if (name == "greaterthan") return PG_EXPR_GT;
    if (name == "greaterthanorequal") return PG_EXPR_GE;
    if (name == "lessthan") return PG_EXPR_LT;
    if (name == "lessthanorequal") return PG_EXPR_LE;
    return -1;
  }

  bool condition_allowed(const Context& ctx, const std::string& name) {
    if (ctx.cond_ok) return true;
    return fail(PG_ERR_UNSUPPORTED, "expression: " + name + " outside a WHEN (a comparison or a logical call is the condition of a CASE, nothing else, on the GPU path)");
  }

  // equals(a,b) ... less_than_or_equal(a,b)
  bool comparison(int depth, int32_t op, const std::string& name, Value& v) {
    Context ctx;
    ctx.text_ok = op == PG_EXPR_EQ || op == PG_EXPR_NE;
    Value args[2];
    int n_args = 0;
    for (bool more = true; more;) {
      Value a;
      if (!argument(depth, ctx, a)) return false;
      if (n_args < 2) args[n_args] = a;
      n_args++;
      if (!more_arguments(more)) return false;
    }
    if (n_args != 2) return fail(PG_ERR_INVALID_ARGUMENT, "expression: " + name + " takes exactly 2 arguments, " + std::to_string(n_args) + " given");
    if (args[0].literal && args[1].literal) return fail(PG_ERR_UNSUPPORTED, "expression: " + name + " over two literals (the reference folds it before a segment sees it)");
    ExprComparison rec;
    for (int k = 0; k < 2; k++) {
      const Value& x = args[k];
      const Value& other = args[1 - k];
      if (x.case_index >= 0) return fail(PG_ERR_UNSUPPORTED, "expression: a CASE as an operand of " + name);
      if (x.literal) {
        if (x.lit_type == PG_EXPR_T_STRING && (other.literal || other.ref >= PG_EXPR_MAX_SRCS))   // only a column can turn out to be a STRING
          return fail(PG_ERR_INVALID_ARGUMENT, "expression: the literal '" + shown_text(x.text) + "' is not a decimal number");
        rec.literal = k;
        rec.literal_type = x.lit_type;
        rec.ival = x.ival;
        rec.text = x.text;
      } else if (x.ref < PG_EXPR_MAX_SRCS) {
        rec.column[k] = x.ref;
      }
    }
    const int32_t dst = n_nodes++;
    rec.step = out.n_steps;
    if (!step(op, dst, args[0], args[1])) return false;
    out.comparisons.push_back(std::move(rec));
    out.conditional = true;
    v.literal = false;
    v.cond = true;
    v.ref = PG_EXPR_MAX_SRCS + dst;
    return true;
  }

  // and(c1,c2,...) / or(c1,c2,...) / not(c)
  bool logical(int depth, int32_t op, const std::string& name, Value& v) {
    Context ctx;
    ctx.cond_ok = true;
    std::vector<Value> args;
    for (bool more = true; more;) {
      Value a;
      if (!argument(depth, ctx, a)) return false;
      if (!a.cond) return fail(PG_ERR_UNSUPPORTED, "expression: " + name + " over a column, a literal or a value (comparisons and logical calls are its operands on the GPU path)");
      if (args.size() < (size_t)PG_EXPR_MAX_OPS + 2) args.push_back(a);   // (beyond that the steps run out below)
      if (!more_arguments(more)) return false;
    }
    if (op == PG_EXPR_NOT ? args.size() != 1 : args.size() < 2)
      return fail(PG_ERR_INVALID_ARGUMENT, "expression: " + name + " takes " + (op == PG_EXPR_NOT ? "exactly 1 argument, " : "2 or more arguments, ") + std::to_string(args.size()) + " given");
    const int32_t dst = n_nodes++;
    Value acc = args[0];
    if (op == PG_EXPR_NOT) {
      if (!step(op, dst, acc, acc)) return false;
    } else {
      for (size_t k = 1; k < args.size(); k++) {
        if (!step(op, dst, acc, args[k])) return false;
        acc.ref = PG_EXPR_MAX_SRCS + dst;
      }
    }
    out.conditional = true;
    v.literal = false;
    v.cond = true;
    v.ref = PG_EXPR_MAX_SRCS + dst;
    return true;
  }

  // case(when1,then1,...,whenN,thenN,else)
  bool case_call(int depth, Value& v) {
    std::vector<Value> whens, thens;
    Value otherwise;
    int n_args = 0;
    for (bool more = true; more;) {
      Context ctx;
      const bool even = n_args % 2 == 0;
      ctx.cond_ok = even;    // a WHEN — or the ELSE, which the end of the list tells
      ctx.null_ok = even;
      Value a;
      if (!argument(depth, ctx, a)) return false;
      if (!more_arguments(more)) return false;
      n_args++;
      if (!even) {
        thens.push_back(a);
      } else if (more) {
        if (!a.cond) return fail(PG_ERR_UNSUPPORTED, "expression: a WHEN that is no comparison or logical call (argument " + std::to_string(n_args) + " of case)");
        whens.push_back(a);
      } else {
        if (a.cond) return fail(PG_ERR_UNSUPPORTED, "expression: a comparison or a logical call as the ELSE of a CASE");
        otherwise = a;
      }
      if (whens.size() > (size_t)PG_EXPR_MAX_OPS) return fail(PG_ERR_UNSUPPORTED, "expression with more than " + std::to_string(PG_EXPR_MAX_OPS) + " operations");
    }
    if (n_args % 2 == 0 || n_args < 3)
      return fail(PG_ERR_INVALID_ARGUMENT, "expression: case takes an odd number of arguments, 3 or more (when1,then1,...,else), " + std::to_string(n_args) + " given");
    ExprCase rec;
    rec.has_else = !otherwise.is_null;
    auto branch_of = [](const Value& x) {
      ExprBranch b;
      if (x.literal) { b.kind = ExprBranch::LITERAL; b.ref = x.lit_type; b.ival = x.ival; }
      else if (x.case_index >= 0) { b.kind = ExprBranch::CASE; b.ref = x.case_index; }
      else if (x.ref < PG_EXPR_MAX_SRCS) { b.kind = ExprBranch::COLUMN; b.ref = x.ref; }
      else b.kind = ExprBranch::ARITHMETIC;
      return b;
    };
    for (const Value& x : thens) rec.branches.push_back(branch_of(x));
    if (rec.has_else) rec.branches.push_back(branch_of(otherwise));
    const int32_t dst = n_nodes++;
    const size_t N = whens.size();
    for (size_t k = N; k-- > 0;) {   // from the last WHEN backwards: the first true one is written last
      pg_expr_step* st = new_step(PG_EXPR_SELECT, dst);
      if (!st) return false;
      const int32_t at = out.n_steps - 1;
      st->a = whens[k].ref;
      st->b = thens[k].literal ? -1 : thens[k].ref;
      st->lit = thens[k].literal ? thens[k].v : 0.0;
      rec.branches[k].step = at;
      rec.branches[k].slot = 0;
      if (k + 1 == N) {
        st->c = otherwise.literal ? -1 : otherwise.ref;
        st->lit2 = otherwise.literal ? otherwise.v : 0.0;   // ('null': 0.0, NullValuePlaceHolder.DOUBLE)
        if (rec.has_else) { rec.branches[N].step = at; rec.branches[N].slot = 1; }
      } else {
        st->c = PG_EXPR_MAX_SRCS + dst;
      }
    }
    out.cases.push_back(std::move(rec));
    out.conditional = true;
    v.literal = false;
    v.ref = PG_EXPR_MAX_SRCS + dst;
    v.case_index = (int32_t)out.cases.size() - 1;
    return true;
  }

  bool call(int depth, const Context& ctx, Value& v) {
    if (depth > kMaxDepth) return fail(PG_ERR_UNSUPPORTED, "expression nested deeper than " + std::to_string(kMaxDepth) + " calls");
    skip_ws();
    const size_t from = i;
    while (i < n && !delimiter(s[i])) i++;
    std::string name;
    for (size_t k = from; k < i; k++) {
      const char c = s[k];
      if (c == '_') continue;   // FunctionContext canonicalises names: no underscores, lower case
      name.push_back(c >= 'A' && c <= 'Z' ? (char)(c - 'A' + 'a') : c);
    }
    skip_ws();
    if (name.empty() || i >= n || s[i] != '(') return fail(PG_ERR_INVALID_ARGUMENT, "expression: a function call expected at '" + shown(from, n) + "'");
    i++;
    int32_t op;
    if (name == "add" || name == "plus") op = PG_EXPR_ADD;
    else if (name == "sub" || name == "minus") op = PG_EXPR_SUB;
    else if (name == "mult" || name == "times") op = PG_EXPR_MULT;
    else if (name == "div" || name == "divide") op = PG_EXPR_DIV;
    else if (name == "case") return case_call(depth, v);
    else if (comparison_of(name) >= 0) return condition_allowed(ctx, name) && comparison(depth, comparison_of(name), name, v);
    else if (name == "and" || name == "or" || name == "not") return condition_allowed(ctx, name) && logical(depth, name == "and" ? PG_EXPR_AND : name == "or" ? PG_EXPR_OR : PG_EXPR_NOT, name, v);
    else return fail(PG_ERR_UNSUPPORTED, "expression: the function " + shown_text(name) + " (add, sub, mult, div and plus, minus, times, divide run on the GPU path)");
    Value args[2];                 // sub / div: both; add / mult: the running value
    const bool nary = op == PG_EXPR_ADD || op == PG_EXPR_MULT;
    double lit = nary && op == PG_EXPR_MULT ? 1.0 : 0.0;
    std::vector<Value> others;     // add / mult: the non-literal arguments in argument order
    int n_args = 0;
    for (bool more = true; more;) {
      Value a;
      if (!argument(depth, Context(), a)) return false;
      if (nary) {
        if (a.literal) lit = op == PG_EXPR_ADD ? lit + a.v : lit * a.v;
        else others.push_back(a);
      } else if (n_args < 2) {
        args[n_args] = a;
      }
      n_args++;
      if (!more_arguments(more)) return false;
    }
    if (nary ? n_args < 2 : n_args != 2)
      return fail(PG_ERR_INVALID_ARGUMENT, "expression: " + name + " takes " + (nary ? "2 or more" : "exactly 2") + " arguments, " + std::to_string(n_args) + " given");
    if (nary) {
      if (others.empty()) { v.literal = true; v.v = lit; return true; }
      const int32_t dst = n_nodes++;
      Value acc;
      acc.literal = true;
      acc.v = lit;
      for (const Value& x : others) {
        if (!step(op, dst, acc, x)) return false;
        acc.literal = false;
        acc.ref = PG_EXPR_MAX_SRCS + dst;
      }
      v = Value();
      v.ref = acc.ref;
      return true;
    }
    if (args[0].literal && args[1].literal) {
      v.literal = true;
      v.v = op == PG_EXPR_SUB ? args[0].v - args[1].v : args[0].v / args[1].v;
      return true;
    }
    const int32_t dst = n_nodes++;
    if (!step(op, dst, args[0], args[1])) return false;
    v.literal = false;
    v.ref = PG_EXPR_MAX_SRCS + dst;
    return true;
  }
};

}  // namespace

int32_t expr_split_arguments(const char* text, std::vector<ExprArgument>& out, std::string& error) {
  out.clear();
  error.clear();
  auto bad = [&](const std::string& msg) { out.clear(); error = msg; return (int32_t)PG_ERR_INVALID_ARGUMENT; };
  if (!text) return bad("argument list: null text");
  ExprProgram unused;
  Parser p(text, unused, error);   // the lexer's blanks and delimiters
  for (;;) {
    p.skip_ws();
    ExprArgument arg;
    if (p.i < p.n && p.s[p.i] == '\'') {   // a quoted literal
      const size_t from = ++p.i;
      while (p.i < p.n && p.s[p.i] != '\'') p.i++;
      if (p.i >= p.n) return bad("argument list: unterminated quote");
      arg.text.assign(p.s + from, p.i - from);
      arg.quoted = true;
      p.i++;
    } else {
      const size_t from = p.i;
      int depth = 0;
      for (; p.i < p.n; p.i++) {
        const char c = p.s[p.i];
        if (c == '\'') {   // a literal inside a nested call
          p.i++;
          while (p.i < p.n && p.s[p.i] != '\'') p.i++;
          if (p.i >= p.n) return bad("argument list: unterminated quote");
        } else if (c == '(') {
          depth++;
        } else if (c == ')') {
          if (--depth < 0) return bad("argument list: unbalanced parentheses");
        } else if (c == ',' && depth == 0) {
          break;
        }
      }
      if (depth != 0) return bad("argument list: unbalanced parentheses");
      size_t to = p.i;
      while (to > from && (p.s[to - 1] == ' ' || p.s[to - 1] == '\t' || p.s[to - 1] == '\n' || p.s[to - 1] == '\r')) to--;
      if (to == from) return bad("argument list: an empty argument");
      arg.text.assign(p.s + from, to - from);
    }
    out.push_back(std::move(arg));
    p.skip_ws();
    if (p.i >= p.n) return PG_OK;
    if (p.s[p.i] != ',') return bad("argument list: ',' expected at '" + p.shown(p.i, p.n) + "'");
    p.i++;
  }
}

int32_t expr_parse(const char* text, ExprProgram& out, std::string& error) {
  out.columns.clear();
  out.n_steps = 0;
  out.conditional = false;
  out.cases.clear();
  out.comparisons.clear();
  error.clear();
  if (!text) { error = "expression: null text"; return PG_ERR_INVALID_ARGUMENT; }
  Parser p(text, out, error);
  Value v;
  if (p.call(1, Context(), v)) {
    p.skip_ws();
    if (p.i < p.n) p.fail(PG_ERR_INVALID_ARGUMENT, "expression: trailing text '" + p.shown(p.i, p.n) + "'");
    else if (v.literal || out.columns.empty()) p.fail(PG_ERR_INVALID_ARGUMENT, "expression without a column (the reference folds literal-only expressions before they reach a segment)");
  }
  if (p.status != PG_OK) { out.columns.clear(); out.n_steps = 0; out.conditional = false; out.cases.clear(); out.comparisons.clear(); }
  return p.status;
}

}  // namespace pg
