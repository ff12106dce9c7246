// Parser of the expression texts of pg_expr.h (host code only; see the header for the grammar and the program's meaning).
#include "pg_expr.h"

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
  int32_t ref = 0;   // column index, or PG_EXPR_MAX_SRCS + dst
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

  bool number(const std::string& t, double& v) {
    if (t.empty()) return fail(PG_ERR_INVALID_ARGUMENT, "expression: an empty literal");
    for (char c : t)   // decimal notation only: no "inf", "nan" or hexadecimal floats
      if (!((c >= '0' && c <= '9') || c == '+' || c == '-' || c == '.' || c == 'e' || c == 'E'))
        return fail(PG_ERR_INVALID_ARGUMENT, "expression: the literal '" + shown_text(t) + "' is not a decimal number");
    // std::from_chars: correctly rounded like Double.parseDouble and, unlike strtod, blind to the process locale (it takes no leading '+')
    const char* first = t.c_str() + (t[0] == '+' ? 1 : 0);
    const char* last = t.c_str() + t.size();
    v = 0;
    const std::from_chars_result r = std::from_chars(first, last, v);
    if (first == last || r.ptr != last || r.ec != std::errc() || !std::isfinite(v))
      return fail(PG_ERR_INVALID_ARGUMENT, "expression: the literal '" + shown_text(t) + "' is not a finite number");
    return true;
  }
  static std::string shown_text(const std::string& t) { return t.size() > 64 ? t.substr(0, 61) + "..." : t; }

  bool step(int32_t op, int32_t dst, const Value& a, const Value& b) {
    if (out.n_steps >= PG_EXPR_MAX_OPS)
      return fail(PG_ERR_UNSUPPORTED, "expression with more than " + std::to_string(PG_EXPR_MAX_OPS) + " operations");
    pg_expr_step& st = out.steps[out.n_steps++];
    st.op = op;
    st.dst = dst;
    st.a = a.literal ? -1 : a.ref;
    st.b = b.literal ? -1 : b.ref;
    st.lit = a.literal ? a.v : (b.literal ? b.v : 0.0);
    return true;
  }

  bool argument(int depth, Value& v) {
    skip_ws();
    if (i < n && s[i] == '\'') {   // a quoted literal
      const size_t from = ++i;
      while (i < n && s[i] != '\'') i++;
      if (i >= n) return fail(PG_ERR_INVALID_ARGUMENT, "expression: unterminated quote");
      const std::string t(s + from, i - from);
      i++;
      v.literal = true;
      return number(t, v.v);
    }
    const size_t from = i;
    while (i < n && !delimiter(s[i])) i++;
    if (i == from) return fail(PG_ERR_INVALID_ARGUMENT, i < n ? "expression: an empty argument at '" + shown(i, n) + "'" : std::string("expression: the text ends inside an argument list"));
    const size_t to = i;
    skip_ws();
    if (i < n && s[i] == '(') {   // a nested call
      i = from;
      return call(depth + 1, v);
    }
    const std::string t(s + from, to - from);
    const char c = t[0];
    if ((c >= '0' && c <= '9') || c == '-' || c == '+' || c == '.') {
      v.literal = true;
      return number(t, v.v);
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

  bool call(int depth, Value& v) {
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
    else return fail(PG_ERR_UNSUPPORTED, "expression: the function " + shown_text(name) + " (add, sub, mult, div and plus, minus, times, divide run on the GPU path)");
    Value args[2];                 // sub / div: both; add / mult: the running value
    const bool nary = op == PG_EXPR_ADD || op == PG_EXPR_MULT;
    double lit = nary && op == PG_EXPR_MULT ? 1.0 : 0.0;
    std::vector<Value> others;     // add / mult: the non-literal arguments in argument order
    int n_args = 0;
    for (;;) {
      Value a;
      if (!argument(depth, a)) return false;
      if (nary) {
        if (a.literal) lit = op == PG_EXPR_ADD ? lit + a.v : lit * a.v;
        else others.push_back(a);
      } else if (n_args < 2) {
        args[n_args] = a;
      }
      n_args++;
      skip_ws();
      if (i < n && s[i] == ',') { i++; continue; }
      if (i < n && s[i] == ')') { i++; break; }
      return fail(PG_ERR_INVALID_ARGUMENT, i < n ? "expression: ',' or ')' expected at '" + shown(i, n) + "'" : std::string("expression: unbalanced parentheses"));
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
      v = acc;
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
  error.clear();
  if (!text) { error = "expression: null text"; return PG_ERR_INVALID_ARGUMENT; }
  Parser p(text, out, error);
  Value v;
  if (p.call(1, v)) {
    p.skip_ws();
    if (p.i < p.n) p.fail(PG_ERR_INVALID_ARGUMENT, "expression: trailing text '" + p.shown(p.i, p.n) + "'");
    else if (v.literal || out.columns.empty()) p.fail(PG_ERR_INVALID_ARGUMENT, "expression without a column (the reference folds literal-only expressions before they reach a segment)");
  }
  if (p.status != PG_OK) { out.columns.clear(); out.n_steps = 0; }
  return p.status;
}

}  // namespace pg
