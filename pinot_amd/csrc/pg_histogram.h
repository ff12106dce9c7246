// HISTOGRAM (HistogramAggregationFunction.java; shared by the kernels of pg_kernels_hist.hip, the executor pg_exec_hist.hip and a
// stand-alone host harness, tests/histogram_main.cpp).  Plain C++ over include/pinot_gpu.h without HIP types, usable from host and device:
//   the argument list   pg_agg_spec.column of a PG_AGG_HISTOGRAM: "x,'lower','upper','numBins'" or "x,arrayvalueconstructor(e0,e1,...)",
//                       every edge quoted, or bare for Infinity / -Infinity; commas split at depth 0, blanks are ignored (hist_parse_arguments)
//   the bin specification   kind, lower, upper, binLength, edges (pg_hist_spec: what a kernel reads; HistSpec: what the host keeps)
//   pg_hist_bin         the single statement of getBinId: a bin, PG_HIST_NONE, or one of the two inputs on which the reference throws
// The equal-width bin is floor((val - lower) / binLength): two separately rounded IEEE operations, never contracted and never a multiply
// by a reciprocal.  Contraction is off inside pg_hist_bin (and in the whole of pg_kernels_hist.hip, through pg_expr_device.h).
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/pinot_gpu.h"

#if defined(__HIPCC__)
#define PG_HIST_FN __host__ __device__ static inline
#else
#define PG_HIST_FN static inline
#endif

#define PG_HIST_MAX_BINS 65536   // bins of one histogram
#define PG_HIST_MAX_SPECS 4      // distinct (column, bin specification) pairs of one query

enum pg_hist_kind : int32_t { PG_HIST_EQUAL_WIDTH = 0, PG_HIST_EDGES = 1 };
// what pg_hist_bin returns besides a bin
enum : int32_t {
  PG_HIST_NONE = -1,           // val > upper || val < lower: INVALID_BIN
  PG_HIST_THROWS_NAN = -2,     // a NaN: the edge form's search walks to index numBins, where incrementElement's checkState throws
  PG_HIST_THROWS_INDEX = -3    // an equal-width index that rounds up to numBins: HISTOGRAM(x, 0, 1, 3) over 0.9999999999999999
};

struct pg_hist_spec {
  int32_t kind;          // pg_hist_kind
  int32_t n_bins;
  double lower, upper;
  double bin_length;     // equal width: (upper - lower) / numBins, in double
  const double* edges;   // the edge form: n_bins + 1 strictly increasing edges
};

// getBinId(val); `val` is the column's value as getDoubleValuesSV gives it (an INT exact, a LONG (double)-rounded, a FLOAT widened exactly)
PG_HIST_FN int32_t pg_hist_bin(const pg_hist_spec& s, double val) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (val != val) return PG_HIST_THROWS_NAN;
  if (val > s.upper || val < s.lower) return PG_HIST_NONE;
  if (val == s.upper) return s.n_bins - 1;
  if (s.kind == PG_HIST_EQUAL_WIDTH) {
#if defined(__HIP_DEVICE_COMPILE__)
    const double f = floor(__ddiv_rn(__dsub_rn(val, s.lower), s.bin_length));
#else
    const volatile double d = val - s.lower;   // (volatile: the two operations stay two, whatever the host compiler's flags)
    const double f = floor(d / s.bin_length);
#endif
    // Java's (int): NaN is 0 (an overflowing upper - lower), the rest saturates; lower <= val < upper keeps f at or above 0
    if (f != f) return 0;
    if (f >= (double)s.n_bins) return PG_HIST_THROWS_INDEX;
    return (int32_t)f;
  }
  int32_t i = 0, j = s.n_bins;   // the reference's search: the largest i with edges[i] <= val
  while (i < j) {
    const int32_t mid = (i + j + 1) / 2;
    if (s.edges[mid] > val) j = mid - 1;
    else i = mid;
  }
  return i;
}

// ---- the host's half: the argument list and the specification it names --------------------------------------------------------------------
namespace pg {

struct HistSpec {
  std::string column;          // the first argument as given (a column, or an expression's text: the executor refuses that)
  int32_t kind = PG_HIST_EQUAL_WIDTH;
  int32_t n_bins = 0;
  double lower = 0, upper = 0, bin_length = 0;
  std::vector<double> edges;   // the edge form only
  bool same_bins(const HistSpec& o) const {
    return kind == o.kind && n_bins == o.n_bins && lower == o.lower && upper == o.upper && edges == o.edges;
  }
  pg_hist_spec device(const double* edges_at) const { return pg_hist_spec{kind, n_bins, lower, upper, bin_length, edges_at}; }
};

namespace hist_detail {
struct Argument { std::string text; bool quoted = false; };
inline bool blank(char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r'; }
// `text` split at its commas of depth 0; blanks outside quotes dropped; a quoted literal loses its quotes
inline bool split(const std::string& text, std::vector<Argument>& out, std::string& error) {
  out.clear();
  Argument cur;
  int depth = 0;
  bool any = false;
  for (size_t i = 0; i < text.size(); i++) {
    const char c = text[i];
    if (c == '\'') {
      if (depth == 0 && (!cur.text.empty() || cur.quoted)) { error = "text next to a quoted literal"; return false; }
      size_t j = i + 1;
      while (j < text.size() && text[j] != '\'') cur.text.push_back(text[j++]);
      if (j >= text.size()) { error = "unterminated quote"; return false; }
      if (depth == 0) cur.quoted = true;   // (inside parentheses the literal stays part of its argument's text, without its quotes)
      i = j;
      any = true;
      continue;
    }
    if (blank(c)) continue;
    if (c == ',' && depth == 0) {
      if (cur.text.empty() && !cur.quoted) { error = "empty argument"; return false; }
      out.push_back(cur);
      cur = Argument();
      continue;
    }
    if (cur.quoted && depth == 0) { error = "text next to a quoted literal"; return false; }
    if (c == '(') depth++;
    if (c == ')' && --depth < 0) { error = "unbalanced parentheses"; return false; }
    cur.text.push_back(c);
    any = true;
  }
  if (depth != 0) { error = "unbalanced parentheses"; return false; }
  if (!any) { error = "empty argument list"; return false; }
  if (cur.text.empty() && !cur.quoted) { error = "empty argument"; return false; }
  out.push_back(cur);
  return true;
}
// Double.parseDouble of a literal's text: decimal numbers, Infinity / -Infinity / NaN spelled as Java spells them
inline bool number(const std::string& t, double& v) {
  if (t == "Infinity" || t == "+Infinity") { v = INFINITY; return true; }
  if (t == "-Infinity") { v = -INFINITY; return true; }
  if (t == "NaN") { v = NAN; return true; }
  if (t.empty()) return false;
  for (char c : t) if (!((c >= '0' && c <= '9') || c == '.' || c == '-' || c == '+' || c == 'e' || c == 'E')) return false;
  char* end = nullptr;
  v = strtod(t.c_str(), &end);
  return end && *end == 0 && end != t.c_str();
}
// Double.toString for the messages' %s: integral values below 10^7 as "1000.0", the rest by the shortest digits that read back
inline std::string java_double(double v) {
  char buf[40];
  if (v != v) return "NaN";
  if (v == INFINITY) return "Infinity";
  if (v == -INFINITY) return "-Infinity";
  if (v == floor(v) && fabs(v) < 1e7) { snprintf(buf, sizeof(buf), "%.1f", v); return buf; }
  for (int prec = 1; prec <= 17; prec++) { snprintf(buf, sizeof(buf), "%.*g", prec, v); if (strtod(buf, nullptr) == v) break; }
  return buf;
}
}  // namespace hist_detail

// The specification `text` names.  PG_OK, or PG_ERR_INVALID_ARGUMENT with the reference's message in `error` (an argument count other than
// 2 or 4, a second argument that is no array, fewer than 2 edges, edges not strictly increasing, upper <= lower, numBins <= 0, a bound that
// is no number) and for a malformed list.
inline int32_t hist_parse_arguments(const char* text, HistSpec& out, std::string& error) {
  using namespace hist_detail;
  out = HistSpec();
  error.clear();
  if (!text) { error = "HISTOGRAM needs its argument list"; return PG_ERR_INVALID_ARGUMENT; }
  std::vector<Argument> args;
  if (!split(text, args, error)) { error = "HISTOGRAM(" + std::string(text) + "): " + error; return PG_ERR_INVALID_ARGUMENT; }
  if (args.size() != 2 && args.size() != 4) {
    error = "Histogram expects 2 or 4 arguments, got: " + std::to_string(args.size()) +
            "; usage example: `Histogram(columnName, ARRAY[0,1,10,100])` to specify bins [0,1), [1,10), [10,1000] or "
            "`Histogram(columnName, 0, 1000, 10)` to specify 10 equal-length bins [0,100), [100,200), ..., [900,1000]";
    return PG_ERR_INVALID_ARGUMENT;
  }
  if (args[0].quoted) { error = "HISTOGRAM: the first argument must be a column, not the literal '" + args[0].text + "'"; return PG_ERR_INVALID_ARGUMENT; }
  out.column = args[0].text;
  auto not_a_number = [&](const std::string& t) { error = "For input string: \"" + t + "\""; return (int32_t)PG_ERR_INVALID_ARGUMENT; };
  if (args.size() == 2) {
    static const char kArray[] = "arrayvalueconstructor(";
    const std::string& a = args[1].text;
    if (args[1].quoted || a.size() < sizeof(kArray) || a.compare(0, sizeof(kArray) - 1, kArray) != 0 || a.back() != ')') {
      error = "Please use the format of `Histogram(columnName, ARRAY[1,10,100])` to specify the bin edges";
      return PG_ERR_INVALID_ARGUMENT;
    }
    std::vector<Argument> edges;
    const std::string inner = a.substr(sizeof(kArray) - 1, a.size() - sizeof(kArray));
    if (!inner.empty() && !split(inner, edges, error)) { error = "HISTOGRAM(" + std::string(text) + "): " + error; return PG_ERR_INVALID_ARGUMENT; }
    if (edges.size() < 2) { error = "The number of bin edges must be greater than 1"; return PG_ERR_INVALID_ARGUMENT; }
    for (size_t i = 0; i < edges.size(); i++) {
      double v = 0;
      if (!number(edges[i].text, v)) return not_a_number(edges[i].text);
      if (i > 0 && !(v > out.edges.back())) { error = "The bin edges must be strictly increasing"; return PG_ERR_INVALID_ARGUMENT; }
      out.edges.push_back(v);
    }
    out.kind = PG_HIST_EDGES;
    out.n_bins = (int32_t)(out.edges.size() - 1);
    out.lower = out.edges.front();
    out.upper = out.edges.back();
    return PG_OK;
  }
  double bins = 0;
  if (!number(args[1].text, out.lower)) return not_a_number(args[1].text);
  if (!number(args[2].text, out.upper)) return not_a_number(args[2].text);
  if (!number(args[3].text, bins) || bins != floor(bins) || fabs(bins) > 2147483647.0) return not_a_number(args[3].text);
  if (!(out.upper > out.lower)) {
    error = "The right most edge must be greater than left most edge, given " + java_double(out.lower) + " and " + java_double(out.upper);
    return PG_ERR_INVALID_ARGUMENT;
  }
  if (!(bins > 0)) { error = "The number of bins must be greater than zero, given " + std::to_string((long long)bins); return PG_ERR_INVALID_ARGUMENT; }
  out.kind = PG_HIST_EQUAL_WIDTH;
  out.n_bins = (int32_t)bins;
  {
    const volatile double width = out.upper - out.lower;
    out.bin_length = width / (double)out.n_bins;
  }
  return PG_OK;
}

// What the GPU path leaves to the Java plan: PG_OK, or PG_ERR_UNSUPPORTED with the reason in `error`
inline int32_t hist_spec_supported(const HistSpec& s, std::string& error) {
  if (s.kind == PG_HIST_EQUAL_WIDTH && (isinf(s.lower) || isinf(s.upper) || s.lower != s.lower || s.upper != s.upper)) {
    error = "HISTOGRAM with equal-width bins between non-finite bounds (" + hist_detail::java_double(s.lower) + ", " + hist_detail::java_double(s.upper) + ")";
    return PG_ERR_UNSUPPORTED;
  }
  if (s.n_bins > PG_HIST_MAX_BINS) {
    error = "HISTOGRAM with " + std::to_string(s.n_bins) + " bins: more than " + std::to_string(PG_HIST_MAX_BINS) + " bins in one histogram";
    return PG_ERR_UNSUPPORTED;
  }
  return PG_OK;
}

}  // namespace pg
