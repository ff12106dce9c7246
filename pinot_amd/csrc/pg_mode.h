// MODE (ModeAggregationFunction.java; shared by the kernels of pg_kernels_mode.hip, the executor pg_exec_percentile.hip and a stand-alone
// host harness, tests/mode_main.cpp).  Plain C++ over include/pinot_gpu.h without HIP types:
//   the argument list   pg_agg_spec.column of a PG_AGG_MODE: "x" or "x,'MAX'" — commas split at depth 0, blanks are ignored; the reducer is
//                       MultiModeReducerType.valueOf's: exactly MIN, MAX or AVG (mode_parse_arguments, host only)
//   the selection's partial   (max_count, n_tied, lowest tied id, highest tied id) over a range of ids, and its combine rule
//                       (pg_mode_combine, host and device): the single statement of "the most frequent ids of a row"
//   mode_exact_sum      AVG's sum: the exact sum of the tied keys as doubles, rounded once (host only)
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/pinot_gpu.h"

#if defined(__HIPCC__)
#define PG_MODE_FN __host__ __device__ static inline
#else
#define PG_MODE_FN static inline
#endif

enum pg_mode_reducer : int32_t { PG_MODE_MIN = 0, PG_MODE_MAX = 1, PG_MODE_AVG = 2 };

// The most frequent ids of a range of ids.  Ids whose count is 0 are not in the map: a range without a counted id is the identity
// {0, 0, 0xFFFFFFFF, 0}.  n_tied ids share max_count; lo / hi are the lowest and the highest of them.
struct pg_mode_partial {
  uint32_t max_count;
  uint32_t n_tied;
  uint32_t lo, hi;
};

PG_MODE_FN pg_mode_partial pg_mode_identity() { return pg_mode_partial{0u, 0u, 0xFFFFFFFFu, 0u}; }

// the partial of one id
PG_MODE_FN pg_mode_partial pg_mode_of(uint32_t id, uint32_t count) { return count ? pg_mode_partial{count, 1u, id, id} : pg_mode_identity(); }

// Associative and commutative: the greater count wins; equal counts add n_tied and take min / max of the ids.  (Two identities combine to
// the identity: 0 ties, min / max of the sentinels.)
PG_MODE_FN pg_mode_partial pg_mode_combine(const pg_mode_partial& a, const pg_mode_partial& b) {
  if (a.max_count > b.max_count) return a;
  if (b.max_count > a.max_count) return b;
  return pg_mode_partial{a.max_count, a.n_tied + b.n_tied, a.lo < b.lo ? a.lo : b.lo, a.hi > b.hi ? a.hi : b.hi};
}

// ---- the host's half -------------------------------------------------------------------------------------------------------------------------
namespace pg {

struct ModeSpec {
  std::string column;                  // the first argument as given (a column, or an expression's text: the executor refuses that)
  int32_t reducer = PG_MODE_MIN;       // pg_mode_reducer
};

namespace mode_detail {
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
      if (depth == 0) cur.quoted = true;
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
}  // namespace mode_detail

// PG_OK, or PG_ERR_INVALID_ARGUMENT with the reason in `error` — the reference's text where it has one
inline int32_t mode_parse_arguments(const char* text, ModeSpec& out, std::string& error) {
  std::vector<mode_detail::Argument> args;
  if (!mode_detail::split(text ? text : "", args, error)) return PG_ERR_INVALID_ARGUMENT;
  if (args.size() > 2) {
    error = "Mode expects at most 2 arguments, got: " + std::to_string(args.size());
    return PG_ERR_INVALID_ARGUMENT;
  }
  if (args[0].quoted) { error = "MODE: the first argument must be a column"; return PG_ERR_INVALID_ARGUMENT; }
  out.column = args[0].text;
  out.reducer = PG_MODE_MIN;
  if (args.size() == 2) {
    if (!args[1].quoted) { error = "MODE: the second argument must be a quoted MultiModeReducerType ('MIN', 'MAX' or 'AVG'), got " + args[1].text; return PG_ERR_INVALID_ARGUMENT; }
    const std::string& r = args[1].text;   // valueOf: the exact upper-case name
    if (r == "MIN") out.reducer = PG_MODE_MIN;
    else if (r == "MAX") out.reducer = PG_MODE_MAX;
    else if (r == "AVG") out.reducer = PG_MODE_AVG;
    else {
      error = "No enum constant org.apache.pinot.core.query.aggregation.function.ModeAggregationFunction.MultiModeReducerType." + r;
      return PG_ERR_INVALID_ARGUMENT;
    }
  }
  return PG_OK;
}

// The exact sum of `v` rounded to nearest-even once.  A NaN among them, or infinities of both signs, give NaN; else an infinity gives
// itself.  Finite values go into a two's-complement fixed-point accumulator of 64-bit limbs that spans every double's bits (bit 0 is
// 2^-1074) with 64 bits of headroom: up to 2^63 addends cannot overflow it.
inline double mode_exact_sum(const double* v, size_t n) {
  constexpr int kLimbs = 34;   // 2 176 bits >= 1074 + 1024 + 64
  uint64_t acc[kLimbs];
  memset(acc, 0, sizeof(acc));
  bool nan = false, pinf = false, ninf = false;
  for (size_t i = 0; i < n; i++) {
    const double x = v[i];
    if (x != x) { nan = true; continue; }
    if (x == INFINITY) { pinf = true; continue; }
    if (x == -INFINITY) { ninf = true; continue; }
    uint64_t u;
    memcpy(&u, &x, 8);
    const int e = (int)((u >> 52) & 0x7FF);
    uint64_t m = u & ((1ULL << 52) - 1);
    if (e) m |= 1ULL << 52;
    if (!m) continue;
    const int shift = e ? e - 1 : 0;   // the mantissa's bit 0 is 2^(shift - 1074)
    const int limb = shift / 64, off = shift % 64;
    uint64_t part[2] = {m << off, off ? m >> (64 - off) : 0};
    if (!(u >> 63)) {
      unsigned carry = 0;
      for (int k = limb; k < kLimbs; k++) {
        const uint64_t add = k - limb < 2 ? part[k - limb] : 0;
        if (k - limb >= 2 && !carry) break;
        const uint64_t s = acc[k] + add, s2 = s + carry;
        carry = (s < add) || (s2 < s);
        acc[k] = s2;
      }
    } else {
      unsigned borrow = 0;
      for (int k = limb; k < kLimbs; k++) {
        const uint64_t sub = k - limb < 2 ? part[k - limb] : 0;
        if (k - limb >= 2 && !borrow) break;
        const uint64_t d = acc[k] - sub, d2 = d - borrow;
        borrow = (acc[k] < sub) || (d < borrow);
        acc[k] = d2;
      }
    }
  }
  if (nan || (pinf && ninf)) return NAN;
  if (pinf) return INFINITY;
  if (ninf) return -INFINITY;
  const bool neg = (acc[kLimbs - 1] >> 63) != 0;
  if (neg) {   // the magnitude
    unsigned carry = 1;
    for (int k = 0; k < kLimbs; k++) {
      const uint64_t s = ~acc[k] + carry;
      carry = carry && s == 0;
      acc[k] = s;
    }
  }
  int top = -1;   // the highest set bit
  for (int k = kLimbs - 1; k >= 0 && top < 0; k--)
    if (acc[k]) top = k * 64 + 63 - __builtin_clzll(acc[k]);
  if (top < 0) return 0.0;   // (an exact zero sum: +0.0, as a running sum of cancelling terms gives)
  auto bit = [&](int b) { return b >= 0 && ((acc[b / 64] >> (b % 64)) & 1); };
  double r;
  if (top <= 52) {   // subnormal or the smallest normals: exact
    r = ldexp((double)acc[0], -1074);
  } else {
    uint64_t m = 0;
    for (int b = top; b > top - 53; b--) m = (m << 1) | (bit(b) ? 1u : 0u);
    const int below = top - 53;   // the round bit
    bool sticky = false;
    for (int b = below - 1; b >= 0 && !sticky; b--) {
      if (b % 64 == 63 && !acc[b / 64]) { b -= 63; continue; }
      sticky = bit(b);
    }
    if (bit(below) && (sticky || (m & 1))) m++;   // (m may become 2^53: ldexp keeps that exact)
    r = ldexp((double)m, top - 52 - 1074);        // beyond the largest double: infinity
  }
  return neg ? -r : r;
}

}  // namespace pg
