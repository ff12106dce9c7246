// Parser of the time-bucket transform texts of pg_time_expr.h (host code only; see the header for the family and pg_time_program.h for the
// normal form).
#include "pg_time_expr.h"

#include <string.h>

#include <charconv>
#include <vector>

#include "../../include/pinot_gpu.h"

namespace pg {
namespace {

std::string shown(const std::string& t) { return t.size() > 64 ? t.substr(0, 61) + "..." : t; }
std::string upper(std::string t) { for (char& c : t) if (c >= 'a' && c <= 'z') c = (char)(c - 'a' + 'A'); return t; }
std::string lower(std::string t) { for (char& c : t) if (c >= 'A' && c <= 'Z') c = (char)(c - 'A' + 'a'); return t; }

// the canonical name of the call at the head of `text` (FunctionContext: lower case, no underscores); empty when the text is no call
std::string head_name(const char* text, size_t* after = nullptr) {
  size_t i = 0;
  while (text[i] == ' ' || text[i] == '\t' || text[i] == '\n' || text[i] == '\r') i++;
  std::string name;
  for (; text[i] && text[i] != '(' && text[i] != ')' && text[i] != ',' && text[i] != '\'' && text[i] != ' ' && text[i] != '\t' && text[i] != '\n' && text[i] != '\r'; i++) {
    const char c = text[i];
    if (c == '_') continue;
    name.push_back(c >= 'A' && c <= 'Z' ? (char)(c - 'A' + 'a') : c);
  }
  while (text[i] == ' ' || text[i] == '\t' || text[i] == '\n' || text[i] == '\r') i++;
  if (text[i] != '(') return std::string();
  if (after) *after = i + 1;
  return name;
}

enum Family { F_NONE, F_TIMECONVERT, F_TOEPOCH, F_DATETIMECONVERT, F_DATETRUNC };
enum Variant { V_PLAIN, V_ROUNDED, V_BUCKET };
// TimeUnit's ordinals
enum Unit { U_NANOS, U_MICROS, U_MILLIS, U_SECONDS, U_MINUTES, U_HOURS, U_DAYS, U_CUSTOM, U_UNKNOWN };
const int64_t kUnitNanos[7] = {1LL, 1000LL, 1000000LL, 1000000000LL, 60000000000LL, 3600000000000LL, 86400000000000LL};

Family family_of(const std::string& name, Unit* unit, Variant* variant) {
  if (name == "timeconvert") return F_TIMECONVERT;
  if (name == "datetimeconvert") return F_DATETIMECONVERT;
  if (name == "datetrunc") return F_DATETRUNC;
  if (name.compare(0, 7, "toepoch") != 0) return F_NONE;
  std::string rest = name.substr(7);
  Variant v = V_PLAIN;
  auto ends = [&](const char* tail) {
    const size_t n = strlen(tail);
    if (rest.size() <= n || rest.compare(rest.size() - n, n, tail) != 0) return false;
    rest.resize(rest.size() - n);
    return true;
  };
  if (ends("rounded")) v = V_ROUNDED;
  else if (ends("bucket")) v = V_BUCKET;
  Unit u;
  if (rest == "seconds") u = U_SECONDS;
  else if (rest == "minutes") u = U_MINUTES;
  else if (rest == "hours") u = U_HOURS;
  else if (rest == "days") u = U_DAYS;
  else return F_NONE;
  if (unit) *unit = u;
  if (variant) *variant = v;
  return F_TOEPOCH;
}

// an upper-case TimeUnit name; WEEKS / MONTHS / YEARS are DateTimeTransformUnits only (U_CUSTOM)
Unit unit_of(const std::string& t) {
  static const char* names[7] = {"NANOSECONDS", "MICROSECONDS", "MILLISECONDS", "SECONDS", "MINUTES", "HOURS", "DAYS"};
  for (int k = 0; k < 7; k++) if (t == names[k]) return (Unit)k;
  if (t == "WEEKS" || t == "MONTHS" || t == "YEARS") return U_CUSTOM;
  return U_UNKNOWN;
}

// TimeUnit#convert(d, from) seen from `to`
pg_time_conv conv_of(Unit from, Unit to) {
  pg_time_conv c;
  memset(&c, 0, sizeof(c));
  const int64_t a = kUnitNanos[from], b = kUnitNanos[to];
  if (a == b) { c.kind = PG_TIME_CONV_SAME; return c; }
  if (a > b) {
    c.kind = PG_TIME_CONV_UP;
    c.mul = a / b;
    c.limit = INT64_MAX / c.mul;
  } else {
    c.kind = PG_TIME_CONV_DOWN;
    c.div = time_divisor_of(b / a);
  }
  return c;
}

struct Arg {
  enum Kind { QUOTED, BARE, CALL } kind = BARE;
  std::string text;
};

struct Parser {
  const char* s;
  size_t n, i = 0;
  std::string& error;
  int32_t status = PG_OK;
  Parser(const char* text, std::string& e) : s(text), n(strlen(text)), error(e) {}

  bool fail(int32_t st, const std::string& msg) {
    if (status == PG_OK) { status = st; error = "time function: " + msg; }
    return false;
  }
  void skip_ws() { while (i < n && (s[i] == ' ' || s[i] == '\t' || s[i] == '\n' || s[i] == '\r')) i++; }
  static bool delimiter(char c) { return c == '(' || c == ')' || c == ',' || c == '\'' || c == ' ' || c == '\t' || c == '\n' || c == '\r'; }

  // the arguments up to and including the closing parenthesis; a nested call is kept whole (its text only names it in a refusal)
  bool arguments(std::vector<Arg>& args) {
    for (;;) {
      Arg a;
      skip_ws();
      if (i < n && s[i] == '\'') {
        const size_t from = ++i;
        while (i < n && s[i] != '\'') i++;
        if (i >= n) return fail(PG_ERR_INVALID_ARGUMENT, "unterminated quote");
        a.kind = Arg::QUOTED;
        a.text.assign(s + from, i - from);
        i++;
      } else {
        const size_t from = i;
        while (i < n && !delimiter(s[i])) i++;
        if (i == from) return fail(PG_ERR_INVALID_ARGUMENT, i < n ? "an empty argument at '" + shown(std::string(s + i, n - i)) + "'" : std::string("the text ends inside the argument list"));
        size_t to = i;
        skip_ws();
        if (i < n && s[i] == '(') {   // a nested call: to its closing parenthesis, quotes respected
          int depth = 0;
          for (; i < n; i++) {
            if (s[i] == '\'') { i++; while (i < n && s[i] != '\'') i++; if (i >= n) break; continue; }
            if (s[i] == '(') depth++;
            else if (s[i] == ')' && --depth == 0) { i++; break; }
          }
          if (depth != 0 || i > n) return fail(PG_ERR_INVALID_ARGUMENT, "unbalanced parentheses");
          a.kind = Arg::CALL;
          to = i;
        }
        a.text.assign(s + from, to - from);
      }
      args.push_back(std::move(a));
      skip_ws();
      if (i < n && s[i] == ',') { i++; continue; }
      if (i < n && s[i] == ')') { i++; return true; }
      return fail(PG_ERR_INVALID_ARGUMENT, i < n ? "',' or ')' expected at '" + shown(std::string(s + i, n - i)) + "'" : std::string("unbalanced parentheses"));
    }
  }

  bool literal(const Arg& a, const char* what, std::string& t) {
    if (a.kind == Arg::CALL) return fail(PG_ERR_INVALID_ARGUMENT, std::string("the ") + what + " must be a literal, not " + shown(a.text));
    t = a.text;
    return true;
  }
  bool long_literal(const Arg& a, const char* what, int64_t& v) {
    std::string t;
    if (!literal(a, what, t)) return false;
    const char* first = t.c_str() + (!t.empty() && t[0] == '+' ? 1 : 0);
    const char* last = t.c_str() + t.size();
    v = 0;
    const std::from_chars_result r = std::from_chars(first, last, v);
    if (first == last || r.ptr != last || r.ec != std::errc()) return fail(PG_ERR_INVALID_ARGUMENT, std::string("the ") + what + " '" + shown(t) + "' is not a long");
    return true;
  }
  // the value argument: one plain column
  bool value(const Arg& a, const std::string& fn, std::string& column) {
    if (a.kind == Arg::CALL)
      return fail(PG_ERR_UNSUPPORTED, fn + " over the expression " + shown(a.text) + " (its value argument must be a plain column on the GPU path)");
    const char c = a.text.empty() ? '\0' : a.text[0];
    if (a.kind == Arg::QUOTED || (c >= '0' && c <= '9') || c == '-' || c == '+' || c == '.')
      return fail(PG_ERR_INVALID_ARGUMENT, "the value argument of " + fn + " is the literal '" + shown(a.text) + "', not a column");
    column = a.text;
    return true;
  }
  bool count(const std::string& fn, size_t got, size_t lo, size_t hi) {
    if (got >= lo && got <= hi) return true;
    std::string want = lo == hi ? "exactly " + std::to_string(lo) : std::to_string(lo) + " to " + std::to_string(hi);
    return fail(PG_ERR_INVALID_ARGUMENT, fn + " takes " + want + " arguments, " + std::to_string(got) + " given");
  }
  // a java.util.concurrent.TimeUnit by name; `custom_refused`: WEEKS / MONTHS / YEARS are PG_ERR_UNSUPPORTED instead of unknown
  bool time_unit(const std::string& name, const char* what, bool custom_refused, Unit& u) {
    u = unit_of(name);
    if (u == U_CUSTOM && custom_refused)
      return fail(PG_ERR_UNSUPPORTED, std::string("the ") + what + " " + name + " (WEEKS, MONTHS and YEARS are no java.util.concurrent.TimeUnit: the Java plan answers)");
    if (u == U_CUSTOM || u == U_UNKNOWN) return fail(PG_ERR_INVALID_ARGUMENT, std::string("unknown ") + what + " '" + shown(name) + "'");
    return true;
  }
  static std::vector<std::string> split(const std::string& t, char sep, size_t max) {
    std::vector<std::string> out;
    size_t from = 0;
    while (out.size() + 1 < max) {
      const size_t at = t.find(sep, from);
      if (at == std::string::npos) break;
      out.push_back(t.substr(from, at - from));
      from = at + 1;
    }
    out.push_back(t.substr(from));
    return out;
  }
  bool positive_int(const std::string& t, const std::string& in, int64_t& v) {
    int32_t x = 0;
    const std::from_chars_result r = std::from_chars(t.c_str(), t.c_str() + t.size(), x);
    if (t.empty() || r.ptr != t.c_str() + t.size() || r.ec != std::errc() || x <= 0) return fail(PG_ERR_INVALID_ARGUMENT, "invalid size '" + shown(t) + "' in '" + shown(in) + "' (a positive int)");
    v = x;
    return true;
  }
  // DateTimeFormatSpec, EPOCH only: size:UNIT:EPOCH or EPOCH|UNIT(|size)
  bool format(const std::string& f, const char* what, int64_t& size, Unit& unit) {
    if (f.empty()) return fail(PG_ERR_INVALID_ARGUMENT, std::string("empty ") + what);
    const bool colon = f[0] >= '0' && f[0] <= '9';
    const std::vector<std::string> tok = colon ? split(f, ':', 4) : split(f, '|', 3);
    const std::string kind = colon ? (tok.size() >= 3 ? tok[2] : std::string()) : tok[0];
    if (kind == "SIMPLE_DATE_FORMAT" || kind == "TIMESTAMP")
      return fail(PG_ERR_UNSUPPORTED, std::string("the ") + what + " '" + shown(f) + "' (only EPOCH formats run on the GPU path)");
    if (kind != "EPOCH" || (colon && tok.size() != 3))
      return fail(PG_ERR_INVALID_ARGUMENT, std::string("malformed ") + what + " '" + shown(f) + "' (size:UNIT:EPOCH or EPOCH|UNIT|size)");
    size = 1;
    std::string uname = "MILLISECONDS";
    if (colon) {
      if (!positive_int(tok[0], f, size)) return false;
      uname = tok[1];
    } else {
      if (tok.size() >= 2) uname = tok[1];
      if (tok.size() >= 3 && !positive_int(tok[2], f, size)) return false;
    }
    return time_unit(uname, "time unit", true, unit);
  }
  // DateTimeGranularitySpec: size:UNIT or UNIT(|size)
  bool granularity(const std::string& g, int64_t& millis) {
    if (g.empty()) return fail(PG_ERR_INVALID_ARGUMENT, "empty granularity");
    const bool colon = g[0] >= '0' && g[0] <= '9';
    const std::vector<std::string> tok = colon ? split(g, ':', 2) : split(g, '|', 2);
    if (colon && tok.size() != 2) return fail(PG_ERR_INVALID_ARGUMENT, "malformed granularity '" + shown(g) + "' (size:UNIT)");
    int64_t size = 1;
    if (colon ? !positive_int(tok[0], g, size) : (tok.size() == 2 && !positive_int(tok[1], g, size))) return false;
    Unit u;
    const std::string uname = colon ? tok[1] : tok[0];
    u = unit_of(uname);
    if (u == U_CUSTOM || u == U_UNKNOWN) return fail(PG_ERR_INVALID_ARGUMENT, "unknown time unit '" + shown(uname) + "' in the granularity '" + shown(g) + "'");
    // TimeUnit.MILLISECONDS.convert(size, unit): size is an int, so nothing saturates
    millis = u >= U_MILLIS ? size * (kUnitNanos[u] / kUnitNanos[U_MILLIS]) : size / (kUnitNanos[U_MILLIS] / kUnitNanos[u]);
    if (millis == 0) return fail(PG_ERR_INVALID_ARGUMENT, "the granularity '" + shown(g) + "' is below one millisecond (the reference divides by zero)");
    return true;
  }
  // UTC or +-HH:MM
  bool zone(const std::string& z, int64_t& offset) {
    offset = 0;
    if (upper(z) == "UTC") return true;
    const bool shaped = z.size() == 6 && (z[0] == '+' || z[0] == '-') && z[3] == ':' && z[1] >= '0' && z[1] <= '9' && z[2] >= '0' && z[2] <= '9' &&
                        z[4] >= '0' && z[4] <= '9' && z[5] >= '0' && z[5] <= '9';
    const int hh = shaped ? (z[1] - '0') * 10 + (z[2] - '0') : 99, mm = shaped ? (z[4] - '0') * 10 + (z[5] - '0') : 99;
    if (!shaped || hh > 23 || mm > 59)
      return fail(PG_ERR_UNSUPPORTED, "the time zone '" + shown(z) + "' (UTC and fixed offsets +-HH:MM run on the GPU path, named zones stay with the Java plan)");
    offset = (int64_t)(hh * 60 + mm) * 60000 * (z[0] == '-' ? -1 : 1);
    return true;
  }

  bool run(TimeProgram& out) {
    size_t after = 0;
    const std::string name = head_name(s, &after);
    Unit unit = U_MILLIS;
    Variant variant = V_PLAIN;
    const Family fam = family_of(name, &unit, &variant);
    if (name.empty() || fam == F_NONE) return fail(PG_ERR_INVALID_ARGUMENT, "a call of timeconvert, toepoch..., datetimeconvert or datetrunc expected at '" + shown(s) + "'");
    i = after;
    std::vector<Arg> args;
    if (!arguments(args)) return false;
    skip_ws();
    if (i < n) return fail(PG_ERR_INVALID_ARGUMENT, "trailing text '" + shown(std::string(s + i, n - i)) + "'");
    pg_time_program& P = out.prog;
    memset(&P, 0, sizeof(P));
    P.pre_mul = 1;
    std::string t;
    switch (fam) {
      case F_TIMECONVERT: {
        if (!count(name, args.size(), 3, 3) || !value(args[0], name, out.column)) return false;
        Unit in, to;
        if (!literal(args[1], "input unit", t) || !time_unit(upper(t), "input unit", false, in)) return false;
        if (!literal(args[2], "output unit", t) || !time_unit(upper(t), "output unit", true, to)) return false;
        P.out = conv_of(in, to);
        return true;
      }
      case F_TOEPOCH: {
        const size_t want = variant == V_PLAIN ? 1 : 2;
        if (!count(name, args.size(), want, want) || !value(args[0], name, out.column)) return false;
        P.out = conv_of(U_MILLIS, unit);
        if (variant != V_PLAIN) {
          int64_t nn;
          if (!long_literal(args[1], variant == V_ROUNDED ? "rounding size" : "bucket size", nn)) return false;
          if (nn == 0) return fail(PG_ERR_INVALID_ARGUMENT, name + " by 0 (the reference throws ArithmeticException)");
          P.post = variant == V_ROUNDED ? PG_TIME_POST_ROUND : PG_TIME_POST_DIV;
          P.post_div = time_divisor_of(nn);
        }
        return true;
      }
      case F_DATETIMECONVERT: {
        if (args.size() == 5 && value(args[0], name, out.column))
          return fail(PG_ERR_UNSUPPORTED, "datetimeconvert with a bucketing time zone (its fifth argument)");
        if (!count(name, args.size(), 4, 4) || !value(args[0], name, out.column)) return false;
        int64_t in_size, out_size, gran;
        Unit in_unit, out_unit;
        if (!literal(args[1], "input format", t) || !format(t, "input format", in_size, in_unit)) return false;
        if (!literal(args[2], "output format", t) || !format(t, "output format", out_size, out_unit)) return false;
        if (!literal(args[3], "granularity", t) || !granularity(t, gran)) return false;
        P.pre_mul = in_size;
        P.in = conv_of(in_unit, U_MILLIS);
        P.bucket = PG_TIME_BUCKET_TRUNC;
        P.bucket_div = time_divisor_of(gran);
        P.out = conv_of(U_MILLIS, out_unit);
        if (out_size != 1) { P.post = PG_TIME_POST_DIV; P.post_div = time_divisor_of(out_size); }
        return true;
      }
      default: {
        if (!count(name, args.size(), 2, 5)) return false;
        std::string u;
        if (!literal(args[0], "truncation unit", u)) return false;
        if (args[0].kind != Arg::QUOTED) return fail(PG_ERR_INVALID_ARGUMENT, "the truncation unit of datetrunc must be a quoted literal, not " + shown(u));
        if (!value(args[1], name, out.column)) return false;
        u = lower(u);
        int64_t width = 0;
        if (u == "millisecond") P.bucket = PG_TIME_BUCKET_NONE;
        else if (u == "second") width = 1000;
        else if (u == "minute") width = 60000;
        else if (u == "hour") width = 3600000;
        else if (u == "day") width = 86400000;
        else if (u == "week") { width = 604800000; P.phase = 4 * 86400000LL; }   // 1970-01-05 is a Monday
        else if (u == "month") P.bucket = PG_TIME_BUCKET_MONTH;
        else if (u == "quarter") P.bucket = PG_TIME_BUCKET_QUARTER;
        else if (u == "year") P.bucket = PG_TIME_BUCKET_YEAR;
        else return fail(PG_ERR_INVALID_ARGUMENT, "unknown truncation unit '" + shown(u) + "' (millisecond, second, minute, hour, day, week, month, quarter, year)");
        if (width) { P.bucket = PG_TIME_BUCKET_FLOOR; P.bucket_div = time_divisor_of(width); }
        Unit in = U_MILLIS, to;
        if (args.size() >= 3 && (!literal(args[2], "input unit", t) || !time_unit(upper(t), "input unit", false, in))) return false;
        to = in;
        if (args.size() >= 4 && (!literal(args[3], "time zone", t) || !zone(t, P.offset))) return false;
        if (args.size() >= 5 && (!literal(args[4], "output unit", t) || !time_unit(upper(t), "output unit", false, to))) return false;
        P.in = conv_of(in, U_MILLIS);
        P.out = conv_of(U_MILLIS, to);
        return true;
      }
    }
  }
};

}  // namespace

pg_time_divisor time_divisor_of(int64_t d) {
  pg_time_divisor D;
  memset(&D, 0, sizeof(D));
  D.d = d;
  D.neg = d < 0;
  if (d == INT64_MIN) { D.shift = PG_TIME_DIV_MIN; D.neg = 0; return D; }
  const uint64_t ad = (uint64_t)(d < 0 ? -d : d);
  if (ad <= 1) { D.shift = PG_TIME_DIV_ONE; return D; }   // (0 is refused before it gets here)
  // Hacker's Delight 10-1, `magic` for a positive divisor, in 64 bits
  const uint64_t two63 = 1ULL << 63;
  const uint64_t anc = two63 - 1 - two63 % ad;
  int p = 63;
  uint64_t q1 = two63 / anc, r1 = two63 - q1 * anc, q2 = two63 / ad, r2 = two63 - q2 * ad, delta;
  do {
    p++;
    q1 *= 2; r1 *= 2;
    if (r1 >= anc) { q1++; r1 -= anc; }
    q2 *= 2; r2 *= 2;
    if (r2 >= ad) { q2++; r2 -= ad; }
    delta = ad - r2;
  } while (q1 < delta || (q1 == delta && r1 == 0));
  D.magic = (int64_t)(q2 + 1);
  D.shift = p - 64;
  return D;
}

bool time_expr_is_time_function(const char* text) {
  if (!text) return false;
  return family_of(head_name(text), nullptr, nullptr) != F_NONE;
}

int32_t time_expr_parse(const char* text, TimeProgram& out, std::string& error) {
  out.column.clear();
  memset(&out.prog, 0, sizeof(out.prog));
  error.clear();
  if (!text) { error = "time function: null text"; return PG_ERR_INVALID_ARGUMENT; }
  Parser p(text, error);
  if (!p.run(out)) { out.column.clear(); memset(&out.prog, 0, sizeof(out.prog)); }
  return p.status;
}

}  // namespace pg
