// Queries with a FIRSTWITHTIME / LASTWITHTIME aggregation (PG_AGG_FIRSTWITHTIME, PG_AGG_LASTWITHTIME): a side pass joined to the ordinary
// plan by group key, in the frame of pg_exec_sidepass.hip (which runs step 1 and the filter, maps the admitted groups to rows and joins the
// result, step 4).
//   1. The ordinary part — the query without these aggregations (COUNT(*) if nothing else remains) — runs through execute_query unchanged,
//      never on a star-tree: it decides the groups, the numGroupsLimit admission and the other aggregations' results (a variance or a
//      PERCENTILE among them takes its own side pass from there).  An ORDER BY that names one of them leaves the segment untrimmed.
//   2. One arg-max pass for ALL of them over the filter's match words into a table [G][slots] of 64-bit keys: one slot per distinct (time
//      column, direction) — LASTWITHTIME(a,t,..) and LASTWITHTIME(b,t,..) share a winner doc.  A slot whose time column's range fits beside
//      the docId (pg_with_time.h: the packed bound) is decided in this one pass; the others take the wide mode's second pass over a doc
//      plane.  pg_wt_reg without GROUP BY, pg_wt_lds up to PG_WT_LDS_SLOTS slots, pg_wt_hbm up to Knobs::wt_hbm_max_bytes; beyond that the
//      query is refused.
//   3. pg_wt_gather reads the winner doc, its time and every value column at it for the admitted rows; the host converts the one value per
//      group to the declared type as a Java primitive conversion does.
//   4. The pairs are joined to the ordinary part on the host.
// The kernels are those of pg_kernels_withtime.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <set>
#include <string>

#include "pg_internal.hpp"
#include "pg_expr.h"
#include "pg_with_time.h"

void pg_wt_launch_pass(const PgWtArgs* args, int tier, int grid, hipStream_t stream);
void pg_wt_launch_gather(const PgWtGatherArgs* args, int grid, hipStream_t stream);

namespace pg {
namespace {

const char* kWho = "FIRSTWITHTIME / LASTWITHTIME";
const char* kSubject = "FIRSTWITHTIME / LASTWITHTIME";
const char* const kTierKernel[3] = {"pg_wt_reg", "pg_wt_lds", "pg_wt_hbm"};


// the argument list of pg_agg_spec.column: x, t, 'TYPE' (include/pinot_gpu.h: the general form of aggregations with more than one argument)
struct WtArguments {
  std::string x, t;
  int32_t type = -1;   // pg_data_type of the declared type
};
WtArguments parse_arguments(const pg_agg_spec& s) {
  const char* fn = agg_function_text(s.function);
  if (!s.column) fail(PG_ERR_INVALID_ARGUMENT, "%s needs its argument list: column, time column, 'data type'", fn);
  std::vector<ExprArgument> args;
  std::string error;
  const int32_t st = expr_split_arguments(s.column, args, error);
  if (st != PG_OK) fail(st, "%s(%s): %s", fn, s.column, error.c_str());
  if (args.size() != 3) fail(PG_ERR_INVALID_ARGUMENT, "%s takes 3 arguments (column, time column, 'data type'), %d given: %s", fn, (int)args.size(), s.column);
  if (!args[2].quoted) fail(PG_ERR_INVALID_ARGUMENT, "%s: the third argument must be a quoted data type literal, not %s", fn, args[2].text.c_str());
  for (int k = 0; k < 2; k++) {
    if (args[(size_t)k].quoted) fail(PG_ERR_INVALID_ARGUMENT, "%s: argument %d must be a column, not the literal '%s'", fn, k + 1, args[(size_t)k].text.c_str());
    if (expr_is_expression(args[(size_t)k].text.c_str())) fail(PG_ERR_UNSUPPORTED, "%s over an expression (%s): its arguments are columns on the GPU path", fn, args[(size_t)k].text.c_str());
  }
  std::string type;
  for (char c : args[2].text) type.push_back(c >= 'a' && c <= 'z' ? (char)(c - 'a' + 'A') : c);   // DataType.valueOf(toUpperCase())
  WtArguments A;
  A.x = args[0].text;
  A.t = args[1].text;
  if (type == "INT") A.type = PG_TYPE_INT;
  else if (type == "LONG") A.type = PG_TYPE_LONG;
  else if (type == "FLOAT") A.type = PG_TYPE_FLOAT;
  else if (type == "DOUBLE") A.type = PG_TYPE_DOUBLE;
  else if (type == "BOOLEAN" || type == "STRING" || type == "BIG_DECIMAL" || type == "TIMESTAMP" || type == "JSON" || type == "BYTES")
    fail(PG_ERR_UNSUPPORTED, "%s with the declared type '%s': INT, LONG, FLOAT and DOUBLE run on the GPU path", fn, type.c_str());
  else
    fail(PG_ERR_INVALID_ARGUMENT, "%s: '%s' is no data type", fn, args[2].text.c_str());
  return A;
}

struct WtSlot {
  Column* time = nullptr;
  bool first = false;
  bool packed = false;
  int64_t base = 0;
};
struct WtAgg {
  int index = 0;            // among the query's aggregations
  Column* value = nullptr;
  int slot = 0;
  int32_t type = 0;         // declared type
  bool first = false;
};
struct WtPlan {
  SideTable table;              // one slot per distinct (time column, direction)
  std::vector<WtSlot> slots;
  std::vector<WtAgg> aggs;
  int doc_bits = 1;
  bool any_wide = false;
};

int64_t dict_entry(const Column& c, int32_t id) {   // an INT / LONG dictionary's value (big-endian on the host)
  const uint8_t* p = c.dict_host.data() + (size_t)id * (size_t)c.dict_bytes_per_value;
  uint64_t v = 0;
  for (int k = 0; k < c.dict_bytes_per_value; k++) v = (v << 8) | p[k];
  return c.dict_bytes_per_value == 4 ? (int64_t)(int32_t)(uint32_t)v : (int64_t)v;
}

// the time column's range where the segment knows it: the ends of a sorted dictionary, or the raw column's registered extremes
bool time_range(const Column& c, int64_t& tmin, int64_t& tmax) {
  if (c.has_dictionary) {
    if (c.cardinality < 1 || (c.dict_bytes_per_value != 4 && c.dict_bytes_per_value != 8)) return false;
    if (c.dict_host.size() < (size_t)c.cardinality * (size_t)c.dict_bytes_per_value) return false;
    tmin = dict_entry(c, 0);
    tmax = dict_entry(c, c.cardinality - 1);
    return tmin <= tmax;
  }
  if (!c.has_int_range) return false;
  tmin = c.int_min;
  tmax = c.int_max;
  return tmin <= tmax;
}

WtPlan wt_plan(Segment& seg, const pg_query& q) {
  side_query_check(q, kSubject);
  const bool null_handling = (q.flags & PG_QUERY_FLAG_NULL_HANDLING) != 0;
  WtPlan P;
  P.doc_bits = pg_wt_doc_bits(std::max<int64_t>(1, seg.total_docs));
  std::set<std::string> read;
  std::lock_guard<std::mutex> lock(seg.mu);   // virtual dictionaries are built under the segment's lock
  for (int a = 0; a < q.n_aggregations; a++) {
    const pg_agg_spec& s = q.aggregations[a];
    if (!is_with_time_agg(s)) {
      side_columns_read(s, read);
      continue;
    }
    const char* fn = agg_function_text(s.function);
    const WtArguments A = parse_arguments(s);
    WtAgg g;
    g.index = a;
    g.type = A.type;
    g.first = s.function == PG_AGG_FIRSTWITHTIME;
    g.value = side_argument_column(seg, A.x.c_str(), fn, "column", "column", "", null_handling);
    Column* t = side_argument_column(seg, A.t.c_str(), fn, "time column", "time column", "", null_handling);
    if (t->val_type != PG_V_I32 && t->val_type != PG_V_I64)
      fail(PG_ERR_UNSUPPORTED, "%s with the %s time column %s: an INT or LONG time column runs on the GPU path", fn, t->data_type == PG_TYPE_FLOAT ? "FLOAT" : "DOUBLE", t->name.c_str());
    read.insert(g.value->name);
    read.insert(t->name);
    if (P.aggs.size() >= PG_WT_MAX_AGGS) fail(PG_ERR_UNSUPPORTED, "more than %d FIRSTWITHTIME / LASTWITHTIME aggregations in one query", PG_WT_MAX_AGGS);
    size_t k = 0;
    while (k < P.slots.size() && !(P.slots[k].time == t && P.slots[k].first == g.first)) k++;
    if (k == P.slots.size()) {
      if (k >= PG_WT_MAX_SLOTS) fail(PG_ERR_UNSUPPORTED, "FIRSTWITHTIME / LASTWITHTIME over more than %d distinct (time column, direction) pairs in one query", PG_WT_MAX_SLOTS);
      WtSlot S;
      S.time = t;
      S.first = g.first;
      int64_t tmin = 0, tmax = 0;
      if (time_range(*t, tmin, tmax) && pg_wt_packed_ok(pg_wt_range(tmin, tmax), P.doc_bits)) {
        S.packed = true;
        S.base = g.first ? tmax : tmin;
      } else {
        P.any_wide = true;
      }
      P.slots.push_back(S);
    }
    g.slot = (int)k;
    P.aggs.push_back(g);
  }
  // the wide mode keeps a doc plane next to the keys: twice the bytes
  P.table = side_table_plan(seg, q, kSubject, kWho, read, (int32_t)P.slots.size(), PG_WT_LDS_SLOTS, P.any_wide ? 16 : 8, knobs().wt_hbm_max_bytes, kSubject, "PG_WT_HBM_MAX_BYTES");
  return P;
}

// ---- the Java primitive conversions of get<T>ValuesSV over a column of another stored type (JLS 5.1.2, 5.1.3) -----------------------------------
int64_t java_d2l(double d) {
  if (d != d) return 0;
  if (d >= 9223372036854775807.0) return INT64_MAX;
  if (d <= -9223372036854775808.0) return INT64_MIN;
  return (int64_t)d;
}
int32_t java_d2i(double d) {
  if (d != d) return 0;
  if (d >= 2147483647.0) return INT32_MAX;
  if (d <= -2147483648.0) return INT32_MIN;
  return (int32_t)d;
}
// `bits`: the stored value as pg_wt_gather hands it over; the result: the declared type's value (INT / LONG) or raw IEEE bits (FLOAT: 32)
int64_t convert_value(int64_t bits, int32_t stored, int32_t declared) {
  float f = 0;
  double d = 0;
  if (stored == PG_V_F32) { const uint32_t u = (uint32_t)bits; memcpy(&f, &u, 4); }
  if (stored == PG_V_F64) memcpy(&d, &bits, 8);
  auto float_bits = [](float v) { uint32_t u; memcpy(&u, &v, 4); return (int64_t)(uint64_t)u; };
  auto double_bits = [](double v) { int64_t u; memcpy(&u, &v, 8); return u; };
  switch (declared) {
    case PG_TYPE_INT:
      if (stored == PG_V_F32) return java_d2i((double)f);   // (int) of a float: the widening is exact
      if (stored == PG_V_F64) return java_d2i(d);
      return (int64_t)(int32_t)(uint32_t)(uint64_t)bits;    // (int) of a long keeps the low 32 bits
    case PG_TYPE_LONG:
      if (stored == PG_V_F32) return java_d2l((double)f);
      if (stored == PG_V_F64) return java_d2l(d);
      return bits;
    case PG_TYPE_FLOAT:
      if (stored == PG_V_F32) return (int64_t)(uint64_t)(uint32_t)bits;   // its own type: the bits as they are
      if (stored == PG_V_F64) return float_bits((float)d);                // rounds once
      return float_bits((float)bits);                                     // (float) of an int / a long: one rounding
    default:
      if (stored == PG_V_F32) return double_bits((double)f);
      if (stored == PG_V_F64) return bits;
      return double_bits((double)bits);
  }
}

}  // namespace

bool is_with_time_agg(const pg_agg_spec& s) { return s.function == PG_AGG_FIRSTWITHTIME || s.function == PG_AGG_LASTWITHTIME; }
void with_time_plan_check(Segment& seg, const pg_query& q) { (void)wt_plan(seg, q); }

std::unique_ptr<Result> execute_with_time(Segment& seg, const pg_query& q, const CancelToken* cancel) {
  const double t0 = now_ms();
  use_device(seg.device);
  const WtPlan P = wt_plan(seg, q);
  const double t_plan = now_ms();
  SideBaseQuery B;
  side_base_query(q, B);
  SidePass S = side_pass_begin(seg, q, B, P.table.groups, kWho, cancel);
  const int32_t n_rows = S.n_rows;
  const int64_t M = S.M, n_words = S.n_words;
  const int cus = S.cus;
  const int n_slots = (int)P.slots.size(), n_aggs = (int)P.aggs.size();
  hipStream_t stream = S.stream;
  // ---- the arg-max passes ------------------------------------------------------------------------------------------------------------------------
  PgWtArgs A;
  memset(&A, 0, sizeof(A));
  int64_t doc_bits = side_scan_fill(A.scan, seg, S, P.table.groups);
  A.slots = n_slots;
  A.doc_bits = P.doc_bits;
  A.n_groups = P.table.groups.G;
  A.n_slots = P.table.n_slots;
  for (int s = 0; s < n_slots; s++) {
    const WtSlot& W = P.slots[(size_t)s];
    expr_fill_src(A.slot[s].time, *W.time);
    A.slot[s].first = W.first ? 1 : 0;
    A.slot[s].packed = W.packed ? 1 : 0;
    A.slot[s].base = W.base;
    bool counted = false;   // FIRST and LAST over one time column read it once per pass
    for (int k = 0; k < s; k++) counted = counted || P.slots[(size_t)k].time == W.time;
    if (!counted) doc_bits += value_src_bits(*W.time);
  }
  const size_t plane_bytes = (size_t)P.table.n_slots * 8;
  DeviceBuffer keys(plane_bytes), docs(P.any_wide ? plane_bytes : 8);
  A.keys = keys.as<unsigned long long>();
  A.docs = P.any_wide ? docs.as<unsigned long long>() : nullptr;
  const int passes = P.any_wide ? 2 : 1;
  // PG_QUERY_FLAG_PROFILE: the passes (initialisation, arg-max, gather and its copy) between two events of their own
  ProfileTimer timer(q.flags);
  timer.start(stream);
  PG_HIP(hipMemsetAsync(keys.ptr, 0, plane_bytes, stream));
  if (P.any_wide) PG_HIP(hipMemsetAsync(docs.ptr, 0, plane_bytes, stream));
  if (M > 0 && n_words > 0) {
    // the LDS tier's workgroups are persistent: one per CU for a full table, up to four (32 waves) where the tables are small enough to
    // share the CU's LDS — the loop keeps one load per wave in flight, so the waves per CU decide how much of the bandwidth it reaches
    const int64_t lds_wgs = std::max<int64_t>(1, std::min<int64_t>(4, (int64_t)PG_WT_LDS_SLOTS / (int64_t)std::max<uint64_t>(1, P.table.n_slots)));
    const int grid = side_pass_grid(P.table.tier, cus, n_words, lds_wgs);
    for (int pass = 0; pass < passes; pass++) {   // the second pass reads the first one's maxima: stream order
      A.pass = pass;
      pg_wt_launch_pass(&A, P.table.tier, grid, stream);
      PG_HIP(hipGetLastError());
    }
  }
  const int width = 2 * n_slots + n_aggs;
  std::vector<int64_t> got((size_t)n_rows * (size_t)width);
  side_gather_rows(S, got, cancel, [&](const uint32_t* rows, int64_t* d_out) {
    PgWtGatherArgs Gt;
    memset(&Gt, 0, sizeof(Gt));
    Gt.keys = A.keys;
    Gt.docs = A.docs;
    Gt.rows = rows;
    Gt.n_rows = n_rows;
    Gt.slots = n_slots;
    Gt.n_aggs = n_aggs;
    Gt.doc_bits = P.doc_bits;
    Gt.n_docs = seg.total_docs;
    Gt.out = d_out;
    for (int s = 0; s < n_slots; s++) Gt.slot[s] = A.slot[s];
    for (int k = 0; k < n_aggs; k++) {
      expr_fill_src(Gt.value[k], *P.aggs[(size_t)k].value);
      Gt.value_slot[k] = P.aggs[(size_t)k].slot;
    }
    pg_wt_launch_gather(&Gt, side_flat_grid(cus, (int64_t)n_rows * (n_slots + n_aggs)), stream);
  });
  const float pass_ms = timer.stop_ms();
  // ---- the pairs: (value, time) of the winner doc; the function's default pair over no doc (a query without GROUP BY only) ---------------------------
  const bool empty_ok = q.n_group_by == 0 && M == 0;
  for (int32_t i = 0; i < n_rows; i++) {
    for (int s = 0; s < n_slots; s++) {
      const int64_t doc = got[(size_t)i * (size_t)width + 2 * (size_t)s];
      if (doc < 0 ? !empty_ok : doc >= seg.total_docs)
        fail(PG_ERR_INTERNAL, "FIRSTWITHTIME / LASTWITHTIME: winner doc %lld of an admitted group in a segment of %d docs (%lld matching)", (long long)doc, seg.total_docs, (long long)M);
    }
  }
  std::vector<AggResult> out((size_t)q.n_aggregations);
  for (int k = 0; k < n_aggs; k++) {
    const WtAgg& g = P.aggs[(size_t)k];
    AggResult r;
    r.kind = PG_RESULT_VALUE_TIME_PAIR;
    r.value_type = g.type;
    r.l[0].resize((size_t)n_rows);
    r.l[1].resize((size_t)n_rows);
    const bool floating = g.type == PG_TYPE_FLOAT || g.type == PG_TYPE_DOUBLE;
    if (floating) r.d[0].resize((size_t)n_rows);
    for (int32_t i = 0; i < n_rows; i++) {
      const int64_t* row = &got[(size_t)i * (size_t)width];
      int64_t time, bits;
      if (row[2 * g.slot] < 0) {   // DEFAULT_VALUE_TIME_PAIR: Integer.MIN_VALUE / Long.MIN_VALUE / Float.NaN / Double.NaN; Long.MIN_VALUE (LAST) / Long.MAX_VALUE (FIRST)
        time = g.first ? INT64_MAX : INT64_MIN;
        bits = g.type == PG_TYPE_INT ? (int64_t)INT32_MIN : g.type == PG_TYPE_LONG ? INT64_MIN : g.type == PG_TYPE_FLOAT ? (int64_t)0x7FC00000LL : (int64_t)0x7FF8000000000000LL;
      } else {
        time = row[2 * g.slot + 1];
        bits = convert_value(row[2 * n_slots + k], g.value->val_type, g.type);
      }
      r.l[0][(size_t)i] = time;
      r.l[1][(size_t)i] = bits;
      if (g.type == PG_TYPE_FLOAT) {
        const uint32_t u = (uint32_t)bits;
        float f;
        memcpy(&f, &u, 4);
        r.d[0][(size_t)i] = (double)f;
      } else if (g.type == PG_TYPE_DOUBLE) {
        memcpy(&r.d[0][(size_t)i], &bits, 8);
      }
    }
    out[(size_t)g.index] = std::move(r);
  }
  // the match words and the time and group columns once per pass, the gathered docs, times and values
  const int64_t pass_bytes = side_pass_bytes(seg, S, passes, doc_bits, (int64_t)got.size() * 8);
  std::unique_ptr<Result> res = side_pass_finish(seg, q, B, S, out, {kTierKernel[P.table.tier], pass_bytes, P.table.n_columns_read, pass_ms, t0, t_plan});
  res->merged_elsewhere |= MERGED_WITH_TIME;
  return res;
}

}  // namespace pg
