// Stand-alone driver of the query splitter of the side passes (pinot_amd/csrc/pg_side_query.cpp), built with -fsanitize=address,undefined by
// tests/test_side_query.py: every shape of aggregation list, ORDER BY, agg_params and flags the two paths hand over, each in heap arrays of
// exactly its length so that a read past them is caught; and the tier choice of the slot-table paths (pg::side_tier) at both sides of every
// boundary.  Prints one line per case and "side query ok" at the end.
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../include/pinot_gpu.h"
#include "../pinot_amd/csrc/pg_side_query.h"

static int failures = 0;

// a side aggregation of these cases is a PERCENTILE (as on the percentile path) ...
static bool is_percentile(const pg_agg_spec& s) { return s.function == PG_AGG_PERCENTILE; }
// ... or one whose column holds a '(' (as on the expression path)
static bool is_expression(const pg_agg_spec& s) { return s.column && strchr(s.column, '(') != nullptr; }

static const int32_t kPercentileClears = PG_QUERY_FLAG_FINAL_PERCENTILE | PG_QUERY_FLAG_KEEP_DEVICE_TABLE;
static const int32_t kExpressionClears = PG_QUERY_FLAG_KEEP_DEVICE_TABLE;

struct Agg {
  int32_t function;
  const char* column;
  double param;
};
struct Case {
  const char* what;
  std::vector<Agg> aggs;
  std::vector<pg_order_by> order;
  bool with_params = true;
  bool (*is_side)(const pg_agg_spec&) = is_percentile;
  int32_t clear = kPercentileClears;
  int32_t flags = 0;
  // expectations
  int32_t status = PG_OK;
  std::vector<int> base_index;
  std::vector<int> kept;               // indexes of the query's aggregations the ordinary part holds, in order; -1: the inserted COUNT(*)
  bool order_kept = true;
  std::vector<int32_t> order_index;    // the ORDER BY entries' indexes in the ordinary part
};

static pg_order_by by_agg(int32_t index, int32_t ascending = 0) { return pg_order_by{PG_ORDER_BY_AGGREGATION, index, ascending, 1}; }
static pg_order_by by_key(int32_t index, int32_t ascending = 1) { return pg_order_by{PG_ORDER_BY_GROUP_KEY, index, ascending, 0}; }

static void run(const Case& c) {
  // exact-size heap copies: the splitter must not read one element past them
  pg_agg_spec* aggs = new pg_agg_spec[c.aggs.size()];
  double* params = new double[c.aggs.size()];
  for (size_t a = 0; a < c.aggs.size(); a++) {
    memset(&aggs[a], 0, sizeof(aggs[a]));
    aggs[a].function = c.aggs[a].function;
    aggs[a].log2m = (int32_t)a + 3;   // carried through untouched
    aggs[a].column = c.aggs[a].column;
    params[a] = c.aggs[a].param;
  }
  pg_order_by* order = new pg_order_by[c.order.size()];
  for (size_t i = 0; i < c.order.size(); i++) order[i] = c.order[i];
  const char* group_by[2] = {"g0", "g1"};
  pg_query q;
  memset(&q, 0, sizeof(q));
  q.n_group_by = 2;
  q.group_by_columns = group_by;
  q.n_aggregations = (int32_t)c.aggs.size();
  q.aggregations = aggs;
  q.agg_params = c.with_params ? params : nullptr;
  q.flags = c.flags;
  q.n_order_by = (int32_t)c.order.size();
  q.order_by = c.order.empty() ? nullptr : order;
  q.limit = 7;
  q.num_groups_limit = 13;
  q.min_segment_group_trim_size = 5;

  pg::SideBaseQuery B;
  std::string error;
  const int32_t st = pg::side_base_query(q, c.is_side, c.clear, B, error);
  bool ok = st == c.status;
  std::string why;
  auto check = [&](bool cond, const char* what) { if (!cond) { ok = false; why += std::string(" [") + what + "]"; } };
  if (st != PG_OK) {
    char want[96];
    snprintf(want, sizeof(want), "ORDER BY aggregation %d of %d", c.order_index.empty() ? 0 : c.order_index[0], q.n_aggregations);
    check(error == want, "error text");
  } else if (ok) {
    const pg_query& b = B.q;
    check(error.empty(), "no error text");
    check(B.base_index == c.base_index, "base_index");
    check(b.n_aggregations == (int32_t)c.kept.size() && B.aggs.size() == c.kept.size() && B.params.size() == c.kept.size(), "kept count");
    check(b.aggregations == B.aggs.data(), "aggregations point into the struct");
    for (size_t k = 0; k < c.kept.size() && k < B.aggs.size(); k++) {
      const pg_agg_spec& s = B.aggs[k];
      if (c.kept[k] < 0) {
        check(s.function == PG_AGG_COUNT && s.column == nullptr && s.log2m == 0 && B.params[k] == 0.0, "inserted COUNT(*)");
      } else {
        const size_t a = (size_t)c.kept[k];
        check(s.function == aggs[a].function && s.column == aggs[a].column && s.log2m == aggs[a].log2m, "kept spec");
        check(B.params[k] == (c.with_params ? params[a] : 0.0), "kept param");
      }
    }
    check(c.with_params ? b.agg_params == B.params.data() : b.agg_params == nullptr, "agg_params");
    check(b.flags == ((c.flags | PG_QUERY_FLAG_SKIP_STAR_TREE) & ~c.clear), "flags");
    check(b.filter == q.filter && b.n_group_by == 2 && b.group_by_columns == group_by && b.limit == 7 && b.num_groups_limit == 13 &&
              b.min_segment_group_trim_size == 5 && b.max_initial_result_holder_capacity == 0, "the rest of the query");
    if (c.order.empty()) {
      check(b.n_order_by == 0 && b.order_by == nullptr, "no ORDER BY");
    } else if (!c.order_kept) {
      check(b.n_order_by == 0 && b.order_by == nullptr, "ORDER BY dropped");
    } else {
      check(b.n_order_by == (int32_t)c.order.size() && b.order_by == B.order.data() && B.order.size() == c.order.size(), "ORDER BY kept");
      for (size_t i = 0; i < c.order.size() && i < B.order.size(); i++) {
        const pg_order_by& o = B.order[i];
        check(o.kind == c.order[i].kind && o.ascending == c.order[i].ascending && o.nulls_last == c.order[i].nulls_last, "ORDER BY entry");
        check(o.index == c.order_index[i], "ORDER BY index");
      }
    }
  }
  printf("%s %s: status %d (want %d)%s%s%s\n", ok ? "ok  " : "FAIL", c.what, st, c.status, error.empty() ? "" : " — ", error.c_str(), why.c_str());
  if (!ok) failures++;
  delete[] aggs;
  delete[] params;
  delete[] order;
}

// The tier of a slot-table path's table (pg::side_tier), at both sides of every boundary.  A table has `planes` 8-byte planes per slot:
// 1, or 2 in the wide mode of FIRSTWITHTIME / LASTWITHTIME.
static void tier_case(const char* what, int32_t n_group_by, uint64_t n_slots, int planes, uint64_t lds_max_slots, int64_t hbm_max_bytes, pg::Tier want) {
  const pg::Tier got = pg::side_tier(n_group_by, n_slots, lds_max_slots, n_slots * 8 * (uint64_t)planes, hbm_max_bytes);
  printf("%s tier: %s: %d (want %d)\n", got == want ? "ok  " : "FAIL", what, (int)got, (int)want);
  if (got != want) failures++;
}
static void tier_cases() {
  const uint64_t ceiling = 16384;        // PG_EXPR_LDS_SLOTS / PG_VAR_LDS_SLOTS / PG_WT_LDS_SLOTS
  const int64_t limit = 8 * 100000;      // an HBM knob: room for 100 000 slots
  tier_case("no GROUP BY, one slot", 0, 1, 1, ceiling, limit, pg::TIER_REG);
  tier_case("no GROUP BY, more slots than any limit", 0, 100001, 1, ceiling, limit, pg::TIER_REG);
  tier_case("GROUP BY, one slot", 1, 1, 1, ceiling, limit, pg::TIER_LDS);
  tier_case("slots == LDS ceiling", 2, ceiling, 1, ceiling, limit, pg::TIER_LDS);
  tier_case("slots == LDS ceiling + 1", 2, ceiling + 1, 1, ceiling, limit, pg::TIER_HBM);
  tier_case("a lowered LDS knob: slots == knob", 1, 64, 1, 64, limit, pg::TIER_LDS);
  tier_case("a lowered LDS knob: slots == knob + 1", 1, 65, 1, 64, limit, pg::TIER_HBM);
  tier_case("bytes == HBM limit", 1, 100000, 1, ceiling, limit, pg::TIER_HBM);
  tier_case("bytes == HBM limit + 8", 1, 100001, 1, ceiling, limit, pg::TIER_REFUSED);
  tier_case("double width: bytes == HBM limit at half the slots", 1, 50000, 2, ceiling, limit, pg::TIER_HBM);
  tier_case("double width: refused at half the slots + 1", 1, 50001, 2, ceiling, limit, pg::TIER_REFUSED);
  tier_case("double width below the LDS ceiling: the slot count decides", 1, ceiling, 2, ceiling, limit, pg::TIER_LDS);
  tier_case("an HBM limit below the LDS ceiling: LDS is asked first", 1, ceiling, 1, ceiling, 8, pg::TIER_LDS);
  static_assert(pg::TIER_REG == 0 && pg::TIER_LDS == 1 && pg::TIER_HBM == 2, "the tiers index the paths' kernel names");
}

int main() {
  tier_cases();
  const Agg P50{PG_AGG_PERCENTILE, "v", 50.0}, P99{PG_AGG_PERCENTILE, "w", 99.0}, SUM{PG_AGG_SUM, "s", 1.5}, MAX{PG_AGG_MAX, "m", 2.5}, COUNT{PG_AGG_COUNT, "*", 3.5};
  const Agg XSUM{PG_AGG_SUM, "add(a,b)", 4.5}, XMIN{PG_AGG_MIN, "mult(a,'2')", 5.5};
  const int32_t every_flag = PG_QUERY_FLAG_PROFILE | PG_QUERY_FLAG_NULL_HANDLING | PG_QUERY_FLAG_FINAL_PERCENTILE | PG_QUERY_FLAG_KEEP_DEVICE_TABLE | PG_QUERY_FLAG_FINAL_DISTINCT;
  std::vector<Case> cases;
  auto add = [&](const Case& c) { cases.push_back(c); };
  {
    Case c; c.what = "no side aggregation: nothing left out";
    c.aggs = {SUM, MAX, COUNT}; c.order = {by_agg(2)}; c.base_index = {0, 1, 2}; c.kept = {0, 1, 2}; c.order_index = {2}; add(c);
  }
  {
    Case c; c.what = "every aggregation a side one: COUNT(*) is inserted";
    c.aggs = {P50, P99}; c.base_index = {-1, -1}; c.kept = {-1}; add(c);
    c.what = "every aggregation a side one, agg_params null"; c.with_params = false; add(c);
  }
  {
    Case c; c.what = "a side aggregation first: the ORDER BY index shifts by 1";
    c.aggs = {P50, SUM, MAX}; c.order = {by_agg(2, 1)}; c.base_index = {-1, 0, 1}; c.kept = {1, 2}; c.order_index = {1}; add(c);
  }
  {
    Case c; c.what = "side aggregations first and in the middle: the ORDER BY index shifts by 2";
    c.aggs = {P50, SUM, P99, MAX}; c.order = {by_agg(3)}; c.base_index = {-1, 0, -1, 1}; c.kept = {1, 3}; c.order_index = {1}; add(c);
  }
  {
    Case c; c.what = "a side aggregation last: no shift";
    c.aggs = {SUM, MAX, P50}; c.order = {by_agg(1)}; c.base_index = {0, 1, -1}; c.kept = {0, 1}; c.order_index = {1}; add(c);
  }
  {
    Case c; c.what = "ORDER BY a side aggregation: ORDER BY is dropped, LIMIT stays";
    c.aggs = {SUM, P50, MAX}; c.order = {by_agg(1)}; c.base_index = {0, -1, 1}; c.kept = {0, 2}; c.order_kept = false; add(c);
    c.what = "ORDER BY a plain and a side aggregation: dropped as well"; c.order = {by_agg(2), by_key(0), by_agg(1)}; add(c);
  }
  {
    Case c; c.what = "ORDER BY a key column and an aggregation mixed";
    c.aggs = {P50, COUNT, P99, SUM}; c.order = {by_key(1, 0), by_agg(3), by_key(0), by_agg(1, 1)}; c.base_index = {-1, 0, -1, 1}; c.kept = {1, 3};
    c.order_index = {1, 1, 0, 0}; add(c);
  }
  {
    Case c; c.what = "ORDER BY aggregation -1: invalid argument";
    c.aggs = {P50, SUM}; c.order = {by_agg(-1)}; c.status = PG_ERR_INVALID_ARGUMENT; c.order_index = {-1}; add(c);
    c.what = "ORDER BY aggregation n: invalid argument"; c.order = {by_agg(2)}; c.order_index = {2}; add(c);
    c.what = "ORDER BY key column n: the splitter leaves key indexes alone"; c.order = {by_key(2)}; c.status = PG_OK; c.base_index = {-1, 0}; c.kept = {1};
    add(c);
  }
  {
    Case c; c.what = "agg_params null: the ordinary part's is null";
    c.aggs = {SUM, P50, MAX}; c.with_params = false; c.base_index = {0, -1, 1}; c.kept = {0, 2}; add(c);
    c.what = "agg_params given: the kept aggregations' params"; c.with_params = true; add(c);
  }
  {
    Case c; c.what = "the percentile path's flags: FINAL_PERCENTILE and KEEP_DEVICE_TABLE cleared";
    c.aggs = {P50, SUM}; c.flags = every_flag; c.base_index = {-1, 0}; c.kept = {1}; add(c);
    c.what = "the percentile path's flags: none set"; c.flags = 0; add(c);
  }
  {
    Case c; c.what = "the expression path: a PERCENTILE stays with its param and FINAL_PERCENTILE, KEEP_DEVICE_TABLE is cleared";
    c.is_side = is_expression; c.clear = kExpressionClears; c.flags = every_flag;
    c.aggs = {XSUM, P50, XMIN, MAX}; c.order = {by_agg(3), by_key(1)}; c.base_index = {-1, 0, -1, 1}; c.kept = {1, 3}; c.order_index = {1, 1}; add(c);
    c.what = "the expression path: ORDER BY the expression aggregation"; c.order = {by_agg(2)}; c.order_kept = false; add(c);
    c.what = "the expression path: only expression aggregations"; c.aggs = {XSUM, XMIN}; c.order = {}; c.base_index = {-1, -1}; c.kept = {-1}; add(c);
  }
  for (const Case& c : cases) run(c);
  if (failures) {
    printf("%d FAILED\n", failures);
    return 1;
  }
  printf("side query ok (%zu cases)\n", cases.size());
  return 0;
}
