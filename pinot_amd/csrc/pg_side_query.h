// The ordinary part of a query that carries side aggregations — aggregations answered by a pass of their own and joined to the ordinary plan
// by group key (exact PERCENTILE: pg_exec_percentile.hip; aggregations over an expression: pg_exec_expr.hip; VAR_POP / VAR_SAMP /
// STDDEV_POP / STDDEV_SAMP: pg_exec_var.hip; FIRSTWITHTIME / LASTWITHTIME: pg_exec_withtime.hip; SKEWNESS / KURTOSIS: pg_exec_moment.hip; HISTOGRAM: pg_exec_hist.hip; the frame they share:
// pg_exec_sidepass.hip).  Plain C++ over include/pinot_gpu.h without HIP types: it compiles stand-alone (tests/side_query_main.cpp).
#pragma once
#include "../../include/pinot_gpu.h"

#include <string>
#include <vector>

namespace pg {
// The query without its side aggregations (COUNT(*) if nothing else remains), never on a star-tree (PG_QUERY_FLAG_SKIP_STAR_TREE), its
// ORDER BY re-indexed — or dropped when it names a side aggregation: the segment is then not trimmed (LIMIT stays).  `q` points into the
// vectors: the struct is filled in place and not copied.
struct SideBaseQuery {
  std::vector<pg_agg_spec> aggs;
  std::vector<double> params;    // the kept aggregations' agg_params (q.agg_params is null when the query had none)
  std::vector<pg_order_by> order;
  std::vector<int> base_index;   // per aggregation of the query: its index in the ordinary part, -1 for a side aggregation
  pg_query q;
  SideBaseQuery() = default;
  SideBaseQuery(const SideBaseQuery&) = delete;
  SideBaseQuery& operator=(const SideBaseQuery&) = delete;
};
// `is_side`: is this aggregation answered by the side pass?  `clear_flags`: PG_QUERY_FLAG_* bits the ordinary part must not see.
// PG_OK, or PG_ERR_INVALID_ARGUMENT (an ORDER BY aggregation index out of range) with the reason in `error`.
int32_t side_base_query(const pg_query& q, bool (*is_side)(const pg_agg_spec&), int32_t clear_flags, SideBaseQuery& out, std::string& error);

// Where a slot-table path (expressions, the variance family, covariance, SKEWNESS / KURTOSIS, HISTOGRAM, FIRSTWITHTIME / LASTWITHTIME) keeps its
// table [G][slots] of 64-bit slots: in registers without GROUP BY (one row; HISTOGRAM: per wavefront in LDS), per workgroup in LDS up to `lds_max_slots` slots, in HBM up to
// `hbm_max_bytes` bytes of table; beyond that the query is refused (side_table_plan, pg_exec_sidepass.hip, words the refusal).  The tiers' values index the paths' kernel names.
enum Tier { TIER_REFUSED = -1, TIER_REG = 0, TIER_LDS = 1, TIER_HBM = 2 };
Tier side_tier(int32_t n_group_by, uint64_t n_slots, uint64_t lds_max_slots, uint64_t table_bytes, int64_t hbm_max_bytes);
}  // namespace pg
