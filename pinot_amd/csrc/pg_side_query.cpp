// The split of a query into its ordinary part and its side aggregations (host code only; see pg_side_query.h).
#include "pg_side_query.h"

#include <stdio.h>
#include <string.h>

namespace pg {

int32_t side_base_query(const pg_query& q, bool (*is_side)(const pg_agg_spec&), int32_t clear_flags, SideBaseQuery& out, std::string& error) {
  out.base_index.assign((size_t)(q.n_aggregations > 0 ? q.n_aggregations : 0), -1);
  for (int a = 0; a < q.n_aggregations; a++) {
    if (is_side(q.aggregations[a])) continue;
    out.base_index[(size_t)a] = (int)out.aggs.size();
    out.aggs.push_back(q.aggregations[a]);
    out.params.push_back(q.agg_params ? q.agg_params[a] : 0.0);
  }
  if (out.aggs.empty()) {
    pg_agg_spec count_star;
    memset(&count_star, 0, sizeof(count_star));
    count_star.function = PG_AGG_COUNT;
    out.aggs.push_back(count_star);
    out.params.push_back(0.0);
  }
  pg_query& b = out.q;
  b = q;
  b.aggregations = out.aggs.data();
  b.n_aggregations = (int32_t)out.aggs.size();
  b.agg_params = q.agg_params ? out.params.data() : nullptr;
  b.flags = (q.flags | PG_QUERY_FLAG_SKIP_STAR_TREE) & ~clear_flags;
  // segment trim: an ORDER BY that names a side aggregation leaves the segment untrimmed; others keep their aggregation by its new index
  if (q.n_order_by > 0 && q.order_by) {
    bool by_side = false;
    for (int32_t i = 0; i < q.n_order_by; i++) {
      pg_order_by ob = q.order_by[i];
      if (ob.kind == PG_ORDER_BY_AGGREGATION) {
        if (ob.index < 0 || ob.index >= q.n_aggregations) {
          char msg[96];
          snprintf(msg, sizeof(msg), "ORDER BY aggregation %d of %d", ob.index, q.n_aggregations);
          error = msg;
          return PG_ERR_INVALID_ARGUMENT;
        }
        if (out.base_index[(size_t)ob.index] < 0) by_side = true;
        else ob.index = out.base_index[(size_t)ob.index];
      }
      out.order.push_back(ob);
    }
    if (by_side) { b.n_order_by = 0; b.order_by = nullptr; }
    else b.order_by = out.order.data();
  }
  return PG_OK;
}

Tier side_tier(int32_t n_group_by, uint64_t n_slots, uint64_t lds_max_slots, uint64_t table_bytes, int64_t hbm_max_bytes) {
  if (n_group_by == 0) return TIER_REG;
  if (n_slots <= lds_max_slots) return TIER_LDS;
  if (table_bytes <= (uint64_t)hbm_max_bytes) return TIER_HBM;
  return TIER_REFUSED;
}

}  // namespace pg
