// Queries with a HISTOGRAM aggregation (PG_AGG_HISTOGRAM): a side pass joined to the ordinary plan by group key.
// The pass is the sum-table pass of pg_exec_sidepass.hip (SumTablePass: the ordinary part, the filter's match words, the table, the timed
// accumulation and gather, the join and the statistics); this file holds what is the path's own:
//   the plan     one table [G][slots] of int64 counts for ALL of them: a row is the concatenated bins of the query's distinct (column, bin
//                specification) pairs (at most PG_HIST_MAX_SPECS; equal pairs share their slots).  There is no count slot: the ordinary
//                part names the groups, and a group whose values all fell outside [lower, upper] keeps its row of zeros.  pg_hist_one
//                without GROUP BY while the row fits PG_HIST_LDS_SLOTS, pg_hist_lds up to PG_HIST_LDS_SLOTS slots, pg_hist_hbm up to
//                Knobs::hist_hbm_max_bytes; beyond that the query is refused.
//   the kernels' arguments (PgHistArgs; the kernels are those of pg_kernels_hist.hip), the edge lists of the ARRAY form in one device
//                buffer with the flag the kernels raise over a doc on which the reference throws
//   the arrays   numBins doubles per group and histogram (PG_RESULT_DOUBLE_ARRAY), the counts as they are.
// The ordinary part is the query without these aggregations (a variance aggregation or a PERCENTILE among the others takes its own side
// pass from there); an ORDER BY that names one of them leaves the segment untrimmed.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <set>
#include <string>

#include "pg_internal.hpp"
#include "pg_expr.h"
#include "pg_histogram.h"

void pg_hist_launch_pass(const PgHistArgs* args, int tier, int grid, size_t lds_bytes, hipStream_t stream);

namespace pg {
namespace {

const char* kWho = "HISTOGRAM";
const char* kSubject = "HISTOGRAM";
const char* const kTierKernel[3] = {"pg_hist_one", "pg_hist_lds", "pg_hist_hbm"};

struct HistColumn {
  Column* col = nullptr;
  HistSpec spec;
  std::vector<int> aggs;    // the aggregations over it (indexes into the query's)
  int32_t first_slot = 0;
  int32_t edge_off = 0;     // its first edge in the plan's edge buffer
};
struct HistPlan {
  SideTable table;
  std::vector<HistColumn> cols;
  std::vector<double> edges;   // the edge lists back to back
};

HistPlan hist_plan(Segment& seg, const pg_query& q) {
  side_query_check(q, kSubject);
  const bool null_handling = (q.flags & PG_QUERY_FLAG_NULL_HANDLING) != 0;
  HistPlan P;
  int64_t slots = 0;
  std::set<std::string> read;
  std::lock_guard<std::mutex> lock(seg.mu);   // virtual dictionaries are built under the segment's lock
  for (int a = 0; a < q.n_aggregations; a++) {
    const pg_agg_spec& s = q.aggregations[a];
    if (!is_histogram_agg(s)) {
      side_columns_read(s, read);
      continue;
    }
    HistSpec spec;
    std::string error;
    int32_t st = hist_parse_arguments(s.column, spec, error);
    if (st != PG_OK) fail(st, "%s", error.c_str());
    if (expr_is_expression(spec.column.c_str()))
      fail(PG_ERR_UNSUPPORTED, "HISTOGRAM over an expression (%s): its argument is a column on the GPU path", spec.column.c_str());
    Column* c = side_argument_column(seg, spec.column.c_str(), "HISTOGRAM", "column", "argument column", " (the reference has no multi-value form)", null_handling);
    st = hist_spec_supported(spec, error);
    if (st != PG_OK) fail(st, "%s", error.c_str());
    read.insert(c->name);
    size_t k = 0;
    while (k < P.cols.size() && !(P.cols[k].col == c && P.cols[k].spec.same_bins(spec))) k++;
    if (k == P.cols.size()) {
      if (k >= PG_HIST_MAX_SPECS)
        fail(PG_ERR_UNSUPPORTED, "HISTOGRAM aggregations over more than %d distinct (column, bin specification) pairs in one query", PG_HIST_MAX_SPECS);
      HistColumn hc;
      hc.col = c;
      hc.first_slot = (int32_t)slots;
      hc.edge_off = (int32_t)P.edges.size();
      P.edges.insert(P.edges.end(), spec.edges.begin(), spec.edges.end());
      slots += spec.n_bins;
      hc.spec = std::move(spec);
      P.cols.push_back(std::move(hc));
    }
    P.cols[k].aggs.push_back(a);
  }
  const int64_t budget = knobs().hist_hbm_max_bytes;
  P.table = side_table_plan(seg, q, kSubject, kWho, read, (int32_t)slots, PG_HIST_LDS_SLOTS, 8, budget, "HISTOGRAM aggregations", "PG_HIST_HBM_MAX_BYTES");
  if (P.table.tier == TIER_REG && slots > PG_HIST_LDS_SLOTS) {   // no GROUP BY, a row beyond pg_hist_one's LDS: the table in HBM, under its budget
    if (slots * 8 > budget)
      fail(PG_ERR_UNSUPPORTED, "HISTOGRAM aggregations: 1 groups x %d slots need a table of %lld bytes, more than PG_HIST_HBM_MAX_BYTES (%lld)", (int)slots,
           (long long)(slots * 8), (long long)budget);
    P.table.tier = TIER_HBM;
  }
  return P;
}

}  // namespace

bool is_histogram_agg(const pg_agg_spec& s) { return s.function == PG_AGG_HISTOGRAM; }
void histogram_plan_check(Segment& seg, const pg_query& q) { (void)hist_plan(seg, q); }

std::unique_ptr<Result> execute_histogram(Segment& seg, const pg_query& q, const CancelToken* cancel) {
  SumTablePass pass(seg, q, kWho, cancel);
  const HistPlan P = hist_plan(seg, q);
  PgHistArgs A;
  int64_t doc_bits = pass.begin(P.table, A);
  A.n_cols = (int32_t)P.cols.size();
  for (size_t i = 0; i < P.cols.size(); i++) {
    const HistColumn& hc = P.cols[i];
    PgHistCol& C = A.cols[i];
    expr_fill_src(C.src, *hc.col);
    C.spec = hc.spec.device(nullptr);
    C.first_slot = hc.first_slot;
    C.edge_off = hc.edge_off;
    doc_bits += value_src_bits(*hc.col);
  }
  // the edge lists and, behind them, the flag of the docs on which the reference throws
  const size_t edge_bytes = P.edges.size() * 8;
  DeviceBuffer side(edge_bytes + 8);
  A.edges = side.as<double>();
  A.n_edges = (int32_t)P.edges.size();
  A.throws = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(side.ptr) + edge_bytes);
  A.combine_rounds = knobs().hist_combine_rounds >= 0 ? (int32_t)knobs().hist_combine_rounds : PG_HIST_COMBINE_ROUNDS;
  // LDS: the tier's table — pg_hist_one: as many 32-bit copies of the row as fit, at most one per wavefront — and the edges where they fit behind it
  size_t table_bytes = 0;
  A.copies = 1;
  if (P.table.tier == TIER_LDS) {
    table_bytes = (size_t)P.table.n_slots * 8;
    A.stage_edges = edge_bytes > 0 && table_bytes + edge_bytes <= PG_HIST_LDS_MAX_BYTES;
  } else if (P.table.tier == TIER_REG) {
    A.copies = (int32_t)std::max<int64_t>(1, std::min<int64_t>(PG_HIST_ONE_WAVES, PG_HIST_ONE_LDS_BYTES / ((int64_t)P.table.slots * 4)));
    table_bytes = ((size_t)A.copies * (size_t)P.table.slots * 4 + 7) / 8 * 8;
    A.stage_edges = edge_bytes > 0 && edge_bytes <= PG_HIST_ONE_EDGE_BYTES;
  }
  const size_t lds_bytes = table_bytes + (A.stage_edges ? edge_bytes : 0);
  // the walk keeps one load per wavefront in flight: what it needs is wavefronts.  pg_hist_lds: as many workgroups of 8 per CU as its LDS
  // admits, at most the CU's 32 wavefronts; pg_hist_one: two workgroups of PG_HIST_ONE_WAVES, persistent like the LDS tier's
  const int64_t lds_wgs_per_cu = std::max<int64_t>(1, std::min<int64_t>(4, PG_HIST_LDS_MAX_BYTES / (int64_t)std::max<size_t>(lds_bytes, 1)));
  bool launched = false;
  pass.accumulate(
      [&](int tier, int grid, hipStream_t stream) {
        if (edge_bytes) PG_HIP(hipMemcpyAsync(side.ptr, P.edges.data(), edge_bytes, hipMemcpyHostToDevice, stream));
        PG_HIP(hipMemsetAsync(A.throws, 0, 8, stream));
        if (tier == TIER_REG) grid = std::min(grid, 2 * device_cus(seg.device));
        pg_hist_launch_pass(&A, tier, grid, lds_bytes, stream);
        launched = true;
      },
      lds_wgs_per_cu, -1);
  if (launched) {   // (the gather has drained the stream)
    uint32_t thrown = 0;
    PG_HIP(hipMemcpy(&thrown, A.throws, 4, hipMemcpyDeviceToHost));
    if (thrown == (uint32_t)(-PG_HIST_THROWS_NAN))
      fail(PG_ERR_UNSUPPORTED, "HISTOGRAM over a matching doc whose value is NaN: the reference's bin search runs past the last bin and throws; the Java plan answers such a query");
    if (thrown)
      fail(PG_ERR_UNSUPPORTED, "HISTOGRAM over a matching doc whose equal-width bin index floor((x - lower) / binLength) rounds up to numBins: the reference throws; the Java plan answers such a query");
  }
  // ---- the arrays: numBins counts per group, a row of zeros for a group (or a query without GROUP BY) whose docs all fell outside ----------
  const int32_t n_rows = pass.n_rows();
  std::vector<AggResult> out((size_t)q.n_aggregations);
  for (const HistColumn& hc : P.cols) {
    AggResult r;
    r.kind = PG_RESULT_DOUBLE_ARRAY;
    const int32_t nb = hc.spec.n_bins;
    r.set_sizes.assign((size_t)n_rows, nb);
    r.d[0].resize((size_t)n_rows * (size_t)nb);
    for (int32_t i = 0; i < n_rows; i++) {
      const int64_t* bins = pass.row(i) + hc.first_slot;
      for (int32_t b = 0; b < nb; b++) {
        if (bins[b] < 0) fail(PG_ERR_INTERNAL, "%s: a bin counts %lld docs", kWho, (long long)bins[b]);
        r.d[0][(size_t)i * (size_t)nb + (size_t)b] = (double)bins[b];
      }
    }
    side_share_result(out, hc.aggs, std::move(r));
  }
  return pass.finish(out, kTierKernel[P.table.tier], doc_bits, MERGED_HISTOGRAM);
}

}  // namespace pg
