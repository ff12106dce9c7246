// HISTOGRAM on the device (HistogramAggregationFunction under pinot-core/.../aggregation/function/, its intermediate a DoubleArrayList of
// numBins counts).  Every matching doc's value is read as the reference's getDoubleValuesSV gives it, its bin decided by pg_hist_bin
// (pg_histogram.h: the single statement of getBinId, IEEE double operation by operation), and 1 added to that bin of its group's row — a
// table [G][slots] of int64, a row the concatenated bins of the query's distinct (column, bin specification) pairs.  Integer additions
// commute: the result does not depend on the tier, the grid or the order of the atomics.
//   pg_hist_lds   GROUP BY, up to PG_HIST_LDS_SLOTS slots: persistent workgroups (up to 4 per CU where their tables fit), 64-bit LDS atomics,
//                 one flush of the touched slots
//   pg_hist_hbm   beyond that, and a row without GROUP BY that has more than PG_HIST_LDS_SLOTS bins: global 64-bit atomics
//   pg_hist_one   no GROUP BY: every lane of a wavefront adds to one of numBins addresses, the case this code base has measured as
//                 pathological (64 lanes adding to ONE LDS slot).  The row is kept as 32-bit counts (a segment has fewer than
//                 2^31 docs) in `copies` copies, a wavefront adding to copy wave % copies, and the copies are folded into the int64 table
//                 at the end: conflicts stay inside a wavefront.  A 64-doc word whose docs all fall into one bin adds their number once
//                 (readfirstlane, ballot, popcount); beyond that `combine_rounds` can ask for the lanes of a mixed word that share a bin
//                 to be combined too, bin by bin — the first live lane's bin is broadcast, the lanes holding it are counted, one of them
//                 adds the count and they all leave —, which measured slower than the plain LDS atomics the remaining lanes take
//                 (PG_HIST_COMBINE_ROUNDS in pg_device.h, profiles/histogram_prof.txt).
// All three walk the filter's match words (none: every doc) with side_scan_walk of pg_side_scan.h; the tiers with GROUP BY run on
// side_sum_table_pass.  Equal-width bins need nothing but the value; the edge form's search is log2(edges) dependent loads per lane, from
// LDS where the edges fit behind the table (stage_edges), else from HBM.  A doc on which the reference throws (a NaN; an equal-width index
// that rounds up to numBins) is not counted: any lane that sees one stores its reason to `throws`, and the executor refuses the query.
// The specifications are kernel arguments: wave-uniform, scalar branches; no scratch (the resource log of this file is checked by
// tests/test_gpu_histogram.py).  The table is zeroed by a memset and its admitted rows are gathered by pg_expr_gather
// (pg_kernels_expr.hip).  Kernel names are stable; the executor reports the tier's (pg_exec_hist.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pg_internal.hpp"
#include "pg_histogram.h"
#include "pg_expr_device.h"
#include "pg_side_scan.h"

#define DEVFN __device__ __forceinline__

namespace {

// the edge lists copied behind the table's `table_bytes` of LDS (before the barrier that follows the table's initialisation)
DEVFN const double* hist_edges(const PgHistArgs& a, unsigned long long* lds, uint64_t table_bytes) {
  if (!a.stage_edges) return a.edges;   // wave-uniform
  double* e = reinterpret_cast<double*>(lds + (table_bytes + 7) / 8);
  for (uint32_t i = threadIdx.x; i < (uint32_t)a.n_edges; i += blockDim.x) e[i] = a.edges[i];
  return e;
}

// the bin of `doc` under column `c`, or PG_HIST_NONE; a doc the reference throws on raises the flag and counts nowhere
DEVFN int32_t hist_bin_of(const PgHistArgs& a, const PgHistCol& C, const double* edges, uint32_t doc) {
  pg_hist_spec s = C.spec;
  s.edges = edges + C.edge_off;
  const int32_t b = pg_hist_bin(s, expr_load(C.src, doc));
  if (b < PG_HIST_NONE) *a.throws = (uint32_t)(-b);
  return b;
}

// the tiers with GROUP BY: `row0` is the table's first slot — the workgroup's copy in LDS, or the table in HBM
template <typename Ptr>
DEVFN void hist_update(const PgHistArgs& a, const double* edges, Ptr row0, uint32_t doc) {
  const uint64_t g = pg_scan_group_key(a.scan, doc);
  if (g >= a.n_groups) return;   // (ids below their cardinalities never are)
  Ptr row = row0 + g * (uint64_t)a.slots;
#pragma unroll 1
  for (int c = 0; c < a.n_cols; c++) {   // wave-uniform
    const PgHistCol& C = a.cols[c];
    const int32_t b = hist_bin_of(a, C, edges, doc);
    if (b >= 0) atomicAdd(reinterpret_cast<unsigned long long*>(&row[C.first_slot + b]), 1ULL);
  }
}

}  // namespace

extern "C" __global__ void __launch_bounds__(512) pg_hist_lds(const PgHistArgs a) {
  extern __shared__ unsigned long long side_lds[];
  const double* edges = hist_edges(a, side_lds, a.n_slots * 8);
  side_sum_table_pass<true>(a.scan, a.n_slots, a.table, [&](int64_t* row0, uint32_t doc) PG_SIDE_INLINE { hist_update(a, edges, row0, doc); });
}
extern "C" __global__ void __launch_bounds__(256) pg_hist_hbm(const PgHistArgs a) {
  side_sum_table_pass<false>(a.scan, a.n_slots, a.table, [&](int64_t* row0, uint32_t doc) PG_SIDE_INLINE { hist_update(a, a.edges, row0, doc); });
}

// No GROUP BY, a row of up to PG_HIST_LDS_SLOTS bins: `copies` copies of the row as 32-bit counts in LDS, the edges behind them.
extern "C" __global__ void __launch_bounds__(64 * PG_HIST_ONE_WAVES) pg_hist_one(const PgHistArgs a) {
  extern __shared__ unsigned long long side_lds[];
  uint32_t* counts = reinterpret_cast<uint32_t*>(side_lds);
  const SideWave at = side_wave();
  const uint32_t slots = (uint32_t)a.slots, total = slots * (uint32_t)a.copies;
  const double* edges = hist_edges(a, side_lds, (uint64_t)total * 4);
  for (uint32_t i = threadIdx.x; i < total; i += blockDim.x) counts[i] = 0;
  __syncthreads();
  uint32_t* mine = counts + (uint32_t)(at.wave % a.copies) * slots;
  const int rounds = a.combine_rounds;
  side_scan_walk(a.scan, at, [&](uint32_t doc) PG_SIDE_INLINE {
#pragma unroll 1
    for (int c = 0; c < a.n_cols; c++) {   // wave-uniform
      const PgHistCol& C = a.cols[c];
      const int32_t b = hist_bin_of(a, C, edges, doc);
      bool live = b >= 0;
      if (rounds > 0) {   // wave-uniform
        // a word whose docs all fall into one bin (or all outside): one add of their number by the first of them
        const unsigned long long docs = __ballot(1);
        const int32_t first = __builtin_amdgcn_readfirstlane(b);
        if (__ballot(b == first) == docs) {
          if (live && at.lane == __ffsll((long long)docs) - 1) atomicAdd(&mine[C.first_slot + first], (uint32_t)__popcll(docs));
          live = false;
        }
        // else, beyond one round, the lanes that share a bin: one add of their number by the first of them, for the first `rounds` distinct
        // bins of the word
        for (int r = 0; rounds > 1 && r < rounds; r++) {
          if (!__any(live)) break;
          if (live) {
            const int32_t head = __builtin_amdgcn_readfirstlane(b);
            const bool same = b == head;
            const unsigned long long holders = __ballot(same);
            if (same) {
              if (at.lane == __ffsll((long long)holders) - 1) atomicAdd(&mine[C.first_slot + head], (uint32_t)__popcll(holders));
              live = false;
            }
          }
        }
      }
      if (live) atomicAdd(&mine[C.first_slot + b], 1u);
    }
  });
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < slots; i += blockDim.x) {
    uint64_t v = 0;
    for (int k = 0; k < a.copies; k++) v += counts[(uint32_t)k * slots + i];
    if (v) atomicAdd(reinterpret_cast<unsigned long long*>(a.table + i), (unsigned long long)v);
  }
}

// ---- launcher (pg_exec_hist.hip) --------------------------------------------------------------------------------------------------------------
// `lds_bytes`: the tier's table (pg_hist_one: its copies) and the staged edges
void pg_hist_launch_pass(const PgHistArgs* args, int tier, int grid, size_t lds_bytes, hipStream_t stream) {
  if (tier == pg::TIER_LDS) {
    PG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(pg_hist_lds), hipFuncAttributeMaxDynamicSharedMemorySize, PG_HIST_LDS_MAX_BYTES));
    hipLaunchKernelGGL(pg_hist_lds, dim3(grid), dim3(512), lds_bytes, stream, *args);
  } else if (tier == pg::TIER_HBM) {
    hipLaunchKernelGGL(pg_hist_hbm, dim3(grid), dim3(256), 0, stream, *args);
  } else {
    PG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(pg_hist_one), hipFuncAttributeMaxDynamicSharedMemorySize, PG_HIST_ONE_LDS_BYTES + PG_HIST_ONE_EDGE_BYTES));
    hipLaunchKernelGGL(pg_hist_one, dim3(grid), dim3(64 * PG_HIST_ONE_WAVES), lds_bytes, stream, *args);
  }
}
