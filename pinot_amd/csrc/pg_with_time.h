// FIRSTWITHTIME / LASTWITHTIME: the order of (time, docId) as one unsigned maximum (shared by the kernels of pg_kernels_withtime.hip, the
// executor pg_exec_withtime.hip and a stand-alone CPU harness, tests/with_time_main.cpp; plain C++, no HIP types).
//
// The reference (LastWithTimeAggregationFunction.java:104-117,194-199, FirstWithTimeAggregationFunction.java:103-116,198-203) walks the
// matching docs in docId order and replaces its pair when  time >= best  (LAST) /  time <= best  (FIRST): among docs tied at the extreme
// time the GREATEST docId wins, for FIRST and for LAST alike.  The winner is therefore the maximum of a total order — order-free, exact, the
// same on every tier, grid and order of the atomics:
//   u            the order-preserving unsigned image of the time t (sign bit flipped): Long.MIN_VALUE -> 0, Long.MAX_VALUE -> 2^64 - 1
//   LAST         maximises (u, doc)
//   FIRST        maximises (~u, doc)
//
// PACKED mode (one pass).  The time column's range [tmin, tmax] is known at plan time.  With D = pg_wt_doc_bits(total_docs), the number of
// bits that hold total_docs - 1 (at least 1, at most 31), a doc's slot value is
//        ((rel + 1) << D) | doc,      rel = t - tmin (LAST),  rel = tmax - t (FIRST),   0 <= rel <= range = tmax - tmin
// and 0 means "no doc".  rel + 1 must fit the 64 - D bits above the doc:  range + 1 <= 2^(64 - D) - 1, that is
//        range <= PG_WT_PACKED_MAX_RANGE(D) = 2^(64 - D) - 2          (pg_wt_packed_max_range; the EXACT bound of pg_wt_packed_ok)
// At 10^6 docs (D = 20) this covers 2^44 - 2 time units.
//
// WIDE mode (two passes) covers every INT / LONG time column: pass 1 takes the maximum of the 64-bit order key per slot, pass 2 the maximum
// of doc + 1 over the docs whose key equals it, into a second plane.  A key of 0 or 2^64 - 1 is an ordinary time (Long.MIN_VALUE /
// Long.MAX_VALUE), so emptiness is decided from the doc plane alone: 0 there means "no doc".
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PG_WT_HD __host__ __device__ static inline
#else
#define PG_WT_HD static inline
#endif

#define PG_WT_MAX_SLOTS 4    // distinct (time column, direction) pairs of one query
#define PG_WT_MAX_AGGS 8     // FIRSTWITHTIME / LASTWITHTIME aggregations of one query
#define PG_WT_LDS_SLOTS 16384   // 64-bit slots of the LDS tier: 128 KiB of the CU's 160 KiB, one persistent workgroup per CU (as pg_var_lds)

// the bits that hold n_docs - 1 (n_docs >= 1): 1 for one or two docs, 31 for 2^31 - 1
PG_WT_HD int pg_wt_doc_bits(int64_t n_docs) {
  int d = 1;
  while (d < 63 && ((int64_t)1 << d) < n_docs) d++;
  return d;
}
// the order-preserving unsigned image of a time
PG_WT_HD uint64_t pg_wt_u(int64_t t) { return (uint64_t)t ^ 0x8000000000000000ULL; }
// the wide order key: greater = later (LAST) / earlier (FIRST)
PG_WT_HD uint64_t pg_wt_order_key(int64_t t, int first) { return first ? ~pg_wt_u(t) : pg_wt_u(t); }
PG_WT_HD int64_t pg_wt_time_of_key(uint64_t key, int first) { return (int64_t)((first ? ~key : key) ^ 0x8000000000000000ULL); }
// tmax - tmin as an unsigned number (tmin <= tmax; up to 2^64 - 1)
PG_WT_HD uint64_t pg_wt_range(int64_t tmin, int64_t tmax) { return (uint64_t)tmax - (uint64_t)tmin; }
// the largest range packed mode admits beside D doc bits (1 <= D <= 31)
PG_WT_HD uint64_t pg_wt_packed_max_range(int D) { return (~0ULL >> D) - 1ULL; }
PG_WT_HD int pg_wt_packed_ok(uint64_t range, int D) { return D >= 1 && D <= 31 && range <= pg_wt_packed_max_range(D); }
// a doc's distance from the losing end of the range: base = tmin for LAST, tmax for FIRST
PG_WT_HD uint64_t pg_wt_rel(int64_t t, int64_t base, int first) { return first ? (uint64_t)base - (uint64_t)t : (uint64_t)t - (uint64_t)base; }
PG_WT_HD uint64_t pg_wt_pack(uint64_t rel, uint32_t doc, int D) { return ((rel + 1ULL) << D) | (uint64_t)doc; }
PG_WT_HD uint32_t pg_wt_packed_doc(uint64_t v, int D) { return (uint32_t)(v & ((1ULL << D) - 1ULL)); }
PG_WT_HD uint64_t pg_wt_packed_rel(uint64_t v, int D) { return (v >> D) - 1ULL; }   // v != 0
PG_WT_HD int64_t pg_wt_time_of_rel(uint64_t rel, int64_t base, int first) { return (int64_t)(first ? (uint64_t)base - rel : (uint64_t)base + rel); }
