"""Every kernel name `dispatch` and its neighbours in pinot_amd/csrc/pg_exec.hip can report in pg_exec_stats.kernel, tied to one query
that reaches it: the segment it runs on, the entry point, the SQL, the knobs, an optional upsert snapshot, and the sizes of the ladder at which
the planner picks that kernel.  Data plus small helpers; tests/test_kernel_inventory.py checks it against pg_exec.hip on the CPU,
tests/test_gpu_kernel_matrix.py runs it against the oracle on the GPU."""
import os
import re
from dataclasses import dataclass, field
from typing import Dict, Optional, Tuple

import numpy as np

from pinot_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXEC_SOURCE = os.path.join(ROOT, "pinot_amd", "csrc", "pg_exec.hip")
KERNEL_NAME = re.compile(r'"(pg_[a-z0-9_]+)"')
KERNEL_FIELD_BYTES = 32            # pg_exec_stats.kernel is char[32]: 31 characters and the terminator

# Segment sizes: none is a multiple of the 2 048-doc wave tile.  49 929 = 3 x PG_TILE_DOCS + 777.
LADDER = (2_047, 49_929, 700_001, 2_500_003)
LARGE = 700_001
ALL = LADDER
# The fused index kernels need every posting leaf dense: bitmap containers (> 4 096 docs of the value) in every 2^16-doc chunk.  2 047 docs
# keep array containers; so does the short last chunk of 2 500 003 docs (9 635 docs: ~1 200 per value of c_inv1), where the planner falls back
# to the tile walk over the interpreted index (pg_fast_none_* / pg_fast_multi_*).
INDEXED = (49_929, 700_001)
DENSE = (49_929, 700_001, 2_500_003)
BIG = (700_001, 2_500_003)


def kernel_names_in_source(path: str = EXEC_SOURCE):
    """Every full string literal "pg_[a-z0-9_]+" of pg_exec.hip: the names the executor can report."""
    with open(path) as f:
        return set(KERNEL_NAME.findall(f.read()))


@dataclass(frozen=True)
class Entry:
    name: str                                  # the kernel pg_exec_stats.kernel must report
    builder: str                               # key of BUILDERS
    sql: str
    sizes: Tuple[int, ...]
    entry: str = "execute"                     # execute | filter (pg_filter_exec, DocIdSet.stats()) | distinct | selection
    knobs: Dict[str, str] = field(default_factory=dict)   # PG_* variables, applied through the gpu_knobs fixture
    snapshot: bool = False                     # run behind the upsert snapshot of `snapshot_doc_ids`
    exact: bool = True                         # QUERY_FLAG_EXACT_FILTER_STATS
    groups_limit: Optional[int] = None         # numGroupsLimit, where the default would trim or refuse the query


# ---- segment builders: (num_docs) -> HostSegment ---------------------------------------------------------------------------------
BENCH_COLUMNS = ["c_inv1", "c_inv2", "r_int", "g1", "g2", "m", "r_int_d", "m_d", "r_int_s", "m_s", "h1", "h2", "h3", "h4", "u"]


def _bench(n):
    return synth.generate_segment(n, segment_index=3, columns=BENCH_COLUMNS)


def _wide(n):
    from tests.fixtures import wide_segment
    return wide_segment(n)


def _mvg(n):
    from tests.mv_fixture import group_table
    return group_table(n, seed=n)


BUILDERS = {"bench": _bench, "wide": _wide, "mvg": _mvg}


def snapshot_doc_ids(n: int, seed: int = 17) -> np.ndarray:
    """An upsert queryableDocIds snapshot: 90 % of the docs (bitmap containers, the dense form the snapshot kernels take), never the last doc,
    and one doc missing inside the last partial 32-doc word and inside the last partial 64-doc word — set bits past numDocs or a tail word
    taken whole would show."""
    keep = np.random.default_rng(seed).random(n) < 0.9
    keep[n - 1] = False
    for w in (32, 64):
        start = n - n % w
        if start < n:
            keep[start + (n - 1 - start) // 2] = False
    return np.flatnonzero(keep)


IDX = "c_inv1 IN (0,1,2,3) AND c_inv2 IN (0,1)"
SPEC = {"PG_WAVE_SPECIALISED": "1"}
NO_SPEC = {"PG_NO_WAVE_SPECIALISED": "1"}
SPECW = {"PG_SPECW": "1"}
NO_DMA = {"PG_SPECD_NO_DMA": "1"}

E = Entry
ENTRIES = [
    # ---- raw INT scan / value columns: pg_kernels.hip, pg_kernels_scan.hip, pg_kernels_dense.hip, pg_kernels_pipe.hip, pg_kernels_spec.hip ----
    E("pg_fast_i32range_fp", "bench", synth.QUERY_CFG2, ALL),
    E("pg_fast_i32range_f", "bench", "SELECT COUNT(*) FROM gpuBench WHERE c_inv1 IN (0,1,2,3) AND r_int BETWEEN 100000 AND 899999", ALL, entry="filter"),
    E("pg_fast_i32range_a", "bench", "SELECT g1, SUM(m), MAX(r_int) FROM gpuBench WHERE r_int > 500000 GROUP BY g1 LIMIT 1000", ALL),
    E("pg_fast_i32range_d", "bench", "SELECT g1, SUM(m), MAX(r_int) FROM gpuBench WHERE c_inv1 IN (0, 1) AND r_int > 500000 GROUP BY g1 LIMIT 1000", INDEXED),
    E("pg_fast_i32range_p", "bench", synth.QUERY_CFG3, INDEXED, knobs=NO_SPEC),
    E("pg_fast_i32range_s", "bench", synth.QUERY_CFG3.replace("MAX(m)", "MIN(m)"), INDEXED, knobs=SPEC),
    E("pg_fast_i32range_st", "bench", synth.QUERY_CFG3.replace("MAX(m)", "COUNT(*)"), INDEXED, knobs=SPEC, snapshot=True),
    E("pg_pipe_index_scan_tail", "bench", synth.QUERY_CFG3.replace("MAX(m)", "MAX(m), MIN(m)"), INDEXED, knobs=NO_SPEC, snapshot=True),
    E("pg_pipe_none", "bench", "SELECT g1, SUM(m), MAX(m) FROM gpuBench GROUP BY g1 LIMIT 1000", ALL),
    E("pg_pipe_scan", "bench", "SELECT g1, g2, SUM(m) FROM gpuBench WHERE r_int BETWEEN 250000 AND 749999 GROUP BY g1, g2 LIMIT 10000", ALL),
    E("pg_pipe_index", "bench", "SELECT g1, SUM(m) FROM gpuBench WHERE c_inv1 IN (0, 1, 2, 3) AND c_inv2 IN (0, 1) GROUP BY g1 LIMIT 1000", INDEXED),
    E("pg_pipe_index2", "bench", "SELECT g2, g1, MAX(m), COUNT(*) FROM gpuBench WHERE c_inv1 NOT IN (3, 4) GROUP BY g2, g1 LIMIT 10000", INDEXED),
    E("pg_pipe_scan_vscan", "bench", "SELECT g1, SUM(m), COUNT(*) FROM gpuBench WHERE r_int BETWEEN 250000 AND 749999 AND m < 500000 GROUP BY g1 LIMIT 1000", ALL),
    E("pg_pipe_index_scan_vscan", "bench", f"SELECT g1, SUM(m), MAX(m) FROM gpuBench WHERE {IDX} AND r_int BETWEEN 250000 AND 749999 "
      "AND m >= 524288 GROUP BY g1 LIMIT 1000", INDEXED),
    E("pg_spec_none", "bench", "SELECT g1, MIN(m), MAX(m) FROM gpuBench GROUP BY g1 LIMIT 1000", ALL, knobs=SPEC),
    E("pg_spec_scan", "bench", "SELECT g1, SUM(m), COUNT(*) FROM gpuBench WHERE r_int < 70000 GROUP BY g1 LIMIT 1000", ALL, knobs=SPEC),
    E("pg_spec_index", "bench", "SELECT g1, MIN(m), SUM(m) FROM gpuBench WHERE c_inv1 IN (0, 1, 2, 3) GROUP BY g1 LIMIT 1000", INDEXED, knobs=SPEC),
    E("pg_nogroup_s1", "bench", "SELECT SUM(m), MIN(m), MAX(m), COUNT(*) FROM gpuBench", ALL),
    E("pg_nogroup_s2", "bench", "SELECT SUM(m), MAX(r_int), MIN(r_int), MINMAXRANGE(m), COUNT(*) FROM gpuBench", ALL),
    E("pg_fast_none_a", "bench", "SELECT g1, SUM(m), MAX(r_int) FROM gpuBench WHERE c_inv1 IN (1, 2) GROUP BY g1 LIMIT 1000", ALL),
    E("pg_fast_none_f", "bench", "SELECT COUNT(*) FROM gpuBench WHERE c_inv1 IN (1, 2)", ALL, entry="filter"),
    E("pg_dense_count", "bench", "SELECT COUNT(*) FROM gpuBench WHERE c_inv1 IN (0, 2) AND c_inv2 != 3", INDEXED),
    E("pg_dict_count", "bench", "SELECT COUNT(*) FROM gpuBench WHERE g2 BETWEEN 3 AND 30", ALL),
    E("pg_fast_multi_a", "bench", "SELECT g1, SUM(m), MAX(r_int) FROM gpuBench WHERE r_int < 600000 AND g2 BETWEEN 5 AND 40 GROUP BY g1 LIMIT 1000", ALL),
    E("pg_fast_multi_f", "bench", "SELECT COUNT(*) FROM gpuBench WHERE r_int < 600000 AND m > 1000", ALL, entry="filter"),
    E("pg_fast_dictrange_a", "bench", "SELECT g1, COUNT(*) FROM gpuBench WHERE g2 BETWEEN 10 AND 30 GROUP BY g1 LIMIT 1000", ALL),
    # (a lone dictionary range is pg_dictrange_fo's shape; the measurement knob PG_NO_SCAN_PIPE leaves it to the tile walk)
    E("pg_fast_dictrange_f", "bench", "SELECT COUNT(*) FROM gpuBench WHERE g2 BETWEEN 12 AND 40", ALL, entry="filter", knobs={"PG_NO_SCAN_PIPE": "1"}),
    E("pg_fast_dictlut_a", "bench", "SELECT g1, COUNT(*), SUM(m) FROM gpuBench WHERE g2 IN (3, 7, 11, 40) GROUP BY g1 LIMIT 1000", ALL),
    E("pg_fast_dictlut_f", "bench", "SELECT COUNT(*) FROM gpuBench WHERE g2 NOT IN (3, 7, 11, 40)", ALL, entry="filter"),
    E("pg_dictrange_fo", "bench", "SELECT COUNT(*) FROM gpuBench WHERE c_inv2 = 1 AND r_int_d BETWEEN 250000 AND 749999", ALL),
    # ---- the interpreter frame (pg_kernels.hip): an OR of an index leaf and a scan, the dense HBM table ----
    E("pg_generic_query_l", "bench", "SELECT g1, SUM(m) FROM gpuBench WHERE c_inv1 = 1 OR r_int < 1000 GROUP BY g1 LIMIT 1000", ALL),
    E("pg_generic_query_f", "bench", "SELECT COUNT(*) FROM gpuBench WHERE c_inv1 = 1 OR r_int < 1000", ALL, entry="filter"),
    E("pg_generic_query_g", "bench", "SELECT u, SUM(m), COUNT(*) FROM gpuBench WHERE c_inv1 = 2 AND r_int < 20000 GROUP BY u LIMIT 1000000", ALL,
      knobs={"PG_NO_RADIX": "1", "PG_NO_PART": "1"}, groups_limit=1_000_000),
    E("pg_generic_query_gd", "wide", "SELECT k, kq, SUM(dm) FROM wide WHERE inv = 3 AND r < 50 GROUP BY k, kq LIMIT 1000000", ALL,
      knobs={"PG_NO_RADIX": "1", "PG_NO_PART": "1"}, groups_limit=1_000_000),
    E("pg_generic_query_ld", "wide", "SELECT k2, SUM(dm), COUNT(*) FROM wide WHERE inv = 1 OR r < 100 GROUP BY k2", ALL),
    # ---- key spaces beyond one LDS table: pg_kernels_part.hip, pg_kernels_oct.hip ----
    E("pg_hash_group_by", "bench", "SELECT u, h1, h2, COUNT(*), SUM(h3) FROM gpuBench WHERE h4 = 1 AND h3 < 3 GROUP BY u, h1, h2 LIMIT 10000000", ALL,
      groups_limit=10_000_000),
    E("pg_radix_group_by", "bench", "SELECT h2, h1, h3, h4, COUNT(*), DISTINCTCOUNTHLL(u) FROM gpuBench GROUP BY h2, h1, h3, h4 LIMIT 20000", ALL,
      knobs={"PG_NO_P2": "1"}, groups_limit=100_000),
    E("pg_part_group_by", "bench", synth.QUERY_CFG5, ALL, groups_limit=100_000),
    E("pg_part_group_by_prefix", "bench", "SELECT u, COUNT(*) FROM gpuBench GROUP BY u LIMIT 1000000", BIG,
      knobs={"PG_LIMIT_PREFIX_MIN_DOCS": "4096"}, groups_limit=5000),
    E("pg_oct_pruned_group_by", "bench", "SELECT h1, h2, h3, h4, COUNT(*), DISTINCTCOUNTHLL(u) FROM gpuBench WHERE h2 < 5 AND u > 1000 "
      "GROUP BY h1, h2, h3, h4 LIMIT 20000", ALL, knobs={"PG_OCT_MIN_DOCS": "0"}, groups_limit=100_000),
    E("pg_oct_c", "bench", "SELECT h1, h2, h3, h4, COUNT(*) FROM gpuBench GROUP BY h1, h2, h3, h4 LIMIT 20000", ALL, knobs={"PG_OCT_COUNT_MIN_DOCS": "0"}),
    E("pg_oct_l", "bench", "SELECT h3, COUNT(*), DISTINCTCOUNTHLL(u) FROM gpuBench GROUP BY h3 LIMIT 1000", ALL),
    E("pg_oct_lm", "bench", "SELECT h3, DISTINCTCOUNTHLL(u) FROM gpuBench WHERE r_int < 500000 GROUP BY h3 LIMIT 100", ALL),
    # ---- dictionary-encoded scan / value columns, independent wavefronts: pg_kernels_specd.hip ----
    E("pg_fast_dictrange_s_a_dma", "bench", synth.QUERY_CFG3_DICT, INDEXED),
    E("pg_fast_dictrange_s_g_dma", "bench", synth.QUERY_CFG3_SPARSE, INDEXED),
    E("pg_fast_dictrange_s_r_dma", "bench", f"SELECT g1, SUM(m), MIN(m) FROM gpuBench WHERE {IDX} AND r_int_d BETWEEN 250000 AND 749999 "
      "GROUP BY g1 ORDER BY g1 LIMIT 1000", INDEXED),
    E("pg_fast_dictrange_s_a", "bench", f"SELECT g1, SUM(m_d), MIN(m_d) FROM gpuBench WHERE {IDX} AND r_int_d BETWEEN 250000 AND 749999 "
      "GROUP BY g1 LIMIT 1000", INDEXED, knobs=NO_DMA),
    E("pg_fast_dictrange_s_g", "bench", f"SELECT g2, COUNT(*), MIN(m_s), MAX(m_s), SUM(m_s) FROM gpuBench WHERE {IDX} AND r_int_s BETWEEN 750000 AND 2249999 "
      "GROUP BY g2 LIMIT 10000", INDEXED, knobs=NO_DMA),
    E("pg_fast_dictrange_s_r", "bench", f"SELECT g1, MAX(m), COUNT(*) FROM gpuBench WHERE {IDX} AND r_int_d BETWEEN 100 AND 900000 GROUP BY g1 LIMIT 1000",
      INDEXED, knobs=NO_DMA),
    E("pg_fast_dictrange_st_a", "bench", f"SELECT g1, SUM(m_d), COUNT(*) FROM gpuBench WHERE {IDX} AND r_int_d BETWEEN 250000 AND 749999 GROUP BY g1 LIMIT 1000",
      INDEXED, snapshot=True),
    E("pg_fast_dictrange_st_g", "bench", f"SELECT g1, SUM(m_s), MIN(m_s) FROM gpuBench WHERE {IDX} AND r_int_s BETWEEN 750000 AND 2249999 GROUP BY g1 LIMIT 1000",
      INDEXED, snapshot=True),
    E("pg_fast_dictrange_st_r", "bench", f"SELECT g1, SUM(m), MAX(m) FROM gpuBench WHERE {IDX} AND r_int_d BETWEEN 250000 AND 749999 GROUP BY g1 LIMIT 1000",
      INDEXED, snapshot=True),
    E("pg_specd_scan_a", "bench", "SELECT g1, g2, SUM(m_d) FROM gpuBench WHERE r_int_d BETWEEN 250000 AND 749999 GROUP BY g1, g2 LIMIT 10000", ALL),
    E("pg_specd_scan_g", "bench", "SELECT g1, SUM(m_s), COUNT(*) FROM gpuBench WHERE r_int_s < 600000 GROUP BY g1 LIMIT 1000", ALL),
    E("pg_specd_scan_r", "bench", "SELECT g1, SUM(m), COUNT(*) FROM gpuBench WHERE r_int_d > 500000 GROUP BY g1 LIMIT 1000", ALL),
    E("pg_specd_index_a", "bench", f"SELECT g1, SUM(m_d) FROM gpuBench WHERE {IDX} GROUP BY g1 LIMIT 1000", INDEXED),
    E("pg_specd_index_g", "bench", "SELECT g2, g1, MAX(m_s), COUNT(*) FROM gpuBench WHERE c_inv1 NOT IN (3, 4) GROUP BY g2, g1 LIMIT 10000", INDEXED),
    E("pg_specd_none_a", "bench", "SELECT g1, SUM(m_d), MAX(m_d) FROM gpuBench GROUP BY g1 LIMIT 1000", ALL),
    E("pg_specd_none_g", "bench", "SELECT g1, g2, COUNT(*), MIN(m_s) FROM gpuBench GROUP BY g1, g2 LIMIT 10000", ALL),
    # ---- ... in the shared-stage frame (PG_SPECW=1): pg_kernels_specw.hip ----
    E("pg_specw_none_a", "bench", "SELECT g2, SUM(m_d), MIN(m_d) FROM gpuBench GROUP BY g2 LIMIT 1000", ALL, knobs=SPECW),
    E("pg_specw_none_g", "bench", "SELECT g2, MAX(m_s), COUNT(*) FROM gpuBench GROUP BY g2 LIMIT 1000", ALL, knobs=SPECW),
    E("pg_specw_index_a", "bench", f"SELECT g2, SUM(m_d) FROM gpuBench WHERE {IDX} GROUP BY g2 LIMIT 1000", INDEXED, knobs=SPECW),
    E("pg_specw_index_g", "bench", "SELECT g2, MIN(m_s) FROM gpuBench WHERE c_inv1 NOT IN (2, 5) GROUP BY g2 LIMIT 1000", INDEXED, knobs=SPECW),
    E("pg_specw_scan_a", "bench", "SELECT g2, SUM(m_d), COUNT(*) FROM gpuBench WHERE r_int_d < 400000 GROUP BY g2 LIMIT 1000", ALL, knobs=SPECW),
    E("pg_specw_scan_g", "bench", "SELECT g2, SUM(m_s) FROM gpuBench WHERE r_int_s >= 1500000 GROUP BY g2 LIMIT 1000", ALL, knobs=SPECW),
    E("pg_specw_scan_r", "bench", "SELECT g2, SUM(m), MIN(m) FROM gpuBench WHERE r_int_d BETWEEN 100000 AND 800000 GROUP BY g2 LIMIT 1000", ALL, knobs=SPECW),
    E("pg_fast_dictrange_w_a", "bench", f"SELECT g2, SUM(m_d), MAX(m_d) FROM gpuBench WHERE {IDX} AND r_int_d BETWEEN 250000 AND 749999 GROUP BY g2 LIMIT 1000",
      INDEXED, knobs=SPECW),
    E("pg_fast_dictrange_w_g", "bench", f"SELECT g2, SUM(m_s), MAX(m_s) FROM gpuBench WHERE {IDX} AND r_int_s BETWEEN 750000 AND 2249999 GROUP BY g2 LIMIT 1000",
      INDEXED, knobs=SPECW),
    E("pg_fast_dictrange_w_r", "bench", f"SELECT g2, SUM(m), MAX(m) FROM gpuBench WHERE {IDX} AND r_int_d BETWEEN 250000 AND 749999 GROUP BY g2 LIMIT 1000",
      INDEXED, knobs=SPECW),
    E("pg_fast_dictrange_wt_a", "bench", f"SELECT g2, SUM(m_d), COUNT(*) FROM gpuBench WHERE {IDX} AND r_int_d BETWEEN 250000 AND 749999 GROUP BY g2 LIMIT 1000",
      INDEXED, knobs=SPECW, snapshot=True),
    E("pg_fast_dictrange_wt_g", "bench", f"SELECT g2, SUM(m_s), COUNT(*) FROM gpuBench WHERE {IDX} AND r_int_s BETWEEN 750000 AND 2249999 GROUP BY g2 LIMIT 1000",
      INDEXED, knobs=SPECW, snapshot=True),
    E("pg_fast_dictrange_wt_r", "bench", "SELECT g2, SUM(m), COUNT(*) FROM gpuBench WHERE c_inv2 = 1 AND r_int_d BETWEEN 250000 AND 749999 GROUP BY g2 LIMIT 1000",
      INDEXED, knobs=SPECW, snapshot=True),
    # ---- no GROUP BY, no filter, one dictionary-encoded INT column: pg_kernels_scan.hip ----
    E("pg_nogroup_da", "bench", "SELECT SUM(m_d), MIN(m_d), MAX(m_d), COUNT(*) FROM gpuBench", ALL),
    E("pg_nogroup_dg", "bench", "SELECT SUM(m_s), MIN(m_s), MAX(m_s), COUNT(*) FROM gpuBench", ALL),
    E("pg_nogroup_dl", "wide", "SELECT SUM(kq), MIN(kq), MAX(kq), COUNT(*) FROM wide", ALL),
    # ---- wide group columns, 64-bit and DOUBLE sources: the general aggregator (aggregate_wtile of pg_kernel_agg.h, in the kernels of pg_kernels.hip) and the wide pipeline (pg_kernels_pipe.hip) ----
    E("pg_fast_none_w", "wide", "SELECT k, SUM(lm), SUM(r) FROM wide GROUP BY k LIMIT 5000", ALL),
    E("pg_fast_none_wd", "wide", "SELECT k, SUM(dm), SUM(lm) FROM wide GROUP BY k LIMIT 5000", ALL),
    E("pg_fast_multi_w", "wide", "SELECT k, SUM(lm) FROM wide WHERE r < 900 AND lm > 0 GROUP BY k LIMIT 5000", ALL),
    E("pg_fast_multi_wd", "wide", "SELECT k, SUM(dm) FROM wide WHERE r < 900 AND lm > 0 GROUP BY k LIMIT 5000", ALL),
    E("pg_pipe_w0_none", "wide", "SELECT k, COUNT(*) FROM wide GROUP BY k LIMIT 5000", ALL),
    E("pg_pipe_w0_index", "wide", "SELECT k, COUNT(*) FROM wide WHERE inv IN (1, 3) GROUP BY k LIMIT 5000", INDEXED),
    E("pg_pipe_w0_scan", "wide", "SELECT k, COUNT(*) FROM wide WHERE r BETWEEN 100 AND 700 GROUP BY k LIMIT 5000", ALL),
    E("pg_pipe_w0_index_scan", "wide", "SELECT k, COUNT(*) FROM wide WHERE inv NOT IN (0, 4) AND r < 500 GROUP BY k LIMIT 5000", INDEXED),
    E("pg_pipe_w32_none", "wide", "SELECT k, MAX(r), SUM(r) FROM wide GROUP BY k LIMIT 5000", ALL),
    E("pg_pipe_w32_index", "wide", "SELECT k, SUM(r), MIN(r) FROM wide WHERE inv = 2 GROUP BY k LIMIT 5000", INDEXED),
    E("pg_pipe_w32_scan", "wide", "SELECT k, SUM(r), COUNT(*) FROM wide WHERE r BETWEEN 100 AND 700 GROUP BY k LIMIT 5000", ALL),
    E("pg_pipe_w32_index_scan", "wide", "SELECT k, MIN(r), COUNT(*) FROM wide WHERE inv IN (0, 2) AND r >= 300 GROUP BY k LIMIT 5000", INDEXED),
    E("pg_pipe_w64_none", "wide", "SELECT k, SUM(lm), MIN(lm), MAX(lm), COUNT(*) FROM wide GROUP BY k LIMIT 5000", ALL),
    E("pg_pipe_w64_index", "wide", "SELECT k2, SUM(lm) FROM wide WHERE inv IN (1, 3) GROUP BY k2", INDEXED),
    E("pg_pipe_w64_scan", "wide", "SELECT k, SUM(lm), MIN(lm) FROM wide WHERE r BETWEEN 100 AND 700 GROUP BY k LIMIT 5000", ALL),
    E("pg_pipe_w64_index_scan", "wide", "SELECT k2, MAX(lm), COUNT(*) FROM wide WHERE inv NOT IN (0, 4) AND r < 500 GROUP BY k2", INDEXED),
    E("pg_pipe_wd_none", "wide", "SELECT k, SUM(dm), MIN(dm), MAX(dm), COUNT(*) FROM wide GROUP BY k LIMIT 5000", ALL),
    E("pg_pipe_wd_index", "wide", "SELECT k, MINMAXRANGE(dm) FROM wide WHERE inv = 4 GROUP BY k LIMIT 5000", INDEXED),
    E("pg_pipe_wd_scan", "wide", "SELECT SUM(dm), MAX(dm), COUNT(*) FROM wide WHERE r BETWEEN 100 AND 700", ALL),
    E("pg_pipe_wd_index_scan", "wide", "SELECT k2, SUM(dm) FROM wide WHERE inv IN (1, 3) AND r < 900 GROUP BY k2", INDEXED),
    # ---- SELECT DISTINCT (pg_kernels_distinct.hip) and selection (pg_kernels_select.hip) ----
    E("pg_distinct_dictionary", "bench", "SELECT DISTINCT g1 FROM gpuBench LIMIT 50", ALL, entry="distinct"),
    E("pg_distinct_keys_lds", "bench", "SELECT DISTINCT g1, g2 FROM gpuBench WHERE c_inv1 IN (1, 2) ORDER BY g1, g2 LIMIT 10000", ALL, entry="distinct"),
    E("pg_distinct_keys_hbm", "bench", "SELECT DISTINCT u, g1 FROM gpuBench WHERE r_int < 500000 ORDER BY u DESC, g1 LIMIT 100", ALL, entry="distinct"),
    E("pg_select_empty", "bench", "SELECT g1, m FROM gpuBench WHERE c_inv1 = 3 LIMIT 0", ALL, entry="selection"),
    E("pg_select_gather", "bench", "SELECT g1, r_int, m FROM gpuBench WHERE c_inv2 = 1 AND r_int < 300000 LIMIT 500", ALL, entry="selection"),
    E("pg_select_topk_lds", "bench", "SELECT u, g1, m FROM gpuBench WHERE c_inv1 IN (1, 5) ORDER BY m DESC, u LIMIT 100", ALL, entry="selection"),
    E("pg_select_sort", "bench", "SELECT r_int, g2 FROM gpuBench WHERE c_inv2 = 2 ORDER BY r_int, g2 LIMIT 5000", DENSE, entry="selection"),
    # ---- multi-value columns: pg_kernels_mv.hip, pg_kernels_mvg.hip ----
    E("pg_mv_group_4", "mvg", "SELECT mvA, COUNT(*), SUM(m) FROM mvg GROUP BY mvA LIMIT 100", ALL),
    E("pg_mv_group_8", "mvg", "SELECT mvC, COUNT(*), SUM(m), MIN(m) FROM mvg GROUP BY mvC LIMIT 100", ALL),
    E("pg_mv_aggr_4", "mvg", "SELECT s1, SUMMV(mvA), COUNTMV(mvA), MAXMV(mvA), MINMV(mvA), COUNT(*) FROM mvg GROUP BY s1 LIMIT 100", ALL),
    E("pg_mv_aggr_8", "mvg", "SELECT md, MAXMV(mvB) FROM mvg GROUP BY md LIMIT 1000", ALL),
    E("pg_mv_query_l", "mvg", "SELECT mvA, COUNT(*), SUM(m) FROM mvg WHERE s1 < 3 GROUP BY mvA LIMIT 100", ALL),
    E("pg_mv_query_g", "mvg", "SELECT mvD, md, COUNT(*) FROM mvg WHERE s1 = 1 AND md < 20 GROUP BY mvD, md LIMIT 1000000", ALL,
      groups_limit=1_000_000),
    E("pg_mv_query_f", "mvg", "SELECT COUNT(*) FROM mvg WHERE mvS = 'k3'", ALL, entry="filter"),
]
del E

# Names the dispatcher holds but no query can reach, each with the planner / dispatcher condition that rules it out.
_TAIL_NEEDS_INDEX_AND_SCAN = (
    "pg_plan.cpp compile_plan: the pipeline sets pipe_tail only in the branch `fast_filter == 100 && n_fast_scans == 1 && tail_posting >= 0`, "
    "which also sets has_scan; tail_posting >= 0 needs an index-only prefix (`n_idx > 0`), so pipe_has_index == 1 too — a tail always comes "
    "with index AND scan, which dispatch names pg_pipe_index_scan_tail (or pg_fast_i32range_st)")
_RAW_VALUE_NEEDS_DICT_SCAN = (
    "pg_plan.cpp compile_plan (specd): `if (ok && vkind == 1 && (!has_scan || sbits == 32)) ok = false;` — a raw INT value column takes the "
    "specd / specw frame only behind a dictionary-encoded range scan, so the value-kind-r row's filter shapes without a scan (none, index) "
    "are never selected")
EXEMPT = {
    "pg_pipe_tail": _TAIL_NEEDS_INDEX_AND_SCAN,
    "pg_pipe_index_tail": _TAIL_NEEDS_INDEX_AND_SCAN,
    "pg_pipe_index2_tail": _TAIL_NEEDS_INDEX_AND_SCAN,
    "pg_pipe_scan_tail": _TAIL_NEEDS_INDEX_AND_SCAN,
    "pg_specd_none_r": _RAW_VALUE_NEEDS_DICT_SCAN,
    "pg_specd_index_r": _RAW_VALUE_NEEDS_DICT_SCAN,
    "pg_specw_none_r": _RAW_VALUE_NEEDS_DICT_SCAN,
    "pg_specw_index_r": _RAW_VALUE_NEEDS_DICT_SCAN,
}

BY_NAME = {e.name: e for e in ENTRIES}


def entries_at(n: int):
    return [e for e in ENTRIES if n in e.sizes]
