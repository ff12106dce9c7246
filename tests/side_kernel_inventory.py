"""Every kernel name the side passes can report in pg_exec_stats.kernel — the string literals of pg_exec_expr.hip, pg_exec_var.hip,
pg_exec_covar.hip, pg_exec_moment.hip, pg_exec_hist.hip, pg_exec_withtime.hip and pg_exec_percentile.hip — tied to queries that reach it:
the family whose model checks the answer, the select list, the GROUP BY, the columns read, the tier, the sizes of the ladder
(tests/kernel_inventory.py), the knobs and an optional upsert snapshot.  MODE and CASE WHEN report their host families' kernels and have
rows of their own.

The side passes walk the filter's match words with a grid-stride loop under a capped grid, so below a tier's WRAP POINT — cap x words per
workgroup x 64 docs — no workgroup ever takes a second step, folds a second stretch of the segment into its LDS copy or carries register
accumulators across iterations.  wrap_point() derives every tier's from the constants of the sources, for a device of `cus` compute units;
tests/test_side_kernel_inventory.py holds every entry to a size beyond its own, tests/test_gpu_side_scale.py runs the entries."""
import os
import re
from dataclasses import dataclass, field
from typing import Dict, Tuple

import numpy as np

from pinot_amd.segment import build_segment
from tests import covariance_model as cm
from tests import fourth_moment_model as fm
from tests import variance_model as vm
from tests import with_time_model as wm
from tests.kernel_inventory import KERNEL_NAME, LADDER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pinot_amd", "csrc")
EXEC_SOURCES = {"expression": "pg_exec_expr.hip", "variance": "pg_exec_var.hip", "covariance": "pg_exec_covar.hip", "moment": "pg_exec_moment.hip",
                "histogram": "pg_exec_hist.hip", "with_time": "pg_exec_withtime.hip", "percentile": "pg_exec_percentile.hip"}
# the family whose kernels a query kind runs on
HOST_FAMILY = {"mode": "percentile", "case": "expression"}
FAMILIES = tuple(EXEC_SOURCES) + tuple(HOST_FAMILY)
ASSUMED_CUS = 256   # the MI355X; tests/test_gpu_side_scale.py recomputes the wrap points if the device has more
SMALL, MID, BIG = LADDER[0], LADDER[2], LADDER[3]
DOCS_PER_WORD = 64


def _source(name: str) -> str:
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def kernel_names_in_sources() -> Dict[str, set]:
    """family -> every full string literal "pg_[a-z0-9_]+" of its executor source"""
    return {family: set(KERNEL_NAME.findall(_source(path))) for family, path in EXEC_SOURCES.items()}


# ---- the constants of the walk and of the grids, from the sources ----------------------------------------------------------------------------------
def _int(pattern: str, text: str, what: str) -> Tuple[int, ...]:
    m = re.search(pattern, text)
    assert m, f"{what}: the source no longer reads as the inventory expects ({pattern})"
    return tuple(int(g) for g in m.groups())


def launch_constants() -> dict:
    """what decides how many docs one grid step covers, read from the sources"""
    scan, side, dev = _source("pg_side_scan.h"), _source("pg_exec_sidepass.hip"), _source("pg_device.h")
    pk, pe, hist = _source("pg_kernels_percentile.hip"), _source("pg_exec_percentile.hip"), _source("pg_exec_hist.hip")
    c = {}
    (c["words_per_wave"],) = _int(r"constexpr int kWordsPerWave = (\d+);", scan, "pg_side_scan.h kWordsPerWave")
    # side_launch_pass: the LDS tier's workgroup, then the HBM tier's and the register tier's
    (c["lds_threads"],) = _int(r"hipLaunchKernelGGL\(lds, dim3\(grid\), dim3\((\d+)\), lds_bytes", scan, "side_launch_pass (LDS)")
    (c["hbm_threads"],) = _int(r"hipLaunchKernelGGL\(hbm, dim3\(grid\), dim3\((\d+)\), 0", scan, "side_launch_pass (HBM)")
    (c["reg_threads"],) = _int(r"hipLaunchKernelGGL\(reg, dim3\(grid\), dim3\((\d+)\), 0", scan, "side_launch_pass (registers)")
    # side_pass_grid: the words a workgroup is counted for and the caps
    c["grid_lds_words"], c["grid_words"] = _int(r"words_per_wg = tier == TIER_LDS \? (\d+) : (\d+);", side, "side_pass_grid words_per_wg")
    (c["wgs_per_cu"],) = _int(r"tier == TIER_LDS \? cus \* lds_wgs_per_cu : \(int64_t\)cus \* (\d+),", side, "side_pass_grid caps")
    # the workgroups per CU of the LDS tier, per family: a literal, or the most that min(., LDS budget / table) allows
    for family, path in (("expression", "pg_exec_expr.hip"), ("variance", "pg_exec_var.hip"), ("moment", "pg_exec_moment.hip")):
        (c["lds_wgs_" + family],) = _int(r"pass\.accumulate\(\[&\]\(int tier, int grid, hipStream_t stream\) \{ pg_\w+_launch_pass\(&A, tier, grid, stream\); \}, (\d+),",
                                         _source(path), path + " accumulate")
    (c["lds_wgs_covariance"],) = _int(r"lds_wgs = std::max<int64_t>\(1, std::min<int64_t>\((\d+), \(int64_t\)PG_COVAR_LDS_SLOTS / \(int64_t\)std::max<uint64_t>\(1, P\.table\.n_slots\)\)\);",
                                      _source("pg_exec_covar.hip"), "pg_exec_covar.hip lds_wgs")
    (c["lds_wgs_with_time"],) = _int(r"lds_wgs = std::max<int64_t>\(1, std::min<int64_t>\((\d+), \(int64_t\)PG_WT_LDS_SLOTS / \(int64_t\)std::max<uint64_t>\(1, P\.table\.n_slots\)\)\);",
                                     _source("pg_exec_withtime.hip"), "pg_exec_withtime.hip lds_wgs")
    (c["lds_wgs_histogram"],) = _int(r"lds_wgs_per_cu = std::max<int64_t>\(1, std::min<int64_t>\((\d+), PG_HIST_LDS_MAX_BYTES / \(int64_t\)std::max<size_t>\(lds_bytes, 1\)\)\);",
                                     hist, "pg_exec_hist.hip lds_wgs_per_cu")
    (c["hist_one_wgs_per_cu"],) = _int(r"if \(tier == TIER_REG\) grid = std::min\(grid, (\d+) \* device_cus\(seg\.device\)\);", hist, "pg_exec_hist.hip pg_hist_one grid")
    for name in ("PG_HIST_ONE_WAVES", "PG_HIST_LDS_MAX_BYTES", "PG_COVAR_LDS_SLOTS", "PG_PCTL_LDS_KEYS"):
        (c[name],) = _int(r"#define %s (\d+)" % name, dev, name)
    c["PG_WT_LDS_SLOTS"] = wm.header_constants()["PG_WT_LDS_SLOTS"]
    # the counting pass of PERCENTILE / MODE: its own walk and its own grid
    (c["pctl_words_per_wave"],) = _int(r"constexpr int kWordsPerWave = (\d+);", pk, "pg_kernels_percentile.hip kWordsPerWave")
    (c["pctl_lds_threads"],) = _int(r"hipLaunchKernelGGL\(pg_pctl_lds, dim3\(grid\), dim3\((\d+)\)", pk, "pg_pctl_launch_count (LDS)")
    (c["pctl_hbm_threads"],) = _int(r"hipLaunchKernelGGL\(pg_pctl_hbm, dim3\(grid\), dim3\((\d+)\)", pk, "pg_pctl_launch_count (HBM)")
    c["pctl_grid_lds_words"], c["pctl_grid_hbm_words"] = _int(r"words_per_wg = pc\.lds \? (\d+) : (\d+);", pe, "pg_exec_percentile.hip words_per_wg")
    (c["pctl_hbm_wgs_per_cu"],) = _int(r"std::min<int64_t>\(pc\.lds \? cus : cus \* (\d+),", pe, "pg_exec_percentile.hip grid caps")
    # the sort tier: one workgroup per tile of the segment, no cap
    assert re.search(r"hipLaunchKernelGGL\(pg_pctl_sort, dim3\(\(unsigned\)n_tiles\)", pk), "pg_pctl_sort no longer launches one workgroup per tile"
    return c


@dataclass(frozen=True)
class Entry:
    name: str                                  # the kernel pg_exec_stats.kernel must report
    family: str                                # whose model checks the answer: a key of EXEC_SOURCES or of HOST_FAMILY
    select: str                                # the aggregations
    reads: Tuple[str, ...]                     # the columns they read
    group_by: Tuple[str, ...] = ()
    tier: str = "reg"                          # reg | lds | hbm | sort
    table_slots: int = 0                       # LDS tier: the table's 64-bit slots, groups x slots of a row (PERCENTILE / MODE: 32-bit counters)
    sizes: Tuple[int, ...] = (SMALL, BIG)
    unfiltered: bool = True                    # also without a filter at the large sizes: the reference is exact and vectorised there
    knobs: Dict[str, str] = field(default_factory=dict)
    snapshot: bool = False                     # run behind the upsert snapshot of kernel_inventory.snapshot_doc_ids
    small_name: str = ""                       # the kernel at 2 047 docs, where the key column holds fewer groups than its space and the table fits LDS

    def kernel_at(self, n: int) -> str:
        return self.small_name if n == SMALL and self.small_name else self.name

    @property
    def host_family(self) -> str:
        return HOST_FAMILY.get(self.family, self.family)

    def sql(self, where: str = "") -> str:
        keys = ", ".join(self.group_by)
        return "SELECT " + (keys + ", " if keys else "") + self.select + " FROM t" + (" WHERE " + where if where else "") + (" GROUP BY " + keys if keys else "")


def lds_wgs_per_cu(e: Entry, c: dict) -> int:
    """the persistent workgroups per CU of an LDS-tier entry, by its family's expression"""
    f = e.host_family
    if f == "percentile":
        return 1
    if f == "histogram":   # equal-width histograms stage no edges: the table alone
        return max(1, min(c["lds_wgs_histogram"], c["PG_HIST_LDS_MAX_BYTES"] // max(e.table_slots * 8, 1)))
    if f in ("covariance", "with_time"):
        budget = c["PG_COVAR_LDS_SLOTS"] if f == "covariance" else c["PG_WT_LDS_SLOTS"]
        return max(1, min(c["lds_wgs_" + f], budget // max(e.table_slots, 1)))
    return c["lds_wgs_" + f]


def wrap_point(e: Entry, cus: int = ASSUMED_CUS, c: dict = None) -> int:
    """the docs one grid step of the entry's pass covers on `cus` compute units: cap x words per workgroup x 64.  0: no cap (pg_pctl_sort)"""
    c = c or launch_constants()
    if e.host_family == "percentile":
        if e.tier == "sort":
            return 0
        if e.tier == "lds":
            return cus * (c["pctl_lds_threads"] // 64 * c["pctl_words_per_wave"]) * DOCS_PER_WORD
        return cus * c["pctl_hbm_wgs_per_cu"] * (c["pctl_hbm_threads"] // 64 * c["pctl_words_per_wave"]) * DOCS_PER_WORD
    if e.tier == "lds":
        return cus * lds_wgs_per_cu(e, c) * (c["lds_threads"] // 64 * c["words_per_wave"]) * DOCS_PER_WORD
    if e.host_family == "histogram" and e.tier == "reg":   # pg_hist_one: persistent workgroups of PG_HIST_ONE_WAVES wavefronts
        return cus * c["hist_one_wgs_per_cu"] * (c["PG_HIST_ONE_WAVES"] * c["words_per_wave"]) * DOCS_PER_WORD
    threads = c["hbm_threads"] if e.tier == "hbm" else c["reg_threads"]
    return cus * c["wgs_per_cu"] * (threads // 64 * c["words_per_wave"]) * DOCS_PER_WORD


# ---- key spaces: the last that fits each family's LDS slots, and one group more -------------------------------------------------------------------------
_KV, _KM, _KC = vm.header_constants(), fm.header_constants(), cm.header_constants()
LDS_SLOTS = 16384                                                           # PG_{EXPR,VAR,COVAR,MOMENT,HIST,WT}_LDS_SLOTS: checked by the CPU test
VAR_DBL_ROW = 1 + _KV["PG_VAR_SUM_LIMBS"] + _KV["PG_VAR_SQ_LIMBS"]          # the doc count, the limbs of Sx and of Sq: 11
VAR_INT_ROW = 1 + _KV["PG_VAR_INT_SLOTS"]                                   # 4
M4_DBL_ROW, M4_INT_ROW = 1 + _KM["PG_M4_DBL_SLOTS"], 1 + _KM["PG_M4_INT_SLOTS"]   # 32, 11
COVAR_INT_LONG_ROW = cm.slots_per_group(["INT", "LONG"], 1, _KC)            # 11
EXPR_SUM_ROW = 4                                                            # PG_EXPR_SUM_LIMBS
HIST_BINS = 64
PCTL_LDS_KEYS, MI_CARD = 32768, 100
K11, K32, K64, K4, K1, KP = (LDS_SLOTS // VAR_DBL_ROW, LDS_SLOTS // M4_DBL_ROW, LDS_SLOTS // HIST_BINS, LDS_SLOTS // EXPR_SUM_ROW, LDS_SLOTS,
                             PCTL_LDS_KEYS // MI_CARD)                      # 1489, 512, 256, 4096, 16384, 327
KEY_SPACES = tuple(k + d for k in (K11, K32, K64, K4, K1, KP) for d in (0, 1))
WIDE_KEYS = 50_000                                                          # kw: workgroups collide on few rows; on many under the small key spaces
PCTL_SORT = {"PG_PCTL_HBM_MAX_BYTES": "4"}                                  # no dense table fits: the sort tier


def kfit(k: int) -> str:
    return "k%d" % k


def kover(k: int) -> str:
    return "k%d" % (k + 1)


# ---- the time columns of FIRSTWITHTIME / LASTWITHTIME: (min, max) as the segment registers them ------------------------------------------------------
TIME_RANGE = {
    "tp": (1_700_000_000_000 - 1, 1_700_000_000_000 + 49 * 10**9 + 2),   # packed at every size
    "tw": (wm.LONG_MIN, wm.LONG_MAX),                                     # never packed: the two-pass route
    "tm": (-12345, -12345 + 2**45),                                       # packed up to 20 011 docs (15 doc bits), two passes at 2 500 003 (22)
}


def planted_docs(n: int, wrap: int):
    """two triples of docs — in the first 64-doc word, in a word of the second grid step (past `wrap`) and in the last word — that share the
    greatest and the smallest time of tp and tm: the docId tie-break is decided across workgroups"""
    mid = wrap + 70 if n > wrap + 200 else n // 2
    return (5, mid, n - 2), (7, mid + 5, n - 3)


def scale_data(n: int, columns=None, wrap: int = 2_097_152):
    """(host segment, data, schema) of `n` docs with the columns named (all by default).  The argument columns follow tests/test_gpu_moments.py:
    the FLOAT / DOUBLE ones inside the models' exact windows, ri[0] = -2^31, rl[0] a LONG that is no double."""
    rng = np.random.default_rng(4099 + n)
    idx = np.arange(n)
    sign = lambda: np.where(rng.integers(0, 2, n) == 0, -1.0, 1.0)   # noqa: E731
    last_ties, first_ties = planted_docs(n, wrap)
    make = {
        "g7": lambda: rng.integers(0, 7, n).astype(np.int32),
        "s": lambda: rng.integers(0, 1000, n).astype(np.int32),                    # the selector: s < 16 is sparse and spread
        "c_inv1": lambda: rng.integers(0, 8, n).astype(np.int32),                  # inverted index
        "srt": lambda: (idx // 4).astype(np.int32),                                # sorted: a docId range as a value range
        "rk": lambda: (rng.integers(0, 50, n) * 1000 - 7).astype(np.int32),        # a raw key: its groups come back as values
        "kw": lambda: rng.integers(0, WIDE_KEYS, n).astype(np.int32),
        "xi": lambda: rng.integers(-5000, 5000, n).astype(np.int32) * 400_003,
        "ri": lambda: rng.integers(-2**31, 2**31 - 1, n, dtype=np.int64).astype(np.int32),
        "xl": lambda: rng.integers(-300, 300, n).astype(np.int64) * 10**15 + 1,
        "rl": lambda: rng.integers(-2**62, 2**62, n, dtype=np.int64),
        "xf": lambda: (rng.choice(rng.uniform(1.0, 1000.0, 97), n) * sign()).astype(np.float32),
        "rf": lambda: (rng.uniform(1.0, 1000.0, n) * sign()).astype(np.float32),
        "xd": lambda: rng.choice(rng.uniform(1e-3, 1.0, 211), n) * sign(),
        "rd": lambda: 1e9 + rng.standard_normal(n),
        "hi": lambda: rng.integers(-50, 1051, n).astype(np.int32),                 # HISTOGRAM arguments: some docs outside [0, 1000]
        "hrd": lambda: rng.uniform(-50.0, 1050.0, n),
        "mi": lambda: rng.permutation(idx % MI_CARD).astype(np.int32) * 3,         # MODE / PERCENTILE arguments: MI_CARD values
        "v16": lambda: rng.integers(0, 60_000, n).astype(np.int32),
        "mrl": lambda: np.array([2**53 + 1, 2**53 + 2, 2**53 + 3, -2**53 - 1, 5, -5], dtype=np.int64)[rng.integers(0, 6, n)],
        "mrd": lambda: np.array([0.0, -0.0, np.inf, -np.inf, 0.1, 2.5, -7.25, 1e30])[rng.integers(0, 8, n)],
        "td": lambda: rng.integers(-4, 5, n).astype(np.int32) * 1000,              # nine distinct times: every group ties at its extremes
        "tp": lambda: rng.integers(0, 50, n).astype(np.int64) * 10**9 + 1_700_000_000_000,
        "tw": lambda: rng.integers(-2**62, 2**62, n, dtype=np.int64),
        "tm": lambda: rng.integers(-12345 + 1, -12345 + 2**45, n, dtype=np.int64),
    }
    for k in KEY_SPACES:
        make["k%d" % k] = lambda k=k: (idx % k).astype(np.int32)
    schema_of = {"xl": "LONG", "rl": "LONG", "xf": "FLOAT", "rf": "FLOAT", "xd": "DOUBLE", "rd": "DOUBLE", "hrd": "DOUBLE", "mrl": "LONG", "mrd": "DOUBLE",
                 "tp": "LONG", "tw": "LONG", "tm": "LONG"}
    raw = ["rk", "ri", "rl", "rf", "rd", "hrd", "mrl", "mrd", "tp", "tw", "tm"]
    names = [c for c in make if columns is None or c in columns]
    assert columns is None or set(columns) <= set(make), sorted(set(columns) - set(make))
    data = {c: make[c]() for c in names}
    if n > 8:
        if "s" in data:                                  # the sparse filter reaches the first and the last match word, behind the snapshot too
            data["s"][[0, 1, 2, 3, n - 5, n - 4, n - 3, n - 2]] = 7
        if "ri" in data:
            data["ri"][0] = -2**31                       # the INT whose powers are largest
        if "rl" in data:
            data["rl"][0] = 2**62 + 1                    # a LONG that is no double
        if "mrd" in data:
            data["mrd"][: n // 3] = 2.5                  # the mode
            data["mrd"][n // 2] = np.nan                 # one NaN: a key of its own, the greatest
        if "tw" in data:                                 # the extremes, many times each: ties at both ends, in every workgroup
            data["tw"][rng.integers(0, n, max(2, n // 20))] = wm.LONG_MIN
            data["tw"][rng.integers(0, n, max(2, n // 20))] = wm.LONG_MAX
        for t in ("tp", "tm"):
            if t in data:
                data[t][list(first_ties)] = TIME_RANGE[t][0]
                data[t][list(last_ties)] = TIME_RANGE[t][1]
        if "g7" in data:                                 # the tied docs share their g7 group
            data["g7"][list(first_ties) + list(last_ties)] = 3
    schema = {c: schema_of.get(c, "INT") for c in names}
    host = build_segment("side_scale_%d" % n, data, schema, inverted_index_columns=[c for c in ("c_inv1",) if c in data],
                         no_dictionary_columns=[c for c in raw if c in data])
    return host, data, schema


FILTER_COLUMNS = ("s", "c_inv1", "srt")
SPARSE = "s < 16"                      # ~1.6 % of the docs, spread over the whole segment
SMALL_FILTERS = ("s < 500", "c_inv1 IN (1, 5)")


def dense_filter(n: int, wrap: int) -> str:
    """every doc of ~3 000 docs just past the first grid step of the tier under test and of the last ~3 000 docs, nothing else: full match words
    on the second step and in the final partial word (srt = doc / 4)"""
    tail = (n - 3000) // 4
    if not 0 < wrap < n - 6200:
        return f"srt >= {tail}"
    return f"srt BETWEEN {wrap // 4} AND {wrap // 4 + 749} OR srt >= {tail}"


# ---- the entries ------------------------------------------------------------------------------------------------------------------------------------------
def _wt(fn, x, t, declared):
    return f"{fn}WITHTIME({x}, {t}, '{declared}')"


E = Entry
ENTRIES = [
    # ---- the variance family: pg_kernels_var.hip ----
    E("pg_var_reg", "variance", "VAR_POP(ri), STDDEV_SAMP(rl), COUNT(*)", ("ri", "rl")),
    E("pg_var_reg", "variance", "VAR_SAMP(rd), STDDEV_POP(xf), VAR_POP(rf), STDDEV_SAMP(xd)", ("rd", "xf", "rf", "xd"), unfiltered=False),
    E("pg_var_lds", "variance", "VAR_POP(xi), VAR_SAMP(xl)", ("xi", "xl"), ("g7",), "lds", 7 * (VAR_INT_ROW + VAR_DBL_ROW - 1), sizes=(SMALL, MID, BIG)),
    E("pg_var_lds", "variance", "STDDEV_POP(rd)", ("rd",), (kfit(K11),), "lds", K11 * VAR_DBL_ROW, unfiltered=False),
    E("pg_var_lds", "variance", "VAR_POP(rf), COUNT(*)", ("rf",), ("rk",), "lds", 50 * VAR_DBL_ROW, unfiltered=False),
    E("pg_var_hbm", "variance", "STDDEV_POP(rd), COUNT(*)", ("rd",), (kover(K11),), "hbm", unfiltered=False),
    E("pg_var_hbm", "variance", "VAR_POP(ri)", ("ri",), (kover(K4),), "hbm", small_name="pg_var_lds"),
    E("pg_var_hbm", "variance", "VAR_SAMP(xd)", ("xd",), ("kw",), "hbm", unfiltered=False),
    # ---- COVAR_POP / COVAR_SAMP: pg_kernels_covar.hip ----
    E("pg_covar_reg", "covariance", "COVAR_POP(ri, rl), COUNT(*)", ("ri", "rl")),
    E("pg_covar_reg", "covariance", "COVAR_SAMP(rd, xf)", ("rd", "xf"), unfiltered=False),
    E("pg_covar_reg_wide", "covariance", "COVAR_POP(ri, xi), COVAR_SAMP(rl, xl), COVAR_POP(xi, rl)", ("ri", "xi", "rl", "xl")),
    E("pg_covar_reg_wide", "covariance", "COVAR_POP(xd, rd), COVAR_SAMP(rf, xd)", ("xd", "rd", "rf"), unfiltered=False),
    E("pg_covar_lds", "covariance", "COVAR_POP(xi, xl)", ("xi", "xl"), ("g7",), "lds", 7 * COVAR_INT_LONG_ROW),
    E("pg_covar_lds", "covariance", "COVAR_SAMP(ri, rl)", ("ri", "rl"), (kfit(K11),), "lds", K11 * COVAR_INT_LONG_ROW),
    E("pg_covar_hbm", "covariance", "COVAR_SAMP(ri, rl), COUNT(*)", ("ri", "rl"), (kover(K11),), "hbm"),
    E("pg_covar_hbm", "covariance", "COVAR_POP(xd, rd)", ("xd", "rd"), ("kw",), "hbm", unfiltered=False),
    # ---- SKEWNESS / KURTOSIS: pg_kernels_moment.hip ----
    E("pg_moment_reg", "moment", "SKEWNESS(ri), KURTOSIS(rl), COUNT(*)", ("ri", "rl")),
    E("pg_moment_reg", "moment", "KURTOSIS(rd), SKEWNESS(xf), KURTOSIS(xd)", ("rd", "xf", "xd"), unfiltered=False),
    E("pg_moment_lds", "moment", "SKEWNESS(xi), KURTOSIS(xl)", ("xi", "xl"), ("g7",), "lds", 7 * (M4_INT_ROW + M4_DBL_ROW - 1), sizes=(SMALL, MID, BIG)),
    E("pg_moment_lds", "moment", "KURTOSIS(rd)", ("rd",), (kfit(K32),), "lds", K32 * M4_DBL_ROW, unfiltered=False),
    E("pg_moment_hbm", "moment", "KURTOSIS(rd), COUNT(*)", ("rd",), (kover(K32),), "hbm", unfiltered=False),
    E("pg_moment_hbm", "moment", "SKEWNESS(ri)", ("ri",), (kover(K11),), "hbm"),
    E("pg_moment_hbm", "moment", "SKEWNESS(xd)", ("xd",), ("kw",), "hbm", unfiltered=False),
    E("pg_moment_lds", "moment", "KURTOSIS(ri), SKEWNESS(rd)", ("ri", "rd"), ("g7",), "lds", 7 * (M4_INT_ROW + M4_DBL_ROW - 1), unfiltered=False, snapshot=True),
    # ---- HISTOGRAM: pg_kernels_hist.hip (up to four LDS workgroups per CU where their tables fit) ----
    E("pg_hist_one", "histogram", "HISTOGRAM(hi, 0, 1000, 10), HISTOGRAM(hrd, ARRAY[0, 0.1, 1, 2.5, 1000]), COUNT(*)", ("hi", "hrd")),
    E("pg_hist_lds", "histogram", "HISTOGRAM(hrd, 0, 1000, 10)", ("hrd",), ("g7",), "lds", 7 * 10),
    E("pg_hist_lds", "histogram", f"HISTOGRAM(hrd, 0, 1000, {HIST_BINS})", ("hrd",), (kfit(K64),), "lds", K64 * HIST_BINS),
    E("pg_hist_hbm", "histogram", f"HISTOGRAM(hi, 0, 1000, {HIST_BINS}), COUNT(*)", ("hi",), (kover(K64),), "hbm"),
    E("pg_hist_hbm", "histogram", "HISTOGRAM(hrd, 0, 1000, 10)", ("hrd",), ("kw",), "hbm"),
    E("pg_hist_hbm", "histogram", f"HISTOGRAM(hrd, 0, 1000, {LDS_SLOTS + 1})", ("hrd",), (), "hbm"),   # a row beyond pg_hist_one's LDS
    E("pg_hist_lds", "histogram", "HISTOGRAM(hi, 0, 1000, 10), COUNT(*)", ("hi",), ("g7",), "lds", 7 * 10, snapshot=True),
    # ---- PERCENTILE: pg_kernels_percentile.hip ----
    E("pg_pctl_lds", "percentile", "PERCENTILE(mi, 50), COUNT(*)", ("mi",), (), "lds", MI_CARD),
    E("pg_pctl_lds", "percentile", "PERCENTILE(mi, 95)", ("mi",), (kfit(KP),), "lds", KP * MI_CARD),
    E("pg_pctl_hbm", "percentile", "PERCENTILE(mi, 99), COUNT(*)", ("mi",), (kover(KP),), "hbm"),
    E("pg_pctl_hbm", "percentile", "PERCENTILE(mi, 50)", ("mi",), ("kw",), "hbm", unfiltered=False),
    E("pg_pctl_sort", "percentile", "PERCENTILE(mrd, 90)", ("mrd",), ("g7",), "sort", knobs=PCTL_SORT),
    # ---- MODE, on the counting pass of PERCENTILE ----
    E("pg_pctl_lds", "mode", "MODE(mi), COUNT(*)", ("mi",), (), "lds", MI_CARD),
    E("pg_pctl_lds", "mode", "MODE(mi, 'MAX')", ("mi",), (kfit(KP),), "lds", KP * MI_CARD),
    E("pg_pctl_lds", "mode", "MODE(mrd)", ("mrd",), ("g7",), "lds", 7 * 9),
    E("pg_pctl_hbm", "mode", "MODE(mi)", ("mi",), (kover(KP),), "hbm"),
    E("pg_pctl_hbm", "mode", "MODE(v16, 'AVG')", ("v16",), ("g7",), "hbm", small_name="pg_pctl_lds"),   # 7 x 60 000 counters; 7 x at most 2 047 on the small segment
    E("pg_pctl_sort", "mode", "MODE(mrl)", ("mrl",), ("g7",), "sort", knobs=PCTL_SORT),
    E("pg_pctl_lds", "mode", "MODE(mi, 'AVG'), COUNT(*)", ("mi",), ("g7",), "lds", 7 * MI_CARD, snapshot=True),
    # ---- SUM / MIN / MAX / AVG over expressions: pg_kernels_expr.hip ----
    E("pg_expr_reg", "expression", "SUM(add(ri,xi)), MIN(sub(ri,xi)), MAX(add(xi,hi))", ("ri", "xi", "hi")),
    E("pg_expr_reg", "expression", "SUM(mult(rd,xd)), AVG(div(rf,xd))", ("rd", "xd", "rf"), unfiltered=False),
    E("pg_expr_lds", "expression", "SUM(add(ri,xi)), MAX(sub(xi,ri))", ("ri", "xi"), ("g7",), "lds", 7 * (EXPR_SUM_ROW + 1)),
    E("pg_expr_lds", "expression", "SUM(add(xi,hi))", ("xi", "hi"), (kfit(K4),), "lds", K4 * EXPR_SUM_ROW),
    E("pg_expr_hbm", "expression", "SUM(add(xi,hi)), COUNT(*)", ("xi", "hi"), (kover(K4),), "hbm", small_name="pg_expr_lds"),
    E("pg_expr_hbm", "expression", "SUM(mult(rd,xd))", ("rd", "xd"), ("kw",), "hbm", unfiltered=False, small_name="pg_expr_lds"),
    # ---- CASE WHEN inside them ----
    E("pg_expr_reg", "case", "SUM(CASE WHEN xi > 0 THEN ri ELSE hi END), COUNT(*)", ("xi", "ri", "hi")),
    E("pg_expr_lds", "case", "SUM(CASE WHEN xi > 0 THEN rd ELSE xd END), MAX(CASE WHEN hi < 500 THEN xl ELSE rl END)", ("xi", "rd", "xd", "hi", "xl", "rl"), ("g7",), "lds",
      7 * (EXPR_SUM_ROW + 1), unfiltered=False),
    E("pg_expr_hbm", "case", "SUM(CASE WHEN hi >= 500 THEN xi ELSE 0 END)", ("hi", "xi"), (kover(K4),), "hbm", small_name="pg_expr_lds"),
    E("pg_expr_lds", "case", "SUM(CASE WHEN xi > 0 THEN ri ELSE hi END), MIN(CASE WHEN hi < 100 THEN xi ELSE ri END)", ("xi", "ri", "hi"), ("g7",), "lds",
      7 * (EXPR_SUM_ROW + 1), unfiltered=False, snapshot=True),
    # ---- FIRSTWITHTIME / LASTWITHTIME: pg_kernels_withtime.hip (up to four LDS workgroups per CU) ----
    E("pg_wt_reg", "with_time", _wt("FIRST", "ri", "tp", "INT") + ", " + _wt("LAST", "ri", "tp", "INT") + ", COUNT(*)", ("ri", "tp")),              # the packed pass
    E("pg_wt_reg", "with_time", _wt("FIRST", "rd", "tw", "DOUBLE") + ", " + _wt("LAST", "rl", "tw", "LONG"), ("rd", "rl", "tw")),                  # two passes
    E("pg_wt_reg", "with_time", _wt("LAST", "xi", "tm", "LONG") + ", " + _wt("FIRST", "rf", "tm", "FLOAT"), ("xi", "rf", "tm")),                  # packed only on small segments
    E("pg_wt_lds", "with_time", _wt("FIRST", "ri", "tp", "INT") + ", " + _wt("LAST", "rd", "td", "DOUBLE"), ("ri", "tp", "rd", "td"), ("g7",), "lds", 7 * 2),
    E("pg_wt_lds", "with_time", _wt("LAST", "ri", "tm", "INT") + ", " + _wt("FIRST", "ri", "tm", "INT"), ("ri", "tm"), ("g7",), "lds", 7 * 2),
    E("pg_wt_lds", "with_time", _wt("LAST", "ri", "td", "INT"), ("ri", "td"), (kfit(K1),), "lds", K1),
    E("pg_wt_hbm", "with_time", _wt("LAST", "ri", "td", "INT") + ", COUNT(*)", ("ri", "td"), (kover(K1),), "hbm", small_name="pg_wt_lds"),
    E("pg_wt_hbm", "with_time", _wt("FIRST", "rl", "tw", "LONG"), ("rl", "tw"), ("kw",), "hbm", unfiltered=False, small_name="pg_wt_lds"),
    E("pg_wt_lds", "with_time", _wt("LAST", "ri", "tp", "INT") + ", " + _wt("FIRST", "rl", "tw", "LONG") + ", COUNT(*)", ("ri", "tp", "rl", "tw"), ("g7",), "lds", 7 * 2,
      unfiltered=False, snapshot=True),
]
del E

# the families whose modules have no snapshot test of their own: each has an entry behind the snapshot
SNAPSHOT_FAMILIES = ("moment", "histogram", "mode", "with_time", "case")


def entries_at(n: int):
    return [e for e in ENTRIES if n in e.sizes]


def columns_at(n: int):
    """the columns the entries of size `n` need: their arguments, their keys and the filters'"""
    cols = set(FILTER_COLUMNS)
    for e in entries_at(n):
        cols |= set(e.reads) | set(e.group_by)
    return cols
