"""The side-kernel inventory (tests/side_kernel_inventory.py) against the side passes' sources, on the CPU: every kernel name their executors
can report has an entry that tests/test_gpu_side_scale.py runs against the models, MODE and CASE WHEN have rows of their own on every tier
they reach, every entry keeps the small size and runs at a size beyond the wrap point of its tier — the docs one grid step covers on 256
compute units, derived from the sources' own constants — and the time columns of FIRSTWITHTIME / LASTWITHTIME sit on the sides of the
packed bound the entries name."""
import collections
import re

import numpy as np

from tests import histogram_model as hm
from tests import kernel_inventory as ki
from tests import side_kernel_inventory as si
from tests import with_time_model as wm


def test_every_side_kernel_name_has_an_entry():
    in_source = si.kernel_names_in_sources()
    assert sum(len(v) for v in in_source.values()) == 22 and not set.intersection(*in_source.values())
    listed = collections.defaultdict(set)
    for e in si.ENTRIES:
        assert e.family in si.FAMILIES, e
        listed[e.host_family].add(e.name)
    for family, names in in_source.items():
        assert sorted(names - listed[family]) == [], f"{family}: kernel names without an inventory entry"
        assert sorted(listed[family] - names) == [], f"{family}: inventory names its source does not hold"
    for name in set.union(*in_source.values()):
        assert len(name) <= ki.KERNEL_FIELD_BYTES - 1, name


def test_mode_and_case_when_have_rows_on_every_tier_they_reach():
    mode = {e.name for e in si.ENTRIES if e.family == "mode"}
    assert mode == {"pg_pctl_sort", "pg_pctl_lds", "pg_pctl_hbm"}
    case = {e.name for e in si.ENTRIES if e.family == "case"}
    assert case == {"pg_expr_reg", "pg_expr_lds", "pg_expr_hbm"}
    for e in si.ENTRIES:
        assert ("MODE(" in e.select) == (e.family == "mode") and ("CASE WHEN" in e.select) == (e.family == "case"), e


def test_the_kernels_cover_what_the_grid_counts():
    """side_pass_grid and the percentile grid count a workgroup for as many words as its wavefronts take per iteration"""
    c = si.launch_constants()
    assert c["lds_threads"] // 64 * c["words_per_wave"] == c["grid_lds_words"]
    assert c["hbm_threads"] // 64 * c["words_per_wave"] == c["grid_words"] == c["reg_threads"] // 64 * c["words_per_wave"]
    assert c["pctl_lds_threads"] // 64 * c["pctl_words_per_wave"] == c["pctl_grid_lds_words"]
    assert c["pctl_hbm_threads"] // 64 * c["pctl_words_per_wave"] == c["pctl_grid_hbm_words"]


def test_wrap_points_of_256_compute_units():
    c = si.launch_constants()
    by = collections.defaultdict(set)
    for e in si.ENTRIES:
        by[(e.host_family, e.tier, si.lds_wgs_per_cu(e, c) if e.tier == "lds" else 0)].add(si.wrap_point(e, si.ASSUMED_CUS, c))
    assert all(len(v) == 1 for v in by.values())
    points = {k: v.pop() for k, v in by.items()}
    for family in ("expression", "variance", "covariance", "moment", "with_time"):
        assert points[(family, "reg", 0)] == points[(family, "hbm", 0)] == 256 * 8 * 16 * 64 == 2_097_152
        assert points[(family, "lds", 1)] == 256 * 32 * 64 == 524_288
    for family in ("covariance", "with_time", "histogram"):   # tables small enough for four workgroups per CU
        assert points[(family, "lds", 4)] == 2_097_152
    assert points[("histogram", "reg", 0)] == 256 * 2 * 64 * 64 == 2_097_152 == points[("histogram", "hbm", 0)]   # pg_hist_one: 16 wavefronts, two per CU
    assert points[("percentile", "lds", 1)] == 256 * 64 * 64 == 1_048_576 and points[("percentile", "hbm", 0)] == 2_097_152
    assert points[("percentile", "sort", 0)] == 0             # one workgroup per tile: no cap, no stride


def test_every_entry_runs_beyond_the_wrap_point_of_its_tier():
    c = si.launch_constants()
    assert si.SMALL == 2_047 and all(n % 2048 for n in ki.LADDER)
    for e in si.ENTRIES:
        assert set(e.sizes) <= set(ki.LADDER) and si.SMALL in e.sizes, e
        assert e.tier in ("reg", "lds", "hbm", "sort") and e.name.endswith({"reg": ("_reg", "_reg_wide", "_one"), "lds": ("_lds",), "hbm": ("_hbm",), "sort": ("_sort",)}[e.tier]), e
        wrap = si.wrap_point(e, si.ASSUMED_CUS, c)
        assert max(e.sizes) > max(wrap, ki.LARGE - 1), (e.name, e.select, wrap)
        # a second step that is more than a remnant: at least one full round of words for a workgroup beyond the wrap
        assert max(e.sizes) - wrap >= 64 * 64, (e.name, wrap)
        assert all(k.startswith("PG_") for k in e.knobs), e
        assert set(e.group_by) | set(e.reads) <= set(si.columns_at(max(e.sizes))), e
        for col in e.reads:
            assert re.search(r"\b%s\b" % col, e.select), (e.name, col)
    # where a HISTOGRAM table leaves room for four workgroups per CU the wrap point is that of the other tiers: those entries run at the largest size
    small_hist = [e for e in si.ENTRIES if e.family == "histogram" and e.tier == "lds" and si.lds_wgs_per_cu(e, c) == 4]
    assert small_hist and all(si.wrap_point(e, 256, c) == 2_097_152 and ki.LADDER[-1] in e.sizes for e in small_hist)


def test_lds_tables_fit_their_budget_and_the_next_key_space_does_not():
    assert si.LDS_SLOTS == 16384
    for name in ("PG_EXPR_LDS_SLOTS", "PG_VAR_LDS_SLOTS", "PG_COVAR_LDS_SLOTS", "PG_HIST_LDS_SLOTS"):
        assert re.search(r"#define %s %d\b" % (name, si.LDS_SLOTS), si._source("pg_device.h")), name
    assert si._KM["PG_MOMENT_LDS_SLOTS"] == wm.header_constants()["PG_WT_LDS_SLOTS"] == hm.header_constants()["PG_HIST_LDS_SLOTS"] == si.LDS_SLOTS
    assert re.search(r"#define PG_PCTL_LDS_KEYS %d\b" % si.PCTL_LDS_KEYS, si._source("pg_device.h"))
    assert re.search(r"#define PG_EXPR_SUM_LIMBS %d\b" % si.EXPR_SUM_ROW, si._source("pg_device.h"))
    assert (si.K11, si.K32, si.K64, si.K4, si.K1, si.KP) == (1489, 512, 256, 4096, 16384, 327)
    for e in si.ENTRIES:
        if e.tier == "lds":
            budget = si.PCTL_LDS_KEYS if e.host_family == "percentile" else si.LDS_SLOTS
            assert 0 < e.table_slots <= budget, e
    # the largest key space that fits, per family, and one group more in the HBM tier
    fit = {(e.host_family, e.group_by[0]) for e in si.ENTRIES if e.tier == "lds" and e.group_by and e.group_by[0] != "g7" and e.group_by[0] != "rk"}
    over = {(e.host_family, e.group_by[0]) for e in si.ENTRIES if e.tier == "hbm" and e.group_by and e.group_by[0] != "kw"}
    for family in si.EXEC_SOURCES:
        fits = [int(k[1:]) for f, k in fit if f == family]
        overs = [int(k[1:]) for f, k in over if f == family]
        assert fits and any(k + 1 in overs for k in fits), (family, fits, overs)
        assert any(e.host_family == family and e.group_by == ("kw",) and e.tier == "hbm" for e in si.ENTRIES), family   # the wide key space
        assert any(e.host_family == family and not e.group_by for e in si.ENTRIES), family


def test_small_names_are_the_lds_tier_of_key_spaces_the_small_segment_cannot_fill():
    """a key column holds min(key space, docs) groups: at 2 047 docs some HBM entries' tables fit LDS, and they say so"""
    row = {"variance": si.VAR_INT_ROW, "expression": si.EXPR_SUM_ROW, "with_time": 1}   # the rows of the entries concerned: one INT column, one SUM, one slot
    for e in si.ENTRIES:
        if not e.small_name:
            assert e.kernel_at(si.SMALL) == e.name
            continue
        assert e.tier == "hbm" and e.small_name == e.name.replace("_hbm", "_lds") and e.kernel_at(ki.LADDER[-1]) == e.name, e
        if e.host_family == "percentile":   # 7 groups x the values of v16: 60 000 of them, at most one per doc
            assert e.group_by == ("g7",) and e.reads == ("v16",) and 7 * si.SMALL <= si.PCTL_LDS_KEYS < 7 * 60_000
            continue
        space = si.WIDE_KEYS if e.group_by == ("kw",) else int(e.group_by[0][1:])
        assert space > si.SMALL and min(space, si.SMALL) * row[e.host_family] <= si.LDS_SLOTS < space * row[e.host_family], e
    # ... and every other HBM entry's table is beyond LDS at 2 047 docs too: its key space is below 2 047 groups, or its row is long enough
    for e in si.ENTRIES:
        if e.tier == "hbm" and not e.small_name and e.group_by and e.group_by != ("kw",):
            assert int(e.group_by[0][1:]) <= si.SMALL, e


def test_entries_have_distinct_queries():
    # plans are cached per segment by query shape: two entries with one query would share the plan of whichever ran first
    sqls = [(e.sql(), e.snapshot) for e in si.ENTRIES]
    assert len(sqls) == len(set(sqls)), [s for s, n in collections.Counter(sqls).items() if n > 1]


def test_snapshot_entries():
    for family in si.SNAPSHOT_FAMILIES:
        rows = [e for e in si.ENTRIES if e.family == family and e.snapshot]
        assert rows and all(si.SMALL in e.sizes and max(e.sizes) >= ki.LARGE for e in rows), family


def test_time_columns_sit_on_their_sides_of_the_packed_bound():
    big, mid = wm.doc_bits(ki.LADDER[-1]), wm.doc_bits(20_011)
    rng = {t: hi - lo for t, (lo, hi) in si.TIME_RANGE.items()}
    assert wm.packed_ok(rng["tp"], big)                                      # one pass at every size
    assert not wm.packed_ok(rng["tw"], wm.doc_bits(2))                       # two passes at every size
    assert wm.packed_ok(rng["tm"], mid) and not wm.packed_ok(rng["tm"], big)   # the bound moves with the doc count
    assert (mid, big) == (15, 22)
    used = collections.Counter(t for e in si.ENTRIES if e.family == "with_time" and ki.LADDER[-1] in e.sizes for t in si.TIME_RANGE if t in e.reads)
    assert all(used[t] >= 1 for t in si.TIME_RANGE), used
    # the columns hold exactly these ranges, and the tied docs stand where the tie-break crosses workgroups
    n = si.SMALL
    host, data, schema = si.scale_data(n, ["tp", "tw", "tm", "g7"])
    for t, (lo, hi) in si.TIME_RANGE.items():
        assert (int(data[t].min()), int(data[t].max())) == (lo, hi), t
    last, first = si.planted_docs(ki.LADDER[-1], 2_097_152)
    for docs in (last, first):
        assert docs[0] < 64 and docs[1] // 64 > 2_097_152 // 64 and docs[2] // 64 == (ki.LADDER[-1] - 1) // 64
    assert len(set(np.asarray(data["g7"])[list(si.planted_docs(n, 2_097_152)[0])])) == 1
