"""The derive-pass inventory (tests/derive_pass_inventory.py) against the sources of pg_expr_pred, pg_expr_keys and pg_time_keys, on the CPU:
the three launch sites and the three kernels agree on what a grid step covers, every pass has entries at 2 047 docs and beyond the wrap
point of 256 compute units, the large size sees every predicate kind, every operand kind of expr_load, every branch of time_load and both
trips and the remainder of the operand loop, and the segment holds what the entries rely on."""
import numpy as np

from tests import derive_pass_inventory as di
from tests import kernel_inventory as ki
from tests import side_kernel_inventory as si
from tests import time_transform_model as tm

WRAP = 2_097_152


def test_launch_sites_and_kernels_agree():
    c = di.launch_constants()
    assert c["words_per_wave"] == 4
    assert len({c[p + ".cap"] for p in di.PASSES}) == 1 and len({c[p + ".per_wg"] for p in di.PASSES}) == 1
    for p in di.PASSES:
        assert c[p + ".bounds"] == c[p + ".threads"] == 256, p
        assert c[p + ".threads"] // 64 * c["words_per_wave"] == c[p + ".per_wg"], p     # the grid counts a workgroup for what its wavefronts take
    # ... and the side passes' register tier wraps at the same point: one ladder size serves both inventories
    s = si.launch_constants()
    assert c["pg_expr_pred.cap"] == s["wgs_per_cu"] and c["pg_expr_pred.per_wg"] == s["grid_words"]


def test_wrap_point_of_256_compute_units():
    c = di.launch_constants()
    for p in di.PASSES:
        assert di.wrap_point(256, c, p) == 256 * 8 * 16 * 64 == WRAP
    assert di.wrap_point(304, c) == 304 * 8 * 16 * 64 and di.wrap_point(1, c) == 8192


def test_every_pass_runs_small_and_beyond_the_wrap():
    assert (di.SMALL, di.BIG) == (2_047, 2_500_003) and all(n % 2048 for n in ki.LADDER)
    assert di.BIG - WRAP >= 64 * 64 and di.BIG % 64 != 0 and di.BIG % di.BAND_DOCS != 0
    assert WRAP % di.BAND_DOCS == 0 and WRAP // di.BAND_DOCS < (di.BIG - 1) // di.BAND_DOCS      # the band that begins at the wrap is not the last
    assert di.DENSE_BACK % 4 == 0 and di.DENSE_BACK // 64 >= 20                                  # srt = doc / 4; twenty full words on either side
    for p in di.PASSES:
        assert di.entries_of(p, di.SMALL) and di.entries_of(p, di.BIG), p
    for e in di.ENTRIES:
        assert e.kernel in di.PASSES and set(e.sizes) <= set(ki.LADDER) and di.SMALL in e.sizes and max(e.sizes) == di.BIG, e
        assert e.shapes and set(e.shapes) <= set(di.PRED_SHAPES if e.kernel == "pg_expr_pred" else di.KEY_SHAPES), e
        assert not e.twin or e.shapes == ("all",), e
    # plans are cached per query shape, derived columns per canonical text: every (pass, text) once
    assert len({(e.kernel, e.expression()) for e in di.ENTRIES if e.kernel != "pg_expr_pred"}) == len([e for e in di.ENTRIES if e.kernel != "pg_expr_pred"])
    assert len({e.text for e in di.ENTRIES}) == len(di.ENTRIES)


def test_predicates_of_the_large_size():
    big = di.entries_of("pg_expr_pred", di.BIG)
    assert {e.predicate_kind() for e in big} == {"RANGE", "EQ", "NOT_EQ", "IN", "NOT_IN"}      # PG_XP_RANGE, EQ, NOT_EQ, IN, NOT_IN
    shapes = [s for e in big for s in e.shapes]
    assert all(shapes.count(s) == 1 for s in ("and", "or", "not", "snapshot", "filter")) and shapes.count("lone") == len(big)


def test_operand_kinds_and_counts_of_the_large_size():
    for p in ("pg_expr_pred", "pg_expr_keys"):
        big = di.entries_of(p, di.BIG)
        assert {di.column_kind(c) for e in big for c in e.sources()} == di.OPERAND_KINDS, p
        counts = {len(e.sources()) for e in big}
        # the operand loop is `#pragma unroll 2`: one column is the remainder alone, an odd count >= 3 a trip and the remainder, 8 four trips
        assert 1 in counts and 8 in counts and any(k >= 3 and k % 2 for k in counts), (p, counts)
        assert max(counts) == 8
    # the eight columns are distinct: PG_EXPR_MAX_SRCS of them
    assert len(set(di.EIGHT.split(","))) == 8


def test_time_load_kinds_of_the_large_size():
    big = di.entries_of("pg_time_keys", di.BIG)
    assert {di.column_kind(e.sources()[0]) for e in big if "all" in e.shapes} == di.TIME_KINDS
    families = {tm.arguments(e.expression())[0] for e in big}
    assert {"toepochdays", "toepochminutesrounded", "timeconvert", "datetrunc"} <= families
    assert any(e.sources() == ["uid"] and set(e.shapes) == {"sparse", "dense"} and e.groups_limit > di.BIG for e in big)


def _check_planted(n):
    data, schema = di.scale_columns(n, WRAP)
    idx = np.arange(n)
    assert np.array_equal(data["pos"], idx) and np.array_equal(data["band"], idx // 65536) and np.array_equal(data["srt"], idx // 4)
    assert {c: schema[c] for c in di.SCHEMA} == di.SCHEMA and set(di.RAW) <= set(data)
    # the key spaces of the high-cardinality keys, every value planted
    assert len(np.unique(data["hk"])) == min(n, di.HK_CARD) and len(np.unique(data["hk2"])) == min(n, di.HK2_CARD)
    if n == di.BIG:
        assert (len(np.unique(data["hk"])) - 1).bit_length() == 17 and (len(np.unique(data["hk2"])) - 1).bit_length() == 22
        assert (n - 1).bit_length() == 22                                        # toepochdays(uid): one key per doc
        for e in di.entries_of("pg_expr_keys", n):
            if e.groups_limit:
                v = di.evaluate(e.expression(), data, schema)
                assert len(np.unique(v)) == len(np.unique(data[e.sources()[0]])) < e.groups_limit   # the expression keeps the keys apart
            else:
                assert 10 <= len(np.unique(di.evaluate(e.expression(), data, schema))) <= 50_000, e     # below the default numGroupsLimit
    assert len(np.unique(di.time_keys("toepochdays(uid)", data))) == n
    # the pools of the time sources
    for col, planted in (("ts", di.PLANTED_MS), ("tsd", di.PLANTED_MS), ("sec", di.PLANTED_S), ("secd", di.PLANTED_S)):
        values = np.unique(data[col])
        assert len(values) <= di.POOL_MAX and set(planted) <= set(values.tolist()), col
    assert 0 in di.PLANTED_MS and -1 in di.PLANTED_MS and 0 in di.PLANTED_S and -1 in di.PLANTED_S
    for boundary, text in ((4 * tm.DAY_MS, "datetrunc('week',ts)"), (978_307_200_000, "datetrunc('year',ts)"), (999_302_400_000, "datetrunc('month',ts)")):
        assert boundary in di.PLANTED_MS and boundary - 1 in di.PLANTED_MS
        assert tm.evaluate(text, [boundary])[0] == boundary and tm.evaluate(text, [boundary - 1])[0] < boundary - tm.DAY_MS
    # every predicate selects between 5 % and 95 % of the docs, in every shape
    for e in di.entries_of("pg_expr_pred", n):
        leaf = di.where_mask(e.text, data, schema)
        assert di.SELECTIVITY[0] <= leaf.mean() <= di.SELECTIVITY[1], (e.text, leaf.mean())
        for shape in e.shapes:
            keep = ki.snapshot_doc_ids(n) if shape == "snapshot" else None
            mask = di.where_mask(e.where(shape, n, WRAP), data, schema, keep)
            assert 0.05 <= mask.mean() <= 0.95, (e.text, shape, mask.mean())
            if n > WRAP:
                band = idx // di.BAND_DOCS
                assert mask[band == WRAP // di.BAND_DOCS].any() and mask[band == band[-1]].any(), (e.text, shape)
    # the two filters of the key passes
    sparse = di.where_mask(si.SPARSE, data, schema)
    assert sparse[:64].any() and sparse[n - n % 64:].any() and sparse.mean() < 0.025
    if n > WRAP:
        assert sparse[WRAP - 1] and sparse[WRAP]
        dense = np.flatnonzero(di.where_mask(si.dense_filter(n, WRAP - di.DENSE_BACK), data, schema))
        first = dense[dense < n - 4000]
        assert (first[0], first[-1]) == (WRAP - di.DENSE_BACK, WRAP + 3000 - di.DENSE_BACK - 1) and len(first) == 3000
        assert dense[-1] == n - 1 and len(dense) - len(first) == n - (n - 3000) // 4 * 4


def test_planted_properties_of_the_small_segment():
    _check_planted(di.SMALL)


def test_planted_properties_of_the_large_segment():
    _check_planted(di.BIG)


def test_twins_hold_the_models_values():
    host, data, schema, twins = di.scale_data(di.SMALL)
    assert set(twins) == {e.expression() for e in di.ENTRIES} and len(twins) == len(di.ENTRIES) - 1      # IN and NOT_IN share di - c_inv1
    for e in di.ENTRIES:
        twin = data[twins[e.expression()]]
        if e.kernel == "pg_time_keys":
            assert schema[twins[e.expression()]] == "LONG" and twin.tolist() == tm.evaluate(e.expression(), data[e.sources()[0]])
        else:
            assert schema[twins[e.expression()]] == "DOUBLE" and di.same_doubles(twin, di.evaluate(e.expression(), data, schema))
    # the rounded sum: multiples of 1 024 above 2^62, of 512 below
    v = data[twins[di.ENTRIES[9].expression()]]
    assert di.ENTRIES[9].text == di.ROUNDED_SUM and ((v - 2.0**62) % 512 == 0).all() and (v < 2.0**62).any() and (v > 2.0**62).any() and 100 < len(np.unique(v)) < 5000


def test_the_folds_against_a_plain_loop():
    """fold_bands and fold_keys — the references of the large sizes — against dictionaries filled doc by doc"""
    data, schema = di.scale_columns(200_003, WRAP)
    mask = di.where_mask("di + 2 = 5", data, schema)
    want = {}
    for doc in np.flatnonzero(mask).tolist():
        r = want.setdefault((doc // 65536,), [0, 0, doc, doc])
        r[0] += 1
        r[1] += doc
        r[3] = doc
    assert di.fold_bands(mask, data) == {k: [r[0], float(r[1]), float(r[2]), float(r[3])] for k, r in want.items()}
    keys = di.double_bits(di.evaluate("divide(ri,'1000')", data, schema))
    u, counts, sums = di.fold_keys(keys, data["pos"])
    want = {}
    for doc, k in enumerate(keys.tolist()):
        r = want.setdefault(k, [0, 0])
        r[0] += 1
        r[1] += doc
    assert u.tolist() == sorted(want) and counts.tolist() == [want[k][0] for k in u.tolist()] and sums.tolist() == [want[k][1] for k in u.tolist()]
