"""The kernel inventory (tests/kernel_inventory.py) against the dispatcher's source, on the CPU: every name pg_exec.hip can report has an entry
that tests/test_gpu_kernel_matrix.py runs against the oracle (or an exemption that says why no query reaches it), no name is truncated by
pg_exec_stats.kernel, and every entry runs at two or more sizes of the ladder, one of them a large segment."""
import collections

from tests import kernel_inventory as ki


def test_every_kernel_name_has_an_inventory_entry():
    in_source = ki.kernel_names_in_source()
    listed = [e.name for e in ki.ENTRIES]
    assert len(listed) == len(set(listed)), [n for n, c in collections.Counter(listed).items() if c > 1]
    assert not set(listed) & set(ki.EXEMPT), "a kernel is both run and exempted"
    assert sorted(in_source - set(listed) - set(ki.EXEMPT)) == [], "kernel names without an inventory entry"
    assert sorted((set(listed) | set(ki.EXEMPT)) - in_source) == [], "inventory names pg_exec.hip does not hold"


def test_exemptions_cite_the_condition_that_rules_the_kernel_out():
    for name, reason in ki.EXEMPT.items():
        assert ("pg_plan.cpp" in reason or "pg_exec.hip" in reason) and len(reason) > 80, name


def test_kernel_names_fit_the_stats_field():
    for name in ki.kernel_names_in_source():
        assert len(name) <= ki.KERNEL_FIELD_BYTES - 1, name


def test_entries_run_on_the_ladder():
    assert all(n % 2048 for n in ki.LADDER)
    for e in ki.ENTRIES:
        assert set(e.sizes) <= set(ki.LADDER), e.name
        assert len(set(e.sizes)) >= 2, e.name
        assert max(e.sizes) >= ki.LARGE, e.name
        assert e.builder in ki.BUILDERS, e.name
        assert e.entry in ("execute", "filter", "distinct", "selection"), e.name
        assert all(k.startswith("PG_") for k in e.knobs), e.name


def test_entries_have_distinct_queries():
    # plans are cached per segment by query shape, and plan-time knobs act only when a plan is compiled: two entries with one query would share
    # the plan of whichever ran first
    sqls = [e.sql for e in ki.ENTRIES]
    assert len(sqls) == len(set(sqls)), [s for s, c in collections.Counter(sqls).items() if c > 1]


def test_snapshot_drops_the_tail_docs():
    for n in ki.LADDER:
        ids = ki.snapshot_doc_ids(n)
        kept = set(ids.tolist())
        assert n - 1 not in kept and ids.max() < n
        for w in (32, 64):
            start = n - n % w
            assert any(d not in kept for d in range(start, n - 1)) or start == n - 1, (n, w)
