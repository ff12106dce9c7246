"""SELECT DISTINCT at 2 x 10^8 docs: config 3's filter with DISTINCT g1, g2 ORDER BY g1, g2 LIMIT 10000 against the oracle's GROUP BY of
the same filter (an unbounded key set, sorted by the same keys), and the LIMIT-without-ORDER-BY form against the oracle's numGroupsLimit
admission (groups in docId order until the limit: po_query.c:425-480)."""
import pytest

from pinot_amd import synth
from pinot_amd.executor import NativeSegment
from pinot_amd.query import parse_sql

pytestmark = pytest.mark.gpu
DOCS = 200_000_000
WHERE = "WHERE c_inv1 IN (0,1,2,3) AND c_inv2 IN (0,1) AND r_int BETWEEN 250000 AND 749999"


def test_config3_filter_distinct_at_scale(gpu_api, oracle_api):
    host = synth.generate_segment(DOCS, segment_index=0, columns=synth.CFG3_COLUMNS)
    g, o = NativeSegment(gpu_api, host), NativeSegment(oracle_api, host)
    try:
        rb = g.execute(f"SELECT DISTINCT g1, g2 FROM gpuBench {WHERE} ORDER BY g1, g2 LIMIT 10000")
        qg = parse_sql(f"SELECT g1, g2, COUNT(*) FROM gpuBench {WHERE} GROUP BY g1, g2")
        qg.num_groups_limit = 2_000_000_000
        og = o.execute(qg)
        want = sorted(og.group_keys)[:10000]
        assert rb.distinct_rows == want
        matched = sum(c[0] for c in og.rows().values())
        assert rb.stats.num_docs_scanned == og.stats.num_docs_scanned == matched
        assert rb.stats.num_entries_scanned_post_filter == 2 * matched
        assert rb.stats.num_entries_scanned_in_filter == og.stats.num_entries_scanned_in_filter
        # LIMIT without ORDER BY: the first 100 tuples in docId order = the oracle's first 100 admitted groups
        rl = g.execute(f"SELECT DISTINCT g1, g2 FROM gpuBench {WHERE} LIMIT 100")
        ql = parse_sql(f"SELECT g1, g2, COUNT(*) FROM gpuBench {WHERE} GROUP BY g1, g2")
        ql.num_groups_limit = 100
        assert set(rl.distinct_rows) == set(o.execute(ql).group_keys)
        assert rl.stats.num_docs_scanned < matched
    finally:
        g.destroy()
        o.destroy()
