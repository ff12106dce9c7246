"""The JNI wire format of PERCENTILE through the shim's C half: tests/shim_percentile_records.c against integration/jni/pinot_gpu_shim.c."""
import os
import subprocess

import pytest

from pinot_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_percentile_records_through_the_shim(tmp_path):
    if not os.path.exists(capi.GPU_LIB_PATH):
        pytest.skip("libpinot_gpu.so not built here")
    csrc = os.path.join(ROOT, "pinot_amd", "csrc")
    exe = str(tmp_path / "shim_percentile_records")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "integration", "jni"), os.path.join(ROOT, "tests", "shim_percentile_records.c"),
                           os.path.join(ROOT, "integration", "jni", "pinot_gpu_shim.c"), "-L" + csrc, "-lpinot_gpu", "-Wl,-rpath," + csrc, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    for line in ("two percentiles round-trip into agg_params", "a truncated double fails cleanly", "a record without a percentile is unchanged", "wire format ok"):
        assert line in out.stdout


def test_abi_version_and_the_new_export():
    header = open(os.path.join(ROOT, "include", "pinot_gpu.h")).read()
    assert "#define PG_ABI_VERSION 5" in header and capi.PG_ABI_VERSION == 5
    assert "PG_AGG_PERCENTILE = 16" in header and capi.AGG_FUNCTIONS["PERCENTILE"] == 16
    assert "PG_RESULT_VALUE_COUNTS = 7" in header and capi.RESULT_VALUE_COUNTS == 7
    assert "#define PG_QUERY_FLAG_FINAL_PERCENTILE 0x200" in header and capi.QUERY_FLAG_FINAL_PERCENTILE == 0x200
    assert "result_set_counts" in capi.GPU_ONLY_SYMBOLS
    assert capi.PgQuery._fields_[-1][0] == "agg_params"   # at the end: callers that zero the struct are unaffected


def test_percentile_kernels_use_no_scratch():
    """the build leaves hipcc's kernel-resource-usage remarks of pg_kernels_percentile.hip behind: no kernel of the path may spill"""
    import re
    log = os.path.join(ROOT, "pinot_amd", "csrc", "pg_kernels_percentile.resources.log")
    if not os.path.exists(log):
        pytest.skip("library was built without the resource log")
    usage, cur = {}, None
    for line in open(log):
        m = re.search(r"Function Name: (\w+)", line)
        if m:
            cur = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and cur:
            usage[cur] = int(m.group(1))
    for k in ("pg_pctl_lds", "pg_pctl_hbm", "pg_pctl_sort", "pg_pctl_select", "pg_pctl_runs", "pg_pctl_sort_select", "pg_pctl_sort_runs", "pg_pctl_tile_counts"):
        assert usage.get(k) == 0, (k, usage.get(k))
