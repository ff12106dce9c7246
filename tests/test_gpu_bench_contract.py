"""bench.py's contract on a small segment: the one JSON line with `roofline` of a plain run, the same line with `cpu_baseline` and every
other block of a `--full` run, and the same script started by `python -m torch.distributed.run` the way the driver starts the multi-GPU
runs (one rank here: the box has one GPU)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REQUIRED = ["metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
            "data", "config", "roofline", "cpu_baseline"]
# what only a --full run measures or checks: runs of their own after the timed steps
FULL_ONLY = ["cpu_baseline", "north_star_variant", "merge_world_of_one", "concurrency", "cfg2", "cfg2_dict", "cfg3_dict", "cfg3_sparse_dictionaries",
             "cfg5_flat", "cfg5_star_tree", "star_tree_route", "multi_gpu_validation"]


def last_json_line(out):
    lines = [ln for ln in out.stdout.strip().splitlines() if ln.startswith("{")]
    assert lines, out.stdout[-2000:] + out.stderr[-2000:]
    return json.loads(lines[-1])


def test_bench_line_on_a_small_segment(tmp_path, oracle_api):
    dump = str(tmp_path / "outputs")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--docs", "3000000", "--steps", "3", "--warmup", "1", "--full",
                          "--no-traffic", "--cpu-sample-docs", "1000000", "--dump-outputs", dump], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    d = last_json_line(out)
    for k in REQUIRED:
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "rows/s" and d["higher_is_better"] is True
    assert d["value"] > 0 and d["scaling"] == "weak" and d["data"] == "synthetic" and "workload" in d["config"]
    r, c = d["roofline"], d["cpu_baseline"]
    assert r["bound"] == "hbm" and r["peak"] == 8000.0 and r["unit"] == "GB/s" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert c["kind"] == "port" and c["cores"] == 1 and c["gpu_equals_oracle_on_sample"] is True and c["value"] > 0
    # BASELINE configs 2 and 5 ride in every --full run: kernel time, roofline fraction and an oracle equality flag each
    for key in ("cfg2", "cfg2_dict", "cfg5_flat"):
        b = d[key]
        assert b["kernel_ms"] > 0 and 0 < b["roofline_frac"] < 1 and b["rows"] == 3000000
        assert b.get("gpu_equals_oracle_at_full_size", b.get("gpu_equals_oracle_on_sample")) is True
    # 3 M docs are under 16 offers per HLL register (12 800 groups x 256): the partition pipeline; the 10^9-doc run takes the pruned-offer
    # passes (pg_kernels_oct.hip; tests/test_gpu_full_size.py asserts that name)
    assert d["cfg5_flat"]["kernel"] == "pg_part_group_by"
    st = d["cfg5_star_tree"]
    assert st["groups"] == 12800 and st["star_tree_index"] == 0 and st["device_ms"] > 0
    # the library merge with nothing to exchange (communicator of one rank): its latency is on record, its result the unmerged one
    m = d["merge_world_of_one"]
    assert m.get("error") is None and m["p50_ms"] > 0 and m["equals_unmerged_result"] is True
    # --dump-outputs: the timed step's result, array for array the oracle's on the same segment
    import bench
    from pinot_amd import synth
    from pinot_amd.executor import NativeSegment
    seg = NativeSegment(oracle_api, synth.generate_segment(3000000, columns=list(synth.CFG3_COLUMNS)))
    bench.dump_outputs(seg.execute(synth.QUERY_CFG3), str(tmp_path / "oracle"))
    seg.destroy()
    names = sorted(os.listdir(dump))
    assert names == sorted(os.listdir(tmp_path / "oracle")) and "group_keys.npy" in names
    for f in names:
        a, b = np.load(os.path.join(dump, f)), np.load(tmp_path / "oracle" / f)
        assert a.dtype == np.float64 and np.array_equal(a, b), f


def test_plain_run_stops_at_the_headline(tmp_path, oracle_api):
    """Without --full: the same contract fields, the roofline of the timed steps' own kernel times, the same --dump-outputs, and none of the
    blocks that take runs of their own (the --no-* options have nothing left to take away)."""
    dump = str(tmp_path / "outputs")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--docs", "3000000", "--steps", "3", "--warmup", "1",
                          "--dump-outputs", dump], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    d = last_json_line(out)
    assert sorted(k for k in REQUIRED if k not in d) == ["cpu_baseline"] and not set(FULL_ONLY) & set(d), sorted(d)
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "rows/s" and d["higher_is_better"] is True
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["dtype"] == "int64" and d["metric"].startswith("rows scanned/sec")
    assert abs(d["value"] - 3000000 / (d["ms_per_step"] * 1e-3)) <= 1e-9 * d["value"]
    r = d["roofline"]
    assert r["kernel_ms"] > 0 and r["traffic"] is None and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    import bench
    from pinot_amd import synth
    from pinot_amd.executor import NativeSegment
    seg = NativeSegment(oracle_api, synth.generate_segment(3000000, columns=list(synth.CFG3_COLUMNS)))
    bench.dump_outputs(seg.execute(synth.QUERY_CFG3), str(tmp_path / "oracle"))
    seg.destroy()
    names = sorted(os.listdir(dump))
    assert names == sorted(os.listdir(tmp_path / "oracle")) and "group_keys.npy" in names
    for f in names:
        assert np.array_equal(np.load(os.path.join(dump, f)), np.load(tmp_path / "oracle" / f)), f


def test_bench_under_torchrun_with_one_rank():
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
                          "--master-port", "29571", os.path.join(ROOT, "bench.py"), "--gpus", "1", "--docs", "1000000", "--steps", "2",
                          "--warmup", "1", "--full", "--no-traffic", "--no-cpu-baseline"], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    d = last_json_line(out)
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["value"] > 0 and "roofline" in d
