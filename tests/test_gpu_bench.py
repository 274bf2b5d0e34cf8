"""bench.py on one GPU, every BASELINE config at development scale: with --full one JSON line, the contract's fields, and the parity
of the timed results against the oracle (`parity_checked.ok`; a mismatch makes bench.py exit non-zero); a plain run's lean line and
its --dump-outputs."""
import json
import os
import subprocess
import sys

import pytest

from tests.util import ROOT

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("extra", [
    ["--config", "2", "--length", "4000000"],
    ["--config", "3", "--scale", "0.002"],
    ["--config", "4", "--scale", "0.002"],
    ["--config", "5", "--scale", "0.01", "--coverage", "60"],
])
def test_bench_line(tmp_path, extra):
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "2", "--warmup", "1", "--cpu-sample-reads", "20000", "--parity-windows", "4", "--e2e-pause", "0.3"] + extra
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, cwd=ROOT, timeout=900)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
              "data", "config", "roofline", "cpu_baseline", "parity_checked"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["value"] > 0 and d["roofline"]["bound"] == "hbm" and 0 < d["roofline"]["frac"] < 1
    # the accounting checks itself: every kernel's algorithmic bytes / time stays below the HBM peak (bench.py exits non-zero otherwise)
    assert "accounting_error" not in d
    for k, e in d["kernels"].items():
        assert 0 < e["frac_of_hbm_peak"] <= 1, (k, e)
    assert d["parity_checked"]["ok"] and d["parity_checked"]["windows"] >= 1
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["kind"] == "port"
    assert d["e2e"]["Mreads_per_s"] > 0
    # round 5: the whole share is checked, not samples -- every row of text (configs 2, 5), every window / BED region of a contig (3, 4)
    cfg = int(extra[1])
    if cfg in (2, 5):
        assert d["parity_checked"]["coverage"] == 1.0 and d["parity_checked"]["full_text"]["ok"]
        assert d["parity_checked"]["full_text"]["slices"] >= 64
    else:
        assert d["parity_checked"]["whole_contig"]["ok"] and d["parity_checked"]["whole_contig"]["regions"] >= 1
    # the token streams are an intermediate, not algorithmic bytes; the fused-path figure is a first-class field
    assert d["kernels"]["huffman_decode"]["intermediate_bytes"] > 0
    assert d["kernels"]["huffman_decode"]["algorithmic_bytes"] < d["kernels"]["lz77_resolve"]["algorithmic_bytes"]
    assert 0 < d["roofline"]["path_frac"] < 1
    # round 6: the older definition beside the redefined one; the pass including its text (configs 2, 5); config 4 timed with the work-list
    # cache off, the cached re-run beside it
    assert d["roofline"]["path_frac_incl_counters"] >= d["roofline"]["path_frac"] and "traffic_total" in d["roofline"]
    if cfg in (2, 5):
        dt = d["device_text"]
        assert "error" not in dt, dt
        assert dt["text_equals_host_copy_path"] and dt["text_bytes"] > 100000 and dt["ms_per_step"] >= d["ms_per_step"] * 0.8
    if cfg == 4:
        assert d["rerun_cached"]["ms_per_step"] > 0
    # counters are joined only from a pass stamped with these very kernel sources: a development-scale line has none
    assert d["roofline"]["traffic"] is None


def test_two_ranks_report_what_the_collective_layer_saw(tmp_path):
    """bench.py --gpus 2 (two ranks sharing the test box's GPU over gloo): the line carries `collective` -- backend, world size,
    an all-reduce of ones, per-rank device identity and kernel times -- so that a scaling record can be audited."""
    env = dict(os.environ, PYTHONPATH=ROOT, SBX_BENCH_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29611",
           os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--steps", "2", "--warmup", "1", "--length", "3000000", "--no-cpu-baseline", "--no-e2e",
           "--no-side-runs", "--parity-windows", "2"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, cwd=ROOT, timeout=900)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    d = json.loads([ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")][0])
    c = d["collective"]
    assert c["world_size"] == 2 and c["allreduce_of_ones"] == 2.0 and c["backend"] == "gloo" and len(c["ranks"]) == 2
    assert sorted(e["rank"] for e in c["ranks"]) == [0, 1] and all(e["kernel_ms"]["lz77_resolve"] > 0 for e in c["ranks"])
    assert d["n_gpus"] == 2 and d["parity_checked"]["ok_all_ranks"]


@pytest.mark.parametrize("extra", [
    ["--config", "2", "--length", "4000000"],
    ["--config", "3", "--scale", "0.002"],
    ["--config", "4", "--scale", "0.002"],
])
def test_plain_run_dumps_the_same_outputs_twice(tmp_path, extra):
    """A plain run (no --full) prints the headline fields and none of the side measurements or checks; --dump-outputs writes
    float arrays of at most 64 MB, the same on two runs with the same arguments, and `depth base` counters equal the oracle's."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    from tests.util import oracle_base_counters
    env = dict(os.environ, PYTHONPATH=ROOT)
    dumps = []
    for k in range(2):
        out = tmp_path / ("out%d" % k)
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--dump-outputs", str(out)] + extra
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, cwd=ROOT, timeout=600)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")]
        assert len(lines) == 1
        d = json.loads(lines[0])
        assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0 and d["full"] is False
        assert d["unit"] == "Mreads/s" and d["higher_is_better"] is True and d["dtype"] == "u8/u32" and d["metric"].startswith("depth_")
        for key in ("cpu_baseline", "parity_checked", "e2e", "device_text", "rerun_cached", "collective"):
            assert d[key] is None, key
        files = sorted(out.iterdir())
        assert sum(f.stat().st_size for f in files) <= 64 * 10**6
        arrays = {f.name[:-4]: np.load(f) for f in files if f.name.endswith(".npy")}
        assert len(arrays) == len(files) and sorted(arrays) == sorted(d["dumped_outputs"])
        assert all(a.dtype in (np.float32, np.float64) and a.size > 0 for a in arrays.values())
        assert arrays["run_counts"][:, 0].sum() == d["reads_total"]
        dumps.append(arrays)
    assert sorted(dumps[0]) == sorted(dumps[1])
    for name in dumps[0]:
        assert np.array_equal(dumps[0][name], dumps[1][name]), name
    a = dumps[0]
    if extra[1] == "2":
        args = bench.parser().parse_args(extra)
        contigs, coverage, seed, gen_extra, _ = bench.workload(args)
        bam = bench.bam_path(contigs, coverage, seed, args.level, args.codec, gen_extra)
        assert np.array_equal(a["base_positions"][:4096], np.stack([np.zeros(4096), np.arange(4096)], axis=1))
        assert np.array_equal(a["base_counters"][:4096], oracle_base_counters(bam, 0, 0, 4096, n_samples=1).astype(np.float64))
    else:
        kind = "window" if extra[1] == "3" else "region"
        n = len(a[kind + "_bounds"])
        assert n > 0 and a[kind + "_reads"].shape[0] == n and a[kind + "_bases"].shape[0] == n
