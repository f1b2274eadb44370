"""The bench.py contract the driver relies on: one JSON line on stdout with the agreed keys, for the single-GPU launch
and for the torch.distributed launch (one rank here; RCCL init, chunked solve + asynchronous all-gather path), with
--full (roofline, CPU baseline, end-to-end) and without it (the headline only, --dump-outputs)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
        "dtype", "data", "config", "roofline"}
SMALL = ["--size", "256", "--frames", "10", "--steps", "2", "--warmup", "1", "--no-variants"]   # frames given: same workload at any N


def run(cmd):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines                      # exactly ONE line on stdout
    return json.loads(lines[0])


def check(d, n_gpus):
    assert KEYS <= set(d)
    assert d["metric"] == "frame-pairs/sec" and d["unit"] == "frame-pairs/s" and d["higher_is_better"] is True
    assert d["n_gpus"] == n_gpus and d["steps"] == 2 and d["warmup"] == 1 and d["scaling"] == "weak"
    assert d["dtype"] == "f64" and d["data"] == "synthetic" and d["vs_baseline"] is None
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["config"]["converged"] is True
    assert "model" not in d["config"] and "workload" in d["config"]
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["peak"] == 8000.0 and r["unit"] == "GB/s"
    assert r["achieved"] > 0 and r["frac"] == pytest.approx(r["achieved"] / r["peak"])
    # an HBM fraction: bytes the launch has to move over its time (the per-sweep work rate is reported separately)
    assert r["achieved"] == pytest.approx(r["bytes_per_launch"] / (r["avg_launch_us"] * 1e-6) / 1e9)
    assert r["frac"] < 1 and r["effective_per_sweep"]["rate"] >= r["achieved"] * 0.999


def test_single_gpu_line_with_cpu_baseline():
    d = run([sys.executable, "bench.py", "--full"] + SMALL)
    check(d, 1)
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] == 1 and c["value"] > 0 and c["unit"] == "frame-pairs/s" and c["sample"]
    assert c["host_cores"] >= 1 and c["all_cores"]["cores"] >= 1 and c["all_cores"]["value"] > 0
    e = d["end_to_end"]
    assert e["unit"] == "frame-pairs/s" and 0 < e["value"] and e["converged"] is True
    w = d["roofline"]["whole_solve"]
    assert 0 < w["frac"] < 1 and w["bytes_per_step"] > 0 and w["frac"] == pytest.approx(w["achieved"] / 8000.0)
    assert d["value"] / c["value"] > 10                # sanity only: the ratio says nothing about kernel quality


def test_distributed_launch_line():
    d = run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
             "--master-port", "29517", "bench.py", "--full", "--gpus", "1", "--force-dist", "--no-cpu-baseline", "--gather-chunks", "3"] + SMALL)
    check(d, 1)
    assert d["config"]["allgather"] is True and d["config"]["gather_chunks"] == 3 and d["config"]["chunk_sizes"] == [3, 3, 3]


PLAIN_KEYS = KEYS - {"roofline"}
FULL_ONLY = {"roofline", "variants", "end_to_end", "cpu_baseline"}


def test_plain_line_and_output_dump(tmp_path):
    """Without --full: the headline line only; --dump-outputs writes the last timed step's fields and statistics, the
    same in two runs with the same arguments."""
    args = ["--size", "256", "--frames", "10", "--steps", "2", "--warmup", "1"]
    runs = [run([sys.executable, "bench.py", "--dump-outputs", str(tmp_path / r)] + args) for r in "ab"]
    for d in runs:
        assert PLAIN_KEYS <= set(d) and not FULL_ONLY & set(d)
        assert d["metric"] == "frame-pairs/sec" and d["unit"] == "frame-pairs/s" and d["higher_is_better"] is True
        assert d["dtype"] == "f64" and d["steps"] == 2 and d["warmup"] == 1 and d["config"]["converged"] is True
        assert d["value"] == pytest.approx(9 * 1e3 / d["ms_per_step"])       # 9 pairs per step
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert {"v_x.npy", "v_y.npy", "remodelling.npy", "speed.npy", "iterations.npy", "relative_residual.npy"} <= set(names)
    for f in names:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype == np.float64
        np.testing.assert_array_equal(a, b, err_msg=f)
    vx = np.load(tmp_path / "a" / "v_x.npy")
    assert vx.shape == (9, 256, 256) and np.isfinite(vx).all()
    it = np.load(tmp_path / "a" / "iterations.npy")
    assert it.shape == (9,) and it.mean() == pytest.approx(runs[0]["config"]["iterations_mean"])
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in names) <= 64 * 2 ** 20


def test_plain_dump_samples_a_large_field(tmp_path):
    """A field of more than DUMP_SAMPLE values is dumped as its seeded sample."""
    import bench
    d = run([sys.executable, "bench.py", "--size", "512", "--frames", "6", "--steps", "1", "--warmup", "0",
             "--dump-outputs", str(tmp_path)])
    assert d["steps"] == 1 and d["config"]["converged"] is True
    for k in ("v_x", "v_y", "remodelling", "speed"):
        a = np.load(tmp_path / (k + ".npy"))
        assert a.shape == (bench.DUMP_SAMPLE,) and a.dtype == np.float64 and np.isfinite(a).all()
