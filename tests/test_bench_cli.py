"""bench.py's launcher contract, checked without a GPU: a request for N > 1 GPUs must never end in an N = 1 line.  On the GPU: what
a plain run prints and what --dump-outputs writes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env=None):
    e = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, env=e, timeout=300)


def test_gpus_2_without_two_gpus_fails_loudly():
    import torch
    if torch.cuda.device_count() >= 2:
        return                      # a real multi-GPU node: the spawn path itself is exercised by the driver's scaling run
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0"])
    assert r.returncode != 0
    assert "needs 2 visible GPUs" in r.stderr
    assert '"metric"' not in r.stdout          # no JSON line at all


def test_world_size_must_match_gpus():
    r = _run(["--gpus", "2"], env={"WORLD_SIZE": "4", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "must agree" in r.stderr and '"metric"' not in r.stdout
    r = _run(["--gpus", "0"])
    assert r.returncode != 0


def test_options_for_the_full_run_and_the_outputs():
    r = _run(["--help"])
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout


def test_dump_outputs_writes_float64(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    bench.dump_outputs(str(tmp_path / "out"), {"dx": np.arange(3, dtype=np.float32), "parameters": [1.0, 2.0]})
    dx = np.load(tmp_path / "out" / "dx.npy")
    assert dx.dtype == np.float64 and dx.tolist() == [0.0, 1.0, 2.0]
    assert np.load(tmp_path / "out" / "parameters.npy").tolist() == [1.0, 2.0]


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    """Without --full: the headline line, nothing measured beside it; --dump-outputs: the last timed step's dx and parameters."""
    r = _run(["--gpus", "1", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path)])
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in out
    assert out["steps"] == 2 and out["warmup"] == 1
    assert out["value"] * out["ms_per_step"] == pytest.approx(1e3)
    for k in ("cpu_baseline", "final_pass_ms", "jtwj_dense_mode", "local_scene"):
        assert k not in out                                   # --full only
    assert "peak_measured" not in out["roofline"]
    dx, par = np.load(tmp_path / "dx.npy"), np.load(tmp_path / "parameters.npy")
    assert dx.dtype == np.float64 and par.dtype == np.float64
    assert dx.shape == (18014,) and par.shape == (18014,)     # config 4: U = 18 014, no fixed slots
    assert np.isfinite(dx).all() and np.isfinite(par).all() and np.abs(dx).max() > 0
