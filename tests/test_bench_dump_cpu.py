"""bench.py's --dump-outputs and --full on the CPU stand-in step (--stub): the dump holds what the last timed
step computed, is identical from run to run with the same arguments, and a plain run leaves out everything
that --full adds.  No GPU."""
import json
import os
import subprocess
import sys

import numpy as np

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env["OMP_NUM_THREADS"] = "2"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--stub", "--batch", "8", "--points", "64"] + extra,
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_dump_is_the_last_step_and_reproducible(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    la = _run(["--steps", "3", "--warmup", "1", "--dump-outputs", str(a)])
    lb = _run(["--steps", "3", "--warmup", "1", "--dump-outputs", str(b)])
    assert la["steps"] == 3 and la["warmup"] == 1 and la["ms_per_step"] > 0
    names = sorted(os.listdir(a))
    assert names == ["grads.npy", "loss.npy", "out.npy", "state.npy"]
    assert sorted(os.listdir(b)) == names
    for n in names:
        x, y = np.load(a / n), np.load(b / n)
        assert x.dtype == np.float32 and np.array_equal(x, y), n
    assert np.load(a / "out.npy").shape == (6, 8, 32, 3)
    assert abs(float(np.load(a / "loss.npy")) - la["loss"]) < 1e-6            # the loss the line reports
    c = tmp_path / "c"                                                          # one step more: another state
    _run(["--steps", "4", "--warmup", "1", "--dump-outputs", str(c)])
    assert not np.array_equal(np.load(a / "state.npy"), np.load(c / "state.npy"))


def test_plain_run_is_lean_and_full_adds_the_rest():
    plain = _run(["--steps", "2", "--warmup", "1"])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in plain
    assert "cpu_baseline" not in plain and "parity" not in plain and "workloads" not in plain
    full = _run(["--steps", "2", "--warmup", "1", "--full", "--cpu-batch", "2"])
    assert full["cpu_baseline"]["unit"] == "segments/s" and full["cpu_baseline"]["value"] > 0
    assert "cpu_baseline" not in _run(["--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline"])


def test_large_arrays_are_a_fixed_seeded_sample(tmp_path, monkeypatch):
    import torch
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 1000)
    t = torch.arange(5000, dtype=torch.float32).reshape(50, 100)
    bench.dump_outputs(str(tmp_path / "a"), {"x": t, "y": torch.ones(10, dtype=torch.float64)})
    bench.dump_outputs(str(tmp_path / "b"), {"x": t})
    x = np.load(tmp_path / "a" / "x.npy")
    assert x.shape == (1000,) and x.dtype == np.float32
    assert np.all(np.diff(x) > 0) and np.array_equal(x, np.load(tmp_path / "b" / "x.npy"))
    assert np.load(tmp_path / "a" / "y.npy").dtype == np.float64
