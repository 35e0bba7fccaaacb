"""A plain `bench.py --gpus 1 --steps K --warmup W` run: K timed steps, one result line with the contract's keys and nothing of
--full, and with --dump-outputs the same outputs from two runs of the same command."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(dump_dir, steps):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "5", "--dump-outputs", dump_dir]
    out = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0, out.stderr.decode()[-3000:]
    lines = [l for l in out.stdout.decode().splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1, out.stdout.decode()[-2000:]
    return json.loads(lines[0])


def test_plain_run_and_its_outputs(tmp_path):
    a = _run(str(tmp_path / "a"), 20)
    b = _run(str(tmp_path / "b"), 20)
    for r in (a, b):
        assert r["steps"] == 20 and r["warmup"] == 5 and r["unit"] == "steps/s" and r["higher_is_better"] is True
        assert r["metric"] == "SLAM steps/sec (map+MCL+A*)" and r["dtype"]
        assert abs(r["ms_per_step"] - 1e3 / r["value"]) < 1e-5                      # (both rounded to 6 decimals on the line)
        assert "cpu_baseline" not in r and "summary" not in r and "detail" not in r
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["map.npy", "particles.npy", "path.npy", "pose.npy"] and files == sorted(os.listdir(tmp_path / "b"))
    for f in files:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype in (np.float32, np.float64) and x.tobytes() == y.tobytes(), f
    pose = np.load(tmp_path / "a" / "pose.npy")
    assert pose[1:].tolist() == pytest.approx(a["final_pose"], abs=1e-6)
    assert np.load(tmp_path / "a" / "map.npy").shape == (200, 200) and np.load(tmp_path / "a" / "particles.npy").shape == (100_000, 9)
