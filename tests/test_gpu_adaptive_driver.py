"""OccupancyGridSLAMT with setGlobalLocalization(true) and setAdaptiveParticles(true) (include/botlab/slam_driver.hpp), built with
g++ -std=c++11 from tests/cpp/adaptive_driver_test.cpp: localization-only mode on a map file, a start the driver is not told, the
calibrated scenario of tests/global_init_model.py at capacity 100 000.  The filter converges within CAL_K moved updates, tracks
within CAL_EST_TOL of the truth from then on, and every update after the first converged iteration draws at most 10 % of the
capacity."""
import math
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import global_init_model as gm
from botlab_amd import synth
from test_gpu_global_localization_driver import _odometry_frame, _write_map_file

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(td):
    exe = os.path.join(td, "adaptive_driver_test")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "adaptive_driver_test.cpp"), "-L" + os.path.join(ROOT, "botlab_amd"),
                           "-lbotlab_hip", "-Wl,-rpath," + os.path.join(ROOT, "botlab_amd"), "-o", exe])
    return exe


def test_driver_adaptive_global_localization(maps):
    n = 100_000
    m = maps[gm.CAL_MAP]
    truth = np.where(m["cells"] > 0, 127, -127).astype(np.int8)
    poses = synth.square_trajectory(gm.CAL_START, gm.CAL_STEPS, **gm.CAL_TRAJ)
    odo = _odometry_frame(poses)
    t0 = 1_000_000
    ev = []
    for k in range(len(poses)):
        t = t0 + k * 100_000
        ev.append(("O", (t, *[np.float32(v) for v in odo[k]])))
        if k >= 1:
            ev.append(("L", synth.raycast_scan(truth, m["origin"], 0.05, poses[k - 1], poses[k], t)))
    with tempfile.TemporaryDirectory() as td:
        exe = _build(td)
        mapfile, script, outp = os.path.join(td, "known.map"), os.path.join(td, "s.bin"), os.path.join(td, "o.bin")
        _write_map_file(mapfile, m)
        with open(script, "wb") as f:
            f.write(struct.pack("<ii", n, len(ev)))
            for kind, x in ev:
                f.write(kind.encode())
                if kind == "O":
                    f.write(struct.pack("<qfff", int(x[0]), x[1], x[2], x[3]))
                else:
                    f.write(struct.pack("<qi", x.utime, x.num_ranges) + x.ranges.tobytes() + x.thetas.tobytes() + x.times.tobytes())
        out = subprocess.check_output([exe, script, mapfile, outp], stderr=subprocess.DEVNULL, timeout=300).decode()
        assert "adaptive_driver_test ok" in out
        raw = open(outp, "rb").read()
    its, off = [], 0
    while raw[off:off + 1] == b"I":
        its.append(struct.unpack_from("<iiiqfff", raw, off + 1))
        off += 1 + struct.calcsize("<iiiqfff")
    assert raw[off:off + 1] == b"E"
    assert len(its) == len(poses) - 1
    assert all(on == 1 for _, on, *_ in its)
    assert its[0][2] == n                                    # seeded with the whole capacity
    first = next(i for i, it in enumerate(its) if it[0])
    assert first <= gm.CAL_K, first
    actives = [it[2] for it in its]
    for i, (conv, on, active, t, x, y, th) in enumerate(its[first:], start=first):
        assert conv == 1
        tr = poses[i + 1]
        assert math.hypot(x - tr[0], y - tr[1]) <= gm.CAL_EST_TOL, (i, (x, y), tr)
        # the count an update draws is set by the cloud of the update before it: the iterations after the first converged one
        # are the ones whose count a converged cloud decided
        if i > first:
            assert active <= n // 10, (first, actives)
    assert first < len(its) - 5
