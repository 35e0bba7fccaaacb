"""OccupancyGridSLAMT with setGlobalLocalization(true) (include/botlab/slam_driver.hpp), built with g++ -std=c++11 from
tests/cpp/global_localization_test.cpp: localization-only mode on a map file, a start the driver is not told (odometry in its own
frame), the calibrated scenario of tests/global_init_model.py.  Until the filter has converged the map stays byte-identical to the
file; convergence comes within CAL_K moved updates; from then on the poses track the truth and the map is extended every iteration."""
import math
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import global_init_model as gm
from botlab_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(td):
    exe = os.path.join(td, "global_localization_test")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "global_localization_test.cpp"), "-L" + os.path.join(ROOT, "botlab_amd"),
                           "-lbotlab_hip", "-Wl,-rpath," + os.path.join(ROOT, "botlab_amd"), "-o", exe])
    return exe


def _write_map_file(path, m):
    """The reference's ASCII .map format (occupancy_grid.cpp:111-136)."""
    c = m["cells"]
    with open(path, "w") as f:
        f.write(f"{float(m['origin'][0]):g} {float(m['origin'][1]):g} {c.shape[1]} {c.shape[0]} {float(m['mpc']):g}\n")
        for row in c:
            f.write(" ".join(str(int(v)) for v in row) + " \n")


def _odometry_frame(poses):
    """The truth expressed in a frame whose origin is the start pose: what wheel odometry reports from switch-on."""
    x0, y0, t0 = poses[0]
    c, s = math.cos(-t0), math.sin(-t0)
    out = []
    for x, y, t in poses:
        dx, dy = x - x0, y - y0
        out.append((c * dx - s * dy, s * dx + c * dy, math.atan2(math.sin(t - t0), math.cos(t - t0))))
    return out


def test_driver_global_localization(maps):
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
        assert "global_localization_test ok" in out
        raw = open(outp, "rb").read()
    its, off = [], 0
    while raw[off:off + 1] == b"I":
        conv, same, maps_made, t, x, y, th = struct.unpack_from("<iiiqfff", raw, off + 1)
        its.append((conv, same, maps_made, t, x, y, th))
        off += 1 + struct.calcsize("<iiiqfff")
    assert raw[off:off + 1] == b"E"
    assert len(its) == len(poses) - 1                        # one iteration per scan
    first = next(i for i, it in enumerate(its) if it[0])
    # iteration i processes scan i + 1; the first one only latches the odometry (no motion), so it is i moved updates
    assert first <= gm.CAL_K, first
    for conv, same, maps_made, *_ in its[:first]:
        assert not conv and same == 1 and maps_made == 0    # the known map is untouched while the filter searches
    for i, (conv, same, maps_made, t, x, y, th) in enumerate(its[first:], start=first):
        assert conv == 1 and maps_made == i - first + 1     # converged stays converged; the map is extended every iteration
        tr = poses[i + 1]
        assert math.hypot(x - tr[0], y - tr[1]) <= gm.CAL_EST_TOL, (i, (x, y), tr)
    assert its[-1][1] == 0                                   # and the extension changed it
    assert first < len(its) - 5                              # several tracked iterations after convergence
