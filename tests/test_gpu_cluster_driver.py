"""OccupancyGridSLAMT with setGlobalLocalizationByCluster (include/botlab/slam_driver.hpp), built with g++ -std=c++11 from
tests/cpp/cluster_driver_test.cpp: the calibrated scenario of tests/test_gpu_global_localization_driver.py (tests/global_init_model.py,
CAL_*; 100 000 particles), a start the driver is not told.  Until the heaviest cluster leads the known map stays byte-identical to the
file; convergence comes within the scans; from then on the poses track the truth and the map is extended every iteration.  The
whole-cloud rule runs on the same inputs and both convergence iterations are printed; no ratio between them is asserted.  The bins
(AMCL's 0.5 m and 10 degrees) and the share of 0.9 are untuned knobs, chosen before the scenario was first run.

Measured on an MI355X: the cluster rule converged at iteration 17, the spread rule at iteration 20 (of 60)."""
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
BIN_XY, THETA_BINS, MIN_SHARE = 0.5, 36, 0.9
REC = "<iiiqffffffd"


def _iterations(raw):
    its, off = [], 0
    while raw[off:off + 1] == b"I":
        its.append(struct.unpack_from(REC, raw, off + 1))
        off += 1 + struct.calcsize(REC)
    assert raw[off:off + 1] == b"E"
    return its


def test_driver_global_localization_by_cluster(maps):
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
        exe = os.path.join(td, "cluster_driver_test")
        subprocess.check_call(["g++", "-std=c++11", "-O2", "-I" + os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "cpp", "cluster_driver_test.cpp"), "-L" + os.path.join(ROOT, "botlab_amd"),
                               "-lbotlab_hip", "-Wl,-rpath," + os.path.join(ROOT, "botlab_amd"), "-o", exe])
        mapfile, script = os.path.join(td, "known.map"), os.path.join(td, "s.bin")
        _write_map_file(mapfile, m)
        with open(script, "wb") as f:
            f.write(struct.pack("<ii", n, len(ev)))
            for kind, x in ev:
                f.write(kind.encode())
                if kind == "O":
                    f.write(struct.pack("<qfff", int(x[0]), x[1], x[2], x[3]))
                else:
                    f.write(struct.pack("<qi", x.utime, x.num_ranges) + x.ranges.tobytes() + x.thetas.tobytes() + x.times.tobytes())
        runs = {}
        for rule, extra in (("cluster", [str(BIN_XY), str(THETA_BINS), str(MIN_SHARE)]), ("spread", [])):
            outp = os.path.join(td, rule + ".bin")
            out = subprocess.check_output([exe, script, mapfile, outp, rule] + extra, stderr=subprocess.DEVNULL, timeout=300).decode()
            assert "cluster_driver_test ok" in out
            runs[rule] = _iterations(open(outp, "rb").read())
    firsts = {rule: next((i for i, it in enumerate(its) if it[0]), None) for rule, its in runs.items()}
    print("convergence iteration: cluster rule %s, spread rule %s (of %d)" % (firsts["cluster"], firsts["spread"], len(poses) - 1))
    its = runs["cluster"]
    assert len(its) == len(poses) - 1                        # one iteration per scan
    first = firsts["cluster"]
    assert first is not None, "the cluster rule did not converge within the scenario"
    for i, (conv, same, maps_made, t, x, y, th, px, py, pth, share) in enumerate(its[:first]):
        assert not conv and same == 1 and maps_made == 0    # the known map is untouched while the filter searches
        assert 0.0 < share <= 1.0 and (x, y, th) == (px, py, pth)      # SLAM_POSE carries the heaviest cluster's pose
    assert its[first][10] >= MIN_SHARE
    for i, (conv, same, maps_made, t, x, y, th, px, py, pth, share) in enumerate(its[first:], start=first):
        assert conv == 1 and maps_made == i - first + 1     # converged stays converged; the map is extended every iteration
        tr = poses[i + 1]
        assert math.hypot(x - tr[0], y - tr[1]) <= gm.CAL_EST_TOL, (i, (x, y), tr)
    assert its[-1][1] == 0                                   # and the extension changed it
