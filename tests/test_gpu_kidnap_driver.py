"""OccupancyGridSLAMT with setKidnapRecovery(true) (include/botlab/slam_driver.hpp), built with g++ -std=c++11 from
tests/cpp/kidnap_recovery_test.cpp: localization-only mode on a map file, started at the true pose (the map frame is chosen so that
the start is its origin), the kidnap of tests/recovery_model.py.  Recovery is on from the start and injects nothing while the
filter tracks; after the kidnap the driver holds its map updates back while the filter injects, and ends within CAL_EST_TOL of the
truth."""
import math
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import global_init_model as gm
import recovery_model as rm
from botlab_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(td):
    exe = os.path.join(td, "kidnap_recovery_test")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "kidnap_recovery_test.cpp"), "-L" + os.path.join(ROOT, "botlab_amd"),
                           "-lbotlab_hip", "-Wl,-rpath," + os.path.join(ROOT, "botlab_amd"), "-o", exe])
    return exe


def _write_map_file(path, cells, origin, mpc):
    """The reference's ASCII .map format (occupancy_grid.cpp:111-136)."""
    with open(path, "w") as f:
        f.write(f"{float(origin[0]):g} {float(origin[1]):g} {cells.shape[1]} {cells.shape[0]} {float(mpc):g}\n")
        for row in cells:
            f.write(" ".join(str(int(v)) for v in row) + " \n")


def test_driver_kidnap_recovery(maps):
    n = 100_000
    m = maps[rm.KID_MAP]
    cells, mpc = m["cells"], m["mpc"]
    truthmap = np.where(cells > 0, 127, -127).astype(np.int8)
    x0, y0, t0 = rm.KID_START
    assert t0 == 0.0
    origin = (float(m["origin"][0]) - x0, float(m["origin"][1]) - y0)          # the start is the map frame's origin
    motion, truth, begin = rm.kidnap_truth()
    shift = lambda p: (p[0] - x0, p[1] - y0, p[2])
    ts = 1_000_000
    ev = []
    for k in range(len(truth)):
        t = ts + k * 100_000
        ev.append(("O", (t, *[np.float32(v) for v in shift(motion[k])])))      # exact wheel odometry of the motion the robot makes
        if k >= 1:
            ev.append(("L", synth.raycast_scan(truthmap, origin, 0.05, shift(begin[k]), shift(truth[k]), t)))
    with tempfile.TemporaryDirectory() as td:
        exe = _build(td)
        mapfile, script, outp = os.path.join(td, "known.map"), os.path.join(td, "s.bin"), os.path.join(td, "o.bin")
        _write_map_file(mapfile, cells, origin, mpc)
        with open(script, "wb") as f:
            f.write(struct.pack("<ii", n, len(ev)))
            for kind, x in ev:
                f.write(kind.encode())
                if kind == "O":
                    f.write(struct.pack("<qfff", int(x[0]), x[1], x[2], x[3]))
                else:
                    f.write(struct.pack("<qi", x.utime, x.num_ranges) + x.ranges.tobytes() + x.thetas.tobytes() + x.times.tobytes())
        out = subprocess.check_output([exe, script, mapfile, outp], stderr=subprocess.DEVNULL, timeout=600).decode()
        assert "kidnap_recovery_test ok" in out
        raw = open(outp, "rb").read()
    its, off = [], 0
    fmt = "<iiiiqfff"              # recovery on, injected so far, map updates so far, map updates held back so far, pose
    while raw[off:off + 1] == b"I":
        its.append(struct.unpack_from(fmt, raw, off + 1))
        off += 1 + struct.calcsize(fmt)
    assert raw[off:off + 1] == b"E" and len(its) == len(truth) - 1
    err = [math.hypot(it[5] - shift(truth[i + 1])[0], it[6] - shift(truth[i + 1])[1]) for i, it in enumerate(its)]
    trace = " ".join("%d:%.2f/%d/%d" % (i, e, it[2], it[3]) for i, (e, it) in enumerate(zip(err, its)))
    assert all(it[0] == 1 for it in its)                                        # on from the start (the filter starts at a pose)
    # iteration i processes scan i + 1 (the first one only latches the odometry): tracking until the kidnap injects nothing, and
    # every iteration extends the map
    assert its[rm.KID_K0 - 1][1] == 0 and its[rm.KID_K0 - 1][2] == rm.KID_K0 and its[rm.KID_K0 - 1][3] == 0, trace
    assert max(err[:rm.KID_K0]) <= gm.CAL_EST_TOL, trace
    # after the kidnap the filter injects and the driver holds the map back while it does; within KID_KR updates it is back at the truth
    assert its[-1][1] > 0 and its[-1][3] > 0, trace
    assert err[-1] <= gm.CAL_EST_TOL, trace
