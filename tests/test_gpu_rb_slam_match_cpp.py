"""RaoBlackwellizedSLAMT::setScanMatching / clearScanMatching (include/botlab/rb_slam.hpp; tests/cpp/rb_slam_match_test.cpp built with
g++ -std=c++11) on a short recorded run against the model (tests/rb_slam_match_model.py): moved, resampled, best index and SLAM pose of
every update, the best map and all poses.  Matching is on for the first OFF_FROM updates and cleared for the rest."""
import math
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import rb_slam_match_model as rmm
from test_gpu_nav_field_driver import _write_map_file
from test_rb_slam_model_cpu import CPM, HIT, MAX_LASER, MISS, make_run

pytestmark = pytest.mark.gpu
MATCH = (2, 2, 2, np.float32(math.radians(0.5)).item(), 8.0, 0)
OFF_FROM = 6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe():
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "rb_slam_match_test")
        subprocess.check_call(["g++", "-std=c++11", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "rb_slam_match_test.cpp"),
                               "-L" + os.path.join(ROOT, "botlab_amd"), "-lbotlab_hip", "-Wl,-rpath," + os.path.join(ROOT, "botlab_amd"), "-o", out])
        yield out


def _pose_bytes(utime, x, y, th):
    return struct.pack("<qfff", int(utime), np.float32(x), np.float32(y), np.float32(th))


def test_cpp_class_matches_the_model(oracle, maps, exe):
    m, poses, odoms, scans = make_run(maps, 8)
    P = 12
    mdl = rmm.RBSlamMatchModel(oracle, P, m["cells"].shape, m["mpc"], CPM, m["origin"], MAX_LASER, HIT, MISS, 1, 1)
    mdl.init_at_pose(odoms[0][0], odoms[0][1], odoms[0][2], 1000)
    assert mdl.set_scan_matching(*MATCH)
    rng = np.random.default_rng(21)
    p = mdl.parts.copy()
    p["x"] += rng.normal(0, 0.01, P).astype(np.float32)
    p["p_x"] = p["x"]
    mdl.set_particles(p)
    R = scans[0].num_ranges
    blob = struct.pack("<iiiiifii", P, len(odoms), R, 1, 1, MAX_LASER, HIT, MISS) + struct.pack("<iiiffii", *(MATCH + (OFF_FROM,))) + \
        _pose_bytes(1000, *odoms[0][:3])
    for q in mdl.parts:
        blob += _pose_bytes(q["utime"], q["x"], q["y"], q["theta"]) + _pose_bytes(q["p_utime"], q["p_x"], q["p_y"], q["p_theta"]) + struct.pack("<d", q["weight"])
    exp = []
    off_centre = 0
    for k in range(len(odoms)):
        if k == OFF_FROM:
            mdl.set_scan_matching(None)
        o = odoms[k]
        noise = mdl.draw_noise(o, rng)
        blob += _pose_bytes(o[3], o[0], o[1], o[2]) + struct.pack("<i", 500 + k) + scans[k].ranges.tobytes() + scans[k].thetas.tobytes() + \
            scans[k].times.tobytes() + noise.tobytes()
        exp.append(mdl.update(o, scans[k], 500 + k, noise))
        if exp[-1]["moved"] and k < OFF_FROM:
            off_centre += int(np.count_nonzero(mdl.match["di"] | mdl.match["dj"] | mdl.match["dk"]))
    assert off_centre > 0                                       # the run has matches that move a pose
    with tempfile.TemporaryDirectory() as td:
        run, outp, mapfile = os.path.join(td, "run.bin"), os.path.join(td, "out.bin"), os.path.join(td, "m.map")
        open(run, "wb").write(blob)
        _write_map_file(mapfile, np.zeros_like(m["cells"]), m["origin"], m["mpc"])
        r = subprocess.run([exe, run, outp, mapfile], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 0 and b"rb_slam_match_test ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
        raw = open(outp, "rb").read()
    off = 0
    for k, e in enumerate(exp):
        moved, resampled, best = struct.unpack_from("<iii", raw, off)
        assert (bool(moved), bool(resampled), best) == (e["moved"], e["resampled"], e["best"]), k
        assert raw[off + 12:off + 32] == _pose_bytes(e["pose"][3], *e["pose"][:3]), k
        off += 32
    n = m["cells"].size
    assert raw[off:off + n] == mdl.maps[mdl.best].tobytes()
    off += n
    for q in mdl.parts:
        assert raw[off:off + 40] == _pose_bytes(q["utime"], q["x"], q["y"], q["theta"]) + _pose_bytes(q["p_utime"], q["p_x"], q["p_y"], q["p_theta"])
        off += 40
    assert off == len(raw)
