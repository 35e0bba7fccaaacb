"""PathShortcutT and MotionPlannerT::shortcutPath (include/botlab/path_shortcut.hpp, planning_dropin.hpp;
tests/cpp/path_shortcut_test.cpp built with g++ -std=c++11) on the obstacle map: the shortened model field path, its costs and its
kept indices against the model (tests/path_shortcut_model.py).  The input path is built on the CPU."""
import os
import struct
import subprocess

import numpy as np
import pytest

import helpers
import nav_field_model as nm
import path_shortcut_model as psm
import test_path_shortcut_model_cpu as cpu
from test_gpu_nav_field_driver import _write_map_file

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPM = helpers.CPM_DEFAULT


def build(td):
    exe = os.path.join(td, "path_shortcut_test")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "path_shortcut_test.cpp"),
                           "-L" + os.path.join(ROOT, "botlab_amd"), "-lbotlab_hip", "-Wl,-rpath," + os.path.join(ROOT, "botlab_amd"), "-o", exe])
    return exe


def run(exe, td, world, poses, p, plan=()):
    """The records of one run: {'S': (poses, cost, input cost), 'M': poses, 'C': kept indices, 'D': poses or None}."""
    mapfile, pathfile, outp = (os.path.join(td, n) for n in ("m.map", "path.bin", "out.bin"))
    _write_map_file(mapfile, world.cells, world.origin, world.mpc)
    open(pathfile, "wb").write(b"".join(poses[k].tobytes()[:20] for k in range(len(poses))))
    r = subprocess.run([exe, mapfile, pathfile, outp, repr(p.clearance), str(p.max_span), str(p.waypoint_cost)] + [repr(v) for v in plan],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0 and b"path_shortcut_test ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    raw = open(outp, "rb").read()

    def path_at(off):
        n, = struct.unpack_from("<i", raw, off)
        a = np.zeros(n, nm.POSE)
        for k in range(n):
            a[k] = struct.unpack_from("<qfff", raw, off + 4 + 20 * k) + (0,)
        return a, off + 4 + 20 * n

    out = {}
    assert raw[0:1] == b"S"
    s, off = path_at(1)
    out["S"] = (s,) + struct.unpack_from("<qq", raw, off)
    assert raw[off + 16:off + 17] == b"M"
    out["M"], off = path_at(off + 17)
    assert raw[off:off + 1] == b"C"
    n, = struct.unpack_from("<i", raw, off + 1)
    out["C"] = np.frombuffer(raw, np.int32, n, off + 5).copy()
    off += 5 + 4 * n
    out["D"] = None
    if raw[off:off + 1] == b"D":
        out["D"], off = path_at(off + 1)
    assert raw[off:off + 1] == b"E" and off + 1 == len(raw)
    return out


def same(a, b):
    return len(a) == len(b) and all(a[k].tobytes() == b[k].tobytes() for k in ("utime", "x", "y", "theta"))


def test_cpp_class_matches_the_model(maps, tmp_path):
    world, poses = cpu.map_case(maps)
    p = psm.Params(0.2, 64, 1024)
    exp, ec, ei = psm.shortcut_poses(world.ok(0.2), poses, world.origin, CPM, p)
    keep, _, _ = psm.shortcut(world.ok(0.2), psm.pose_cells(poses, world.origin, CPM, world.w, world.h), p)
    r = run(build(str(tmp_path)), str(tmp_path), world, poses, p)
    assert same(r["S"][0], exp) and r["S"][1:] == (ec, ei) and len(exp) < len(poses)
    assert same(r["M"], exp) and r["C"].tobytes() == keep.tobytes() and r["D"] is None
