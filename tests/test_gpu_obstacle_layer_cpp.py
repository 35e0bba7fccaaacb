"""ObstacleLayerT (include/botlab/obstacle_layer.hpp) and MotionPlannerT::setMapWithObstacles (include/botlab/planning_dropin.hpp),
built with g++ -std=c++11 from tests/cpp/obstacle_layer_test.cpp and run on one hand-built case: everything the binary writes equals
the model (tests/obstacle_layer_model.py), and the planner's distances equal the Python host's transform of the model's composed
grid."""
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import botlab_amd as bl
import obstacle_layer_model as om
import test_obstacle_layer_model_cpu as cpu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(td):
    exe = os.path.join(td, "obstacle_layer_test")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "obstacle_layer_test.cpp"), "-L" + os.path.join(ROOT, "botlab_amd"),
                           "-lbotlab_hip", "-Wl,-rpath," + os.path.join(ROOT, "botlab_amd"), "-o", exe])
    return exe


def test_cpp_layer_and_planner_equal_the_model(gpu_ctx):
    w, h = 37, 23
    s = cpu.conditions_script(w, h, 1)
    updates = [st for st in s.steps[:4]]                              # two full scans, a scan of 0 rays, the pose outside the grid
    assert all(st[0] == "update" for st in updates)
    p = s.params
    model = om.Layer(w, h, **p)
    with tempfile.TemporaryDirectory() as td:
        exe = _build(td)
        inp, outp = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
        with open(inp, "wb") as f:
            f.write(struct.pack("<iifff", w, h, float(s.mpc), float(s.origin[0]), float(s.origin[1])))
            f.write(s.cells.tobytes())
            f.write(struct.pack("<fiiii", p["max_range"], p["occ_min"], p["tol_cells"], p["ttl_scans"], p["min_hits"]))
            f.write(struct.pack("<i", len(updates)))
            for _, r, t, pose in updates:
                f.write(struct.pack("<i", len(r)) + r.tobytes() + t.tobytes() + struct.pack("<fff", *[float(v) for v in pose]))
        r = subprocess.run([exe, inp, outp], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert r.returncode == 0 and b"obstacle_layer_test ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
        raw = open(outp, "rb").read()
    off = 0
    for k, (_, rr, tt, pose) in enumerate(updates):
        exp = model.update(s.cells, s.origin, np.float32(1.0) / s.mpc, rr, tt, pose)
        assert raw[off:off + 1] == b"U"
        n, = struct.unpack_from("<i", raw, off + 1)
        assert n == len(exp) and raw[off + 5:off + 5 + n] == exp.tobytes(), k
        st = struct.unpack_from("<Ii5iiii", raw, off + 5 + n)
        ms = model.stats()
        assert st == (ms["n"], ms["valid"], *ms["classes"], ms["hs"], ms["clr"], ms["live"]), (k, st, ms)
        off += 5 + n + 40
    assert raw[off:off + 1] == b"S"
    n, = struct.unpack_from("<I", raw, off + 1)
    count = np.frombuffer(raw, np.uint8, w * h, off + 5).reshape(h, w)
    last = np.frombuffer(raw, np.uint32, w * h, off + 5 + w * h).reshape(h, w)
    assert n == model.n and np.array_equal(count, model.count) and np.array_equal(last, model.last)
    off += 5 + 5 * w * h
    assert raw[off:off + 1] == b"L"
    nl, = struct.unpack_from("<i", raw, off + 1)
    live = np.frombuffer(raw, np.int32, 2 * nl, off + 5).reshape(nl, 2)
    assert nl > 0 and np.array_equal(live, model.live_cells())
    off += 5 + 8 * nl
    composed = model.compose(s.cells)
    for tag in (b"G", b"P"):
        assert raw[off:off + 1] == tag
        assert np.array_equal(np.frombuffer(raw, np.int8, w * h, off + 1).reshape(h, w), composed), tag
        off += 1 + w * h
    dist = np.frombuffer(raw, np.float32, w * h, off).reshape(h, w)
    off += 4 * w * h
    assert raw[off:off + 1] == b"E" and off + 1 == len(raw)
    g = bl.OccupancyGrid.from_cells(composed, s.origin, s.mpc, ctx=gpu_ctx)
    d = bl.ObstacleDistanceGrid(ctx=gpu_ctx)
    try:
        d.setDistances(g)
        assert np.array_equal(d.cells().view(np.uint32), dist.view(np.uint32))
    finally:
        d.close()
        g.close()
