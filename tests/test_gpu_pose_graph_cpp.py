"""PoseGraphT and OccupancyGridSLAMT::optimizeHistory (include/botlab/pose_graph.hpp, slam_driver.hpp), built with g++ -std=c++11 from
tests/cpp/pose_graph_test.cpp:

  * PoseGraphT equals tests/pose_graph_model.py bit for bit on three graphs, one of them with two subsets;
  * a mapping-only driver run that never calls optimizeHistory and one that calls it after its last iteration write the same bytes up
    to that point, a driver without a history does nothing, and no result exists without a call;
  * called with the loop edges that botlab_amd.find_loop_closures finds in the world of tests/test_gpu_loop_closure.py, the history's
    poses and lastPoseGraphResult() are the model's, and the driver's map equals ScanHistory.rebuild at the model's poses."""
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import botlab_amd as bl
import pose_graph_cases as pgc
import pose_graph_model as pgm
import test_gpu_loop_closure as lc
import test_gpu_slam_driver as drv

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CELLS = 200 * 200


def _build(td):
    exe = os.path.join(td, "pose_graph_test")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "pose_graph_test.cpp"),
                           "-L" + os.path.join(ROOT, "botlab_amd"), "-lbotlab_hip", "-Wl,-rpath," + os.path.join(ROOT, "botlab_amd"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def exe():
    with tempfile.TemporaryDirectory() as td:
        yield _build(td)


def _params_bytes(p):
    return bytes(bl.posegraph_params(**p._asdict()))


def _run(exe, *args):
    r = subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0 and b"pose_graph_test ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    print(r.stdout.decode().strip())


@pytest.mark.parametrize("name,n_subsets", [("n3_loop_0_2", 0), ("n100_l32", 2), ("n257_l33", 0)])
def test_posegraph_class_equals_the_model(exe, name, n_subsets):
    c = {k.name: k for k in pgc.cases()}[name]
    g = c.graph
    words = (g.L + 31) // 32
    masks = pgc.subset_masks(g.L, n_subsets, seed=5)[:, :words] if n_subsets else np.zeros((0, words), np.uint32)
    utime = 500 + 3 * np.arange(g.N)
    with tempfile.TemporaryDirectory() as td:
        cp, op = os.path.join(td, "case.bin"), os.path.join(td, "out.bin")
        with open(cp, "wb") as f:
            f.write(struct.pack("<iiii", g.N, g.L, n_subsets, words) + _params_bytes(c.params))
            for k in range(g.N):
                f.write(struct.pack("<qfff", int(utime[k]), g.nodes[k, 0], g.nodes[k, 1], g.nodes[k, 2]))
            f.write(bl.posegraph_edges(g.i, g.j, g.z, g.info).tobytes() + np.ascontiguousarray(masks).tobytes())
        _run(exe, "graph", cp, op)
        raw = open(op, "rb").read()
    off = 0
    for s in range(max(n_subsets, 1)):
        want = pgm.solve(g, c.params, masks[s] if n_subsets else None)
        res = np.frombuffer(raw, bl.POSEGRAPH_RESULT_DTYPE, 1, off)[0]; off += 40
        xyt = np.frombuffer(raw, np.float64, 3 * g.N, off).reshape(g.N, 3); off += 24 * g.N
        p32 = [struct.unpack_from("<qfff", raw, off + 20 * k) for k in range(g.N)]; off += 20 * g.N
        before = np.frombuffer(raw, np.float64, g.E, off); off += 8 * g.E
        after = np.frombuffer(raw, np.float64, g.E, off); off += 8 * g.E
        assert (res["tries"], res["accepted"], res["cg_iterations"], res["status"]) == (want.tries, want.accepted, want.cg_iterations, want.status)
        assert np.array([res["cost_before"], res["cost_after"], res["final_lambda"]]).tobytes() == \
            np.array([want.cost_before, want.cost_after, want.final_lambda]).tobytes()
        assert xyt.tobytes() == want.poses.tobytes() and before.tobytes() == want.chi2_before.tobytes() and after.tobytes() == want.chi2_after.tobytes()
        assert [q[0] for q in p32] == list(utime)
        assert np.array([q[1:] for q in p32], np.float32).tobytes() == want.poses32.tobytes()
    assert off == len(raw)


def _read_poses(raw, off, n):
    return np.array([struct.unpack_from("<qfff", raw, off + 20 * i) for i in range(n)], dtype=np.float64).reshape(n, 4), off + 20 * n


def test_optimize_history(exe, gpu_ctx):
    world = lc._world()
    truth, rec = lc._trajectories()
    rec_p = lc._poses(rec)
    scans = lc._scans(world, truth, rec_p["utime"])
    history = bl.ScanHistory(lc.N, 290, ctx=gpu_ctx)
    for k, s in enumerate(scans):
        history.append(s, bl.make_pose(rec[k, 0], rec[k, 1], rec[k, 2], utime=int(rec_p["utime"][k])))
    like = bl.OccupancyGrid(10.0, 10.0, 0.05, ctx=gpu_ctx)
    matcher = bl.ScanMatcher(ctx=gpu_ctx)
    try:
        loops = bl.find_loop_closures(history, matcher, like, stride=4, min_gap=40, radius=0.5, w=5, submap_cells=200, nx=8, ny=8, ntheta=12,
                                      dtheta=lc.DTHETA, max_range=8.0, half_life=64, maxLaserDistance=lc.MAX_LASER, hitOdds=lc.HIT, missOdds=lc.MISS)
        assert len(loops) >= 1
        ev = []
        for k, s in enumerate(scans):
            ev.append(("P", (int(rec_p["utime"][k]), rec_p["x"][k], rec_p["y"][k], rec_p["theta"][k])))
            ev.append(("L", s))
        with tempfile.TemporaryDirectory() as td:
            sp, lp, op = os.path.join(td, "s.bin"), os.path.join(td, "l.bin"), os.path.join(td, "o.bin")
            drv._write_script(sp, 0, 200, ev)
            with open(lp, "wb") as f:
                f.write(struct.pack("<i", len(loops)) + lc.CHAIN_INFO.tobytes() + _params_bytes(pgm.DEFAULT) + loops.tobytes())
            _run(exe, "driver", sp, lp, op)
            raw = open(op, "rb").read()
        # the two runs, byte for byte up to the call
        off, runs = 0, {}
        while raw[off:off + 1] == b"R":
            tag, start = raw[off + 1:off + 2].decode(), off + 2
            off = start
            while raw[off:off + 1] == b"I":
                off += 21
            assert raw[off:off + 1] == b"E"
            off += 1 + CELLS
            runs[tag] = raw[start:off]
        assert sorted(runs) == ["a", "b"] and runs["a"] == runs["b"] and len(runs["a"]) > CELLS + 21 * 100
        live = np.frombuffer(runs["b"][-CELLS:], np.int8).reshape(200, 200)
        assert raw[off:off + 1] == b"h"
        held, = struct.unpack_from("<i", raw, off + 1)
        recorded, off = _read_poses(raw, off + 5, held)
        assert held == lc.N and np.array_equal(recorded[:, 0], rec_p["utime"])
        assert raw[off:off + 1] == b"g"
        did, = struct.unpack_from("<i", raw, off + 1)
        res = np.frombuffer(raw, bl.POSEGRAPH_RESULT_DTYPE, 1, off + 5)[0]
        after, off = _read_poses(raw, off + 45, held)
        assert raw[off:off + 1] == b"m" and off + 1 + CELLS == len(raw)
        got_map = np.frombuffer(raw, np.int8, CELLS, off + 1).reshape(200, 200)
        # the model on the driver's recorded poses
        nodes = recorded[:, 1:]
        z = pgm.relative_pose(nodes[:-1], nodes[1:])
        ei, ej = np.concatenate([np.arange(held - 1), loops["i"]]), np.concatenate([np.arange(1, held), loops["j"]])
        g = pgm.Graph(nodes, ei, ej, np.concatenate([z, loops["z"]]), np.concatenate([np.tile(lc.CHAIN_INFO, (held - 1, 1)), loops["info"]]))
        want = pgm.solve(g, pgm.DEFAULT)
        assert did == 1 and want.accepted >= 1 and want.cost_after < want.cost_before
        assert (res["tries"], res["accepted"], res["cg_iterations"], res["status"]) == (want.tries, want.accepted, want.cg_iterations, want.status)
        assert res["cost_before"] == want.cost_before and res["cost_after"] == want.cost_after
        assert after[:, 1:].astype(np.float32).tobytes() == want.poses32.tobytes() and np.array_equal(after[:, 0], recorded[:, 0])
        model_poses = rec_p.copy()
        model_poses["x"], model_poses["y"], model_poses["theta"] = want.poses32[:, 0], want.poses32[:, 1], want.poses32[:, 2]
        out = bl.OccupancyGrid(10.0, 10.0, 0.05, ctx=gpu_ctx)
        history.rebuild(out, 5.0, 3, 1, poses=model_poses)
        expect = out.cells()
        out.close()
        assert (expect != 0).sum() > 500 and np.array_equal(got_map, expect), f"{(got_map != expect).sum()} cells differ"
        assert not np.array_equal(got_map, live)
    finally:
        matcher.close(); like.close(); history.close()
