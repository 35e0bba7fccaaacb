"""LoopCloserT::findPlaces / places and OccupancyGridSLAMT::closeLoopsByPlace (include/botlab/loop_closer.hpp, slam_driver.hpp), built
with g++ -std=c++11 from tests/cpp/place_closer_test.cpp:

  * findPlaces equals tests/place_model.py with nothing left out, on two named cases;
  * a mapping-only driver run that never calls closeLoopsByPlace and one that calls it after its last iteration write the same bytes
    up to that point, a driver without a history does nothing, and after the call the history's poses are those of
    LoopCloser.find_places and close_loops on the same history and the driver's map equals ScanHistory.rebuild at them."""
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import botlab_amd as bl
from botlab_amd import _capi

import loop_closure_model as lcm
import place_cases as pc
import place_model as pm
import test_gpu_slam_driver as drv
from test_gpu_loop_closure_cpp import _events, _poses_after, _same_poses
from test_gpu_place import DRIFT_CHAIN_INFO

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATE = 11.345
CELLS = 200 * 200


@pytest.fixture(scope="module")
def exe():
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "place_closer_test")
        subprocess.check_call(["g++", "-std=c++11", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "place_closer_test.cpp"),
                               "-L" + os.path.join(ROOT, "botlab_amd"), "-lbotlab_hip", "-Wl,-rpath," + os.path.join(ROOT, "botlab_amd"), "-o", path])
        yield path


def _params_bytes(p, capacity, max_rays):
    match = _capi.ScanMatchParams(p["nx"], p["ny"], p["ntheta"], float(np.float32(p["dtheta"])), float(np.float32(p["max_range"])), p["min_score"], 0)
    prior = _capi.ScanMatchPrior(*p["prior"], p["half_life"], 1)
    prm = _capi.LoopCloseParams(p["stride"], p["min_gap"], 0.0, p["w"], p["submap_cells"], float(np.float32(p["maxLaserDistance"])), p["hitOdds"],
                                p["missOdds"], match, prior)
    place = _capi.PlaceParams(float(np.float32(p["bins_per_meter"])), float(np.float32(p["place_max_range"])), p["dilate"], p["min_key"], p["min_bits"])
    return bytes(prm) + bytes(place) + DRIFT_CHAIN_INFO.tobytes() + struct.pack("<d", GATE) + bytes(bl.posegraph_params()) + \
        struct.pack("<ii", capacity, max_rays)


def _run(exe, mode, ev, params):
    with tempfile.TemporaryDirectory() as td:
        sp, pp, op = os.path.join(td, "s.bin"), os.path.join(td, "p.bin"), os.path.join(td, "o.bin")
        drv._write_script(sp, 0, 200, ev)
        with open(pp, "wb") as f:
            f.write(params)
        r = subprocess.run([exe, mode, sp, pp, op], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert r.returncode == 0 and b"place_closer_test ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
        print(r.stdout.decode().strip())
        return open(op, "rb").read()


@pytest.mark.parametrize("name", ["revisit_plus_100", "stride_3"])
def test_find_places_equals_the_model(exe, name):
    case = pc.cases()[name]
    _, _, places, model = pc.model(name)
    S = case.params["submap_cells"]
    raw = _run(exe, "find", _events(case.scans, case.poses), _params_bytes(case.params, case.capacity, case.max_rays))
    M, = struct.unpack_from("<i", raw, 0)
    cands = np.frombuffer(raw, lcm.CANDIDATE_DTYPE, M, 4)
    off = 4 + 272 * M
    K, = struct.unpack_from("<i", raw, off)
    edges = np.frombuffer(raw, lcm.EDGE_DTYPE, K, off + 4)
    off += 4 + 80 * K
    Q, = struct.unpack_from("<i", raw, off)
    got_places = np.frombuffer(raw, pm.PLACE_DTYPE, Q, off + 4)
    off += 4 + 32 * Q
    assert len(model) >= 1 and M == len(model)
    assert got_places.tobytes() == places.tobytes()
    assert cands.tobytes() == lcm.records(model).tobytes()
    assert edges.tobytes() == lcm.edges(model).tobytes()
    for c in model:
        origin, cells = np.frombuffer(raw, np.float32, 2, off), np.frombuffer(raw, np.int8, S * S, off + 8).reshape(S, S)
        off += 8 + S * S
        assert np.array_equal(cells, c["cells"]) and origin.tobytes() == np.array(c["origin"], np.float32).tobytes()
    assert off == len(raw)


def test_driver_close_loops_by_place(exe, gpu_ctx):
    case = pc.cases()["drift"]
    params = dict(case.params)
    n = len(case.scans)
    raw = _run(exe, "driver", _events(case.scans, case.poses), _params_bytes(params, 256, 290))
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
    assert sorted(runs) == ["a", "b"] and runs["a"] == runs["b"] and len(runs["a"]) > CELLS + 21 * (n - 2)
    live = np.frombuffer(runs["b"][-CELLS:], np.int8).reshape(200, 200)
    assert raw[off:off + 1] == b"h"
    held, = struct.unpack_from("<i", raw, off + 1)
    recorded, off = _poses_after(raw, off + 5, held)
    assert held == n and np.array_equal(recorded[:, 0], [p[3] for p in case.poses])
    assert raw[off:off + 1] == b"g"
    kept_n, = struct.unpack_from("<i", raw, off + 1)
    res = np.frombuffer(raw, bl.POSEGRAPH_RESULT_DTYPE, 1, off + 5)
    after, off = _poses_after(raw, off + 45, held)
    assert raw[off:off + 1] == b"m" and off + 1 + CELLS == len(raw)
    got_map = np.frombuffer(raw, np.int8, CELLS, off + 1).reshape(200, 200)
    # the same on the Python side, from the poses the driver recorded
    history = bl.ScanHistory(256, 290, ctx=gpu_ctx)
    for k, s in enumerate(case.scans):
        history.append(s, bl.make_pose(recorded[k, 1], recorded[k, 2], recorded[k, 3], utime=int(recorded[k, 0])))
    like = bl.OccupancyGrid(10.0, 10.0, 0.05, ctx=gpu_ctx)
    closer = bl.LoopCloser(64, ctx=gpu_ctx)
    try:
        found = closer.find_places(history, like, **params)
        assert len(found) >= 1
        graph = bl.PoseGraph(held, max(len(found), 1), len(found) + 1, ctx=gpu_ctx)
        try:
            want_kept, want_res, want_poses, _ = bl.close_loops(history, graph, found, DRIFT_CHAIN_INFO, gate=GATE)
        finally:
            graph.close()
        assert kept_n == len(want_kept) >= 1 and res.tobytes() == want_res[:1].tobytes()
        assert _same_poses(after, want_poses)
        out = bl.OccupancyGrid(10.0, 10.0, 0.05, ctx=gpu_ctx)
        history.rebuild(out, 5.0, 3, 1)
        expect = out.cells()
        out.close()
        assert (expect != 0).sum() > 500 and np.array_equal(got_map, expect), f"{(got_map != expect).sum()} cells differ"
        assert not np.array_equal(got_map, live)
    finally:
        closer.close(); like.close(); history.close()
