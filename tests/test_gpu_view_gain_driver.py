"""plan_path_to_frontier_by_gain in Python (botlab_amd/host.py) and in C++ (include/botlab/view_gain.hpp; tests/cpp/view_gain_test.cpp
built with g++ -std=c++11) against the model (tests/view_gain_model.py, tests/nav_field_model.py): the chosen cell, its frontier, gain
and cost, and the bytes of the path -- the one planPathOptimal gives to that cell -- on partially explored SLAM maps and on the
constructed map where the choice differs from plan_path_to_frontier_by_cost's."""
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import botlab_amd as bl
import helpers
import nav_field_model as nm
import view_gain_model as vm
from test_gpu_nav_field_driver import _as_array, _poses, _same, _write_map_file

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPM = helpers.CPM_DEFAULT
UTIME = 4242
RADIUS = 0.1
R, K = 40, 180


@pytest.fixture(scope="module")
def exe():
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "view_gain_test")
        subprocess.check_call(["g++", "-std=c++11", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "view_gain_test.cpp"),
                               "-L" + os.path.join(ROOT, "botlab_amd"), "-lbotlab_hip", "-Wl,-rpath," + os.path.join(ROOT, "botlab_amd"), "-o", out])
        yield out


def _choice(raw, off):
    return struct.unpack_from("<iiiII", raw, off), off + 20


def _run_cpp(exe, m, start):
    with tempfile.TemporaryDirectory() as td:
        mapfile, outp = os.path.join(td, "m.map"), os.path.join(td, "o.bin")
        _write_map_file(mapfile, m["cells"], m["origin"], m["mpc"])
        r = subprocess.run([exe, mapfile, outp] + [repr(float(v)) for v in tuple(start) + (RADIUS,)] + [str(R), str(K)], stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 0 and b"view_gain_test ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
        raw = open(outp, "rb").read()
    assert raw[0:1] == b"F"
    nfr, = struct.unpack_from("<i", raw, 1)
    off, fr = 5, []
    for _ in range(nfr):
        k, = struct.unpack_from("<i", raw, off)
        fr.append(np.frombuffer(raw, np.float32, 2 * k, off + 4).reshape(-1, 2).copy())
        off += 4 + 8 * k
    assert raw[off:off + 1] == b"R"
    nr, = struct.unpack_from("<i", raw, off + 1)
    ends = np.frombuffer(raw, np.int32, 2 * nr, off + 5).reshape(-1, 2).copy()
    off += 5 + 8 * nr
    assert raw[off:off + 1] == b"G"
    n, = struct.unpack_from("<i", raw, off + 1)
    choice, off = _choice(raw, off + 5)
    path, off = _poses(raw, off, n)
    assert raw[off:off + 1] == b"Z"
    zero, off = _choice(raw, off + 1)
    assert raw[off:off + 1] == b"N"
    none = struct.unpack_from("<iiii", raw, off + 1)
    assert raw[off + 17:off + 18] == b"E"
    return dict(frontiers=fr, ends=ends, choice=choice, path=path, zero=zero, none=none)


def _start_near(cells, spot, origin, mpc):
    """The pose at the middle of the traversable cell nearest `spot`, and the tables of the metric."""
    h, w = cells.shape
    l1 = nm.l1_distances(cells)
    trav, pen = nm.tables(nm.dist_table(w, h), nm.Params(RADIUS, 10.0 * RADIUS, 1.0))       # MotionPlannerParams(radius)
    tcell, _ = nm.cell_tables(l1, trav, pen)
    ys, xs = np.nonzero(tcell)
    k = int(np.argmin((xs - spot[0]) ** 2 + (ys - spot[1]) ** 2))
    start = (float(origin[0]) + (xs[k] + 0.5) * float(mpc), float(origin[1]) + (ys[k] + 0.5) * float(mpc), 0.25)
    return start, l1, trav, pen


def _check(m, name, gpu_ctx, exe, spot):
    cells = m["cells"]
    h, w = cells.shape
    start, l1, trav, pen = _start_near(cells, spot, m["origin"], m["mpc"])
    reach = next(n for n in range(w + h + 1) if trav[n])                                   # n_min
    g = bl.OccupancyGrid.from_cells(cells, m["origin"], m["mpc"], cellsPerMeter=CPM, ctx=gpu_ctx)
    planner = bl.MotionPlanner(bl.MotionPlannerParams(RADIUS), ctx=gpu_ctx)
    planner.setMap(g)
    s = bl.make_pose(*start, utime=UTIME)
    spose = (UTIME, np.float32(start[0]), np.float32(start[1]), np.float32(start[2]))
    frontiers = bl.find_map_frontiers(g, s)
    fr = frontiers.cells()
    planner.setNumFrontiers(len(fr))
    ox, oy = float(m["origin"][0]), float(m["origin"][1])
    fcells, owner = [], []
    for k, f in enumerate(fr):
        for x, y in f:
            fcells.append((int((float(x) - ox) * float(CPM)), int((float(y) - oy) * float(CPM))))
            owner.append(k)
    vg = bl.ViewGain(R, K, ctx=gpu_ctx)
    p = vm.Params(R, K)
    ends = vg.rayEnds()
    robot = nm.pose_cell((start[0], start[1]), m["origin"], CPM, w, h)

    def expected(**kw):
        c = vm.choose(cells, l1, trav, pen, robot, fcells, owner, reach, p, ends=ends, **kw) if fcells else None
        if c is None:
            return None, None
        field = nm.dijkstra(l1, trav, pen, [c["cell"]], 0)
        poses, _, _ = nm.descend(field, l1, trav, pen, [c["cell"]], 0, spose, m["origin"], m["mpc"], CPM)
        return c, poses

    # ---- Python
    want, want_path = expected()
    path, fi, cell, gain, cost = bl.plan_path_to_frontier_by_gain(frontiers, s, g, planner, view=vg)
    print(name, "frontiers", len(fr), "cells", len(fcells), "->", fi, cell, gain, cost, "path", len(path),
          "model", None if want is None else {k: v for k, v in want.items() if k != "field"})
    if not fr:
        assert (path, fi, cell, gain, cost) == ([], -1, None, 0, nm.UNREACHED)
    elif want is None:
        assert len(path) == 1 and bytes(path[0]) == bytes(s) and (fi, cell, gain, cost) == (-1, None, 0, nm.UNREACHED)
    else:
        assert (fi, cell, gain, cost) == (want["frontier"], want["cell"], want["gain"], want["cost"])
        assert _same(_as_array(path), want_path)
        goal = bl.make_pose(ox + (cell[0] + 0.5) * float(m["mpc"]), oy + (cell[1] + 0.5) * float(m["mpc"]), 0.0)
        assert nm.pose_cell((goal.x, goal.y), m["origin"], CPM, w, h) == cell
        if planner.isValidGoal(goal):
            opt, opt_cost = planner.planPathOptimal(s, goal, return_cost=True)
            assert _same(_as_array(opt), _as_array(path))
        # another weight, thinning, a floor on the gain
        wz, _ = expected(gain_weight=0, stride=2)
        z = bl.plan_path_to_frontier_by_gain(frontiers, s, g, planner, view=vg, gain_weight=0, stride=2)
        assert (z[1:] == (wz["frontier"], wz["cell"], wz["gain"], wz["cost"])) if wz else (z[1] == -1 and len(z[0]) == 1)
        w5, p5 = expected(gain_weight=5, min_gain=50)
        z5 = bl.plan_path_to_frontier_by_gain(frontiers, s, g, planner, view=vg, gain_weight=5, min_gain=50)
        assert (z5[1:] == (w5["frontier"], w5["cell"], w5["gain"], w5["cost"]) and _same(_as_array(z5[0]), p5)) if w5 else z5[1] == -1
    # the empty frontier list and no surviving candidate
    assert bl.plan_path_to_frontier_by_gain([], s, g, planner, view=vg) == ([], -1, None, 0, nm.UNREACHED)
    n = bl.plan_path_to_frontier_by_gain(frontiers, s, g, planner, view=vg, min_gain=1 << 31) if fr else None
    assert n is None or (len(n[0]) == 1 and bytes(n[0][0]) == bytes(s) and n[1:] == (-1, None, 0, nm.UNREACHED))
    # a default view of its own
    if want is not None:
        d = bl.plan_path_to_frontier_by_gain(frontiers, s, g, planner)
        wd = vm.choose(cells, l1, trav, pen, robot, fcells, owner, reach, vm.Params(60, 360))
        assert d[1:] == (wd["frontier"], wd["cell"], wd["gain"], wd["cost"])

    # ---- C++
    r = _run_cpp(exe, m, start)
    assert len(r["frontiers"]) == len(fr) and all(np.array_equal(a, b) for a, b in zip(r["frontiers"], fr))
    assert np.array_equal(r["ends"], ends)
    if not fr:
        assert len(r["path"]) == 0 and r["choice"][0] == -1
    elif want is None:
        assert len(r["path"]) == 1 and r["choice"][0] == -1
    else:
        assert r["choice"] == (fi, cell[0], cell[1], gain, cost)
        assert _same(r["path"], _as_array(path))
        if wz:
            assert r["zero"] == (wz["frontier"],) + wz["cell"] + (wz["gain"], wz["cost"])
        else:
            assert r["zero"][0] == -1
    assert r["none"][0] == 0 and r["none"][1] == -1 and r["none"][3] == -1 and r["none"][2] == (1 if fr else 0)
    by_cost = bl.plan_path_to_frontier_by_cost(frontiers, s, g, planner)[1] if fr else -1
    vg.close()
    g.close()
    return dict(frontiers=len(fr), frontier=fi, by_cost=by_cost, gain=gain, want=want)


@pytest.mark.parametrize("name", helpers.SLAM_MAPS)
def test_partially_explored_slam_maps(maps, gpu_ctx, exe, name):
    cells, spot = vm.partially_explored(maps[name]["cells"])
    m = dict(cells=cells, origin=maps[name]["origin"], mpc=maps[name]["mpc"])
    found = _check(m, name, gpu_ctx, exe, spot)
    assert found["frontiers"] > 0 and found["frontier"] >= 0 and found["gain"] >= 1


def test_choice_differs_from_the_cost_rule_on_the_constructed_map(gpu_ctx, exe):
    cells, origin, mpc, robot = vm.two_frontier_map()
    found = _check(dict(cells=cells, origin=origin, mpc=mpc), "two_frontier_map", gpu_ctx, exe, robot)
    assert found["frontiers"] == 2 and found["frontier"] >= 0 and found["by_cost"] >= 0
    assert found["frontier"] != found["by_cost"]
    assert found["gain"] > 120                       # more than the whole niche holds


def test_fully_known_map_has_no_frontier(maps, gpu_ctx, exe):
    """The smoke pose on a SLAM map as it is: no frontier is reachable, so the empty path and -1."""
    name = "obstacle_slam_10mx10m_5cm"
    m = maps[name]
    g = bl.OccupancyGrid.from_cells(m["cells"], m["origin"], m["mpc"], cellsPerMeter=CPM, ctx=gpu_ctx)
    planner = bl.MotionPlanner(bl.MotionPlannerParams(0.2), ctx=gpu_ctx)
    planner.setMap(g)
    s = bl.make_pose(-0.75, 0.2, 0.0, utime=UTIME)
    frontiers = bl.find_map_frontiers(g, s)
    if len(frontiers.cells()) == 0:
        assert bl.plan_path_to_frontier_by_gain(frontiers, s, g, planner) == ([], -1, None, 0, nm.UNREACHED)
    g.close()
