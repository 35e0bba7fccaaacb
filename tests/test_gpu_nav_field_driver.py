"""planPathOptimal and plan_path_to_frontier_by_cost, in Python (botlab_amd/host.py) and in C++ (include/botlab/planning_dropin.hpp,
nav_field.hpp; tests/cpp/nav_field_test.cpp built with g++ -std=c++11), against the model (tests/nav_field_model.py) on the SLAM
maps from the smoke pose."""
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import botlab_amd as bl
import helpers
import nav_field_model as nm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPM = helpers.CPM_DEFAULT
START = (-0.75, 0.2, 0.0)                    # the smoke pose
GOAL = (-0.35, 0.2)
UTIME = 4242


def _build(td):
    exe = os.path.join(td, "nav_field_test")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "nav_field_test.cpp"),
                           "-L" + os.path.join(ROOT, "botlab_amd"), "-lbotlab_hip", "-Wl,-rpath," + os.path.join(ROOT, "botlab_amd"), "-o", exe])
    return exe


def _write_map_file(path, cells, origin, mpc):
    """The reference's ASCII .map format (occupancy_grid.cpp:111-136)."""
    with open(path, "w") as f:
        f.write(f"{float(origin[0]):g} {float(origin[1]):g} {cells.shape[1]} {cells.shape[0]} {float(mpc):g}\n")
        for row in cells:
            f.write(" ".join(str(int(v)) for v in row) + " \n")


def _poses(raw, off, n):
    a = np.zeros(n, nm.POSE)
    for k in range(n):
        a[k] = struct.unpack_from("<qfff", raw, off + 20 * k) + (0,)
    return a, off + 20 * n


def _run_cpp(exe, td, m, START, GOAL, radius):
    mapfile, outp = os.path.join(td, "m.map"), os.path.join(td, "o.bin")
    _write_map_file(mapfile, m["cells"], m["origin"], m["mpc"])
    r = subprocess.run([exe, mapfile, outp] + [repr(float(v)) for v in tuple(START) + tuple(GOAL) + (radius,)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0 and b"nav_field_test ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    raw = open(outp, "rb").read()
    assert raw[0:1] == b"P"
    n, cost = struct.unpack_from("<iI", raw, 1)
    opt, off = _poses(raw, 9, n)
    assert raw[off:off + 1] == b"F"
    nfr, = struct.unpack_from("<i", raw, off + 1)
    off += 5
    fr = []
    for _ in range(nfr):
        k, = struct.unpack_from("<i", raw, off)
        fr.append(np.frombuffer(raw, np.float32, 2 * k, off + 4).reshape(-1, 2).copy())
        off += 4 + 8 * k
    assert raw[off:off + 1] == b"C"
    n2, fi, cost2, reach = struct.unpack_from("<iiIi", raw, off + 1)
    byc, off = _poses(raw, off + 17, n2)
    assert raw[off:off + 1] == b"T"
    stats = struct.unpack_from("<5q", raw, off + 1)
    assert raw[off + 41:off + 42] == b"E"
    return dict(opt=opt, cost=cost, frontiers=fr, by_cost=byc, frontier=fi, cost2=cost2, reach=reach, stats=stats)


def _same(a, b):
    return len(a) == len(b) and all(a[k].tobytes() == b[k].tobytes() for k in ("utime", "x", "y", "theta"))


def _as_array(path):
    a = np.zeros(len(path), nm.POSE)
    for k, p in enumerate(path):
        a[k] = (p.utime, p.x, p.y, p.theta, 0)
    return a


@pytest.mark.parametrize("name", helpers.SLAM_MAPS)
def test_optimal_plans_equal_the_model_in_python_and_cpp(maps, gpu_ctx, name):
    """The SLAM maps from the smoke pose.  (No frontier is reachable from it on these maps: the frontier planner meets the empty
    list here, and real frontiers in test_cheapest_frontier_of_an_explored_disc.)"""
    _check(maps[name], name, gpu_ctx, START, GOAL, radius=0.2, n_min=3)


def test_cheapest_frontier_of_an_explored_disc(maps, gpu_ctx):
    """A 400 x 400 tiling of the maze, known inside a disc of 150 cells around the middle and unknown outside: frontiers all around,
    the robot on the traversable cell nearest the middle."""
    from botlab_amd import synth
    world = synth.tile_world(maps["astar_maze"]["cells"], 400)
    yy, xx = np.ogrid[:400, :400]
    cells = np.where((xx - 200) ** 2 + (yy - 200) ** 2 <= 150 ** 2, world, 0).astype(np.int8)
    m = dict(cells=cells, origin=(np.float32(-10.0), np.float32(-10.0)), mpc=np.float32(0.05))
    p = nm.Params(0.1, 1.0, 1.0)
    tcell, _ = nm.cell_tables(nm.l1_distances(cells), *nm.tables(nm.dist_table(400, 400), p))
    ys, xs = np.nonzero(tcell)
    c = int(np.argmin((xs - 200) ** 2 + (ys - 200) ** 2))
    f = int(np.argmax((xs - 200) ** 2 + (ys - 200) ** 2))
    start = (-10.0 + (xs[c] + 0.5) * 0.05, -10.0 + (ys[c] + 0.5) * 0.05, 0.25)
    goal = (-10.0 + (xs[f] + 0.5) * 0.05, -10.0 + (ys[f] + 0.5) * 0.05)
    found = _check(m, "explored_disc", gpu_ctx, start, goal, radius=0.1, n_min=2)
    assert found["frontiers"] > 0 and found["path"] > 1 and found["frontier"] >= 0


def _check(m, name, gpu_ctx, START, GOAL, radius, n_min):
    cells = m["cells"]
    h, w = cells.shape
    l1 = nm.l1_distances(cells)
    p = nm.Params(radius, 10.0 * radius, 1.0)                     # MotionPlannerParams(radius): max = 10 * min, exponent 1
    trav, pen = nm.tables(nm.dist_table(w, h), p)
    start = (UTIME, np.float32(START[0]), np.float32(START[1]), np.float32(START[2]))

    # ---- Python
    g = bl.OccupancyGrid.from_cells(cells, m["origin"], m["mpc"], cellsPerMeter=CPM, ctx=gpu_ctx)
    planner = bl.MotionPlanner(bl.MotionPlannerParams(radius), ctx=gpu_ctx)
    planner.setMap(g)
    s, gl = bl.make_pose(*START, utime=UTIME), bl.make_pose(GOAL[0], GOAL[1], 0.0)
    path, cost = planner.planPathOptimal(s, gl, return_cost=True)
    goal_cell = nm.pose_cell(GOAL, m["origin"], CPM, w, h)
    if planner.isValidGoal(gl):
        field = nm.dijkstra(l1, trav, pen, [goal_cell], 0)
        exp, _, exp_cost = nm.descend(field, l1, trav, pen, [goal_cell], 0, start, m["origin"], m["mpc"], CPM)
    else:
        exp, exp_cost = _as_array([s]), nm.UNREACHED
    assert _same(_as_array(path), exp) and cost == exp_cost, (name, len(path), len(exp), cost, exp_cost)
    planner.setPrevGoal(gl)
    planner.setNumFrontiers(2)                                    # isValidGoal now fails: the goal is the previous goal
    failed = planner.planPathOptimal(s, gl)
    assert len(failed) == 1 and bytes(failed[0]) == bytes(s) and len(planner.planPath(s, gl)) == 1
    planner.setNumFrontiers(1)

    frontiers = bl.find_map_frontiers(g, s)
    fr = frontiers.cells()
    planner.setNumFrontiers(len(fr))
    bpath, fi, bcost = bl.plan_path_to_frontier_by_cost(frontiers, s, g, planner)
    assert bl.plan_path_to_frontier_by_cost([], s, g, planner) == ([], -1, nm.UNREACHED)
    reach = next(n for n in range(w + h + 1) if trav[n])          # n_min
    assert reach == n_min
    ox, oy = float(m["origin"][0]), float(m["origin"][1])
    goals, owner = [], []
    for k, f in enumerate(fr):
        for x, y in f:
            goals.append((int((float(x) - ox) * float(CPM)), int((float(y) - oy) * float(CPM))))
            owner.append(k)
    field = nm.dijkstra(l1, trav, pen, goals, reach) if goals else np.full((h, w), nm.UNREACHED, np.uint32)
    exp, label, exp_cost = nm.descend(field, l1, trav, pen, goals, reach, start, m["origin"], m["mpc"], CPM)
    if not fr:                                                    # no frontier: the empty path, as plan_path_to_frontier gives
        exp, label, exp_cost = exp[:0], -1, nm.UNREACHED
    assert _same(_as_array(bpath), exp) and bcost == exp_cost and fi == (owner[label] if label >= 0 else -1), (name, len(bpath), len(exp), fi, label)
    print(name, "frontiers", len(fr), "cells", len(goals), "path", len(bpath), "frontier", fi, "cost", bcost)
    if len(bpath) > 1:
        # the path ends within reach_cells of a cell of the reported frontier
        ex = int(round((bpath[-1].x - ox) / float(m["mpc"])))
        ey = int(round((bpath[-1].y - oy) / float(m["mpc"])))
        near = [max(abs(gx - ex), abs(gy - ey)) for (gx, gy), k in zip(goals, owner) if k == fi]
        assert min(near) <= reach

    # ---- C++
    with tempfile.TemporaryDirectory() as td:
        r = _run_cpp(_build(td), td, m, START, GOAL, radius)
    assert len(r["frontiers"]) == len(fr) and all(np.array_equal(a, b) for a, b in zip(r["frontiers"], fr))
    assert _same(r["opt"], _as_array(path)) and r["cost"] == cost
    assert _same(r["by_cost"], _as_array(bpath)) and r["frontier"] == fi and r["cost2"] == bcost and r["reach"] == reach
    assert r["stats"][2] == int(nm.cell_tables(l1, trav, pen)[0].sum())
    return dict(frontiers=len(fr), path=len(bpath), frontier=fi)
