"""The navigation field on the GPU (bl_navfield_*, botlab_amd/csrc/bl_navfield.hip) against its model (tests/nav_field_model.py):
tables, field, paths and gathers bit for bit on the small maps; on the large ones, where a Python Dijkstra is too slow for the
suite, the Bellman certificate on the downloaded field plus the path properties from 1000 starts."""
import ctypes as C

import numpy as np
import pytest

import botlab_amd as bl
from botlab_amd import _capi, synth
import helpers
import nav_field_model as nm
import test_nav_field_model_cpu as cpu

pytestmark = pytest.mark.gpu
CPM = helpers.CPM_DEFAULT


def _c_params(p):
    return _capi.NavFieldParams(p.minDistanceToObstacle, p.maxDistanceWithCost, p.distanceCostExponent, p.obstacle_gain, p.reach_cells)


def _map_of(name, maps):
    if name == "ragged":
        return dict(cells=cpu.ragged_cells(), origin=(np.float32(-4.0), np.float32(-5.0)), mpc=np.float32(0.05))
    return maps[name]


_dists = {}


def _dist(name, maps, ctx):
    """One device distance grid per map for the whole module."""
    if name not in _dists:
        m = _map_of(name, maps)
        g = bl.OccupancyGrid.from_cells(m["cells"], m["origin"], m["mpc"], cellsPerMeter=CPM, ctx=ctx)
        d = bl.ObstacleDistanceGrid(ctx=ctx)
        d.setDistances(g)
        l1 = cpu._l1(name)
        f = nm.dist_table(l1.shape[1], l1.shape[0])
        exp = np.where(l1 == nm.NONE16, np.float32(-1.0), f[np.minimum(l1, len(f) - 1)])
        assert np.array_equal(d.cells().view(np.uint32), exp.view(np.uint32)), name      # the model's n(c) and f[n] are the grid's
        _dists[name] = (g, d)
    return _dists[name][1]


@pytest.fixture(scope="module")
def nf(gpu_ctx):
    f = bl.NavigationField(gpu_ctx)
    yield f
    f.close()


def test_tables_equal_the_model(maps, gpu_ctx, nf):
    d = _dist("astar_maze", maps, gpu_ctx)
    f = nm.dist_table(200, 200)
    for p in (nm.Params(0.1, 1.0, 1.0), nm.Params(0.2, 2.0, 1.0), nm.Params(0.2, 2.0, 2.5, obstacle_gain=4095), nm.Params(0.3, 0.1, 1.0),
              nm.Params(0.15, 3.0, 0.5, obstacle_gain=7), nm.Params(0.0, 1.0, 0.0, obstacle_gain=1), nm.Params(0.2, 2.0, 1.0, obstacle_gain=0)):
        nf.compute(d, _c_params(p), [(100, 100)])
        trav, pen = nf.tables()
        et, ep = nm.tables(f, p)
        assert len(trav) == 401 and np.array_equal(trav, et) and np.array_equal(pen, ep), vars(p)


@pytest.mark.parametrize("case", cpu.CASES)
def test_field_paths_and_gather_equal_the_model(maps, gpu_ctx, nf, case):
    name, p, goals = cpu.cases()[case]
    l1, trav, pen, goals, p, field = cpu.solved(case)
    m = _map_of(name, maps)
    d = _dist(name, maps, gpu_ctx)
    nf.compute(d, _c_params(p), goals)
    got = nf.cells()
    assert got.dtype == np.uint32 and np.array_equal(got, field), (case, int((got != field).sum()))
    st = nf.stats()
    tcell, _ = nm.cell_tables(l1, trav, pen)
    mask, _ = nm.goal_set(tcell, goals, p.reach_cells)
    assert st["traversable"] == int(tcell.sum()) and st["reached"] == int((field != nm.UNREACHED).sum()) and st["goal_set"] == int(mask.sum())
    assert st["rounds"] <= st["traversable"] + 1                                    # the cap of the rounds
    print(case, st)
    # gather: every kind of cell, and off the grid
    h, w = l1.shape
    rng = np.random.default_rng(3)
    q = np.stack([rng.integers(-5, w + 5, 500), rng.integers(-5, h + 5, 500)], axis=1).astype(np.int32)
    inside = (q[:, 0] >= 0) & (q[:, 0] < w) & (q[:, 1] >= 0) & (q[:, 1] < h)
    exp = np.full(500, nm.UNREACHED, np.uint32)
    exp[inside] = got[q[inside, 1], q[inside, 0]]
    assert np.array_equal(nf.gather(q), exp)
    # paths from 300 starts, some of them off the grid, poses compared as bytes
    starts, tuples = [], []
    for i in range(300):
        x, y = rng.uniform(-1.5, w + 1.5), rng.uniform(-1.5, h + 1.5)
        t = (777 + i, np.float32(float(m["origin"][0]) + x * float(m["mpc"])), np.float32(float(m["origin"][1]) + y * float(m["mpc"])),
             np.float32(rng.uniform(-3, 3)))
        tuples.append(t)
        starts.append(bl.make_pose(t[1], t[2], t[3], utime=t[0]))
    cap = 2048
    (buf, lens), labels, costs = nf.paths(starts, cap_each=cap, raw=True)
    cache = nm.descend_cache(l1, trav, pen, goals, p.reach_cells)
    longest = 0
    for i, t in enumerate(tuples):
        poses, label, cost = nm.descend(field, l1, trav, pen, goals, p.reach_cells, t, m["origin"], m["mpc"], CPM, _cache=cache)
        assert lens[i] == len(poses) and labels[i] == label and costs[i] == cost, (case, i, lens[i], len(poses), labels[i], label, costs[i], cost)
        assert len(poses) <= cap
        a, b = buf[i, :lens[i]], poses
        for k in ("utime", "x", "y", "theta"):
            assert a[k].tobytes() == b[k].tobytes(), (case, i, k)
        longest = max(longest, len(poses))
    if (field != nm.UNREACHED).sum() > 2000:
        assert longest > 1


def test_goals_off_grid_blocked_or_duplicated(maps, gpu_ctx, nf):
    name = "obstacle_slam_10mx10m_5cm"
    d = _dist(name, maps, gpu_ctx)
    l1 = cpu._l1(name)
    p = nm.Params(0.2, 2.0, 1.0)
    trav, pen = nm.tables(nm.dist_table(200, 200), p)
    tcell, _ = nm.cell_tables(l1, trav, pen)
    wall = tuple(int(v) for v in np.argwhere(~tcell)[0][::-1])
    free = cpu.cases()[name + "_far"][2][0]
    for goals in ([(-1, 0), (200, 5), (7, 200), (10 ** 6, -10 ** 6)], [wall], [wall, free, free, (300, 300), free], []):
        nf.compute(d, _c_params(p), goals)
        assert np.array_equal(nf.cells(), nm.dijkstra(l1, trav, pen, goals, 0)), goals
        paths, labels, costs = nf.paths([bl.make_pose(-0.75, 0.2, 0.0)])
        exp = nm.descend(nm.dijkstra(l1, trav, pen, goals, 0), l1, trav, pen, goals, 0, (0, -0.75, 0.2, 0.0), maps[name]["origin"], maps[name]["mpc"], CPM)
        assert len(paths[0]) == len(exp[0]) and labels[0] == exp[1] and costs[0] == exp[2]
        if len(goals) == 5:
            assert labels[0] == 1 and len(paths[0]) > 1      # the lowest index that covers the goal cell: the blocked goal is skipped


def test_compute_to_pose_and_bad_arguments(maps, gpu_ctx, nf):
    name = "obstacle_slam_10mx10m_5cm"
    m = maps[name]
    d = _dist(name, maps, gpu_ctx)
    l1, trav, pen, goals, p, field = cpu.solved(name)
    nf.computeToPose(d, _c_params(p), bl.make_pose(-0.35, 0.2, 1.0))
    assert np.array_equal(nf.cells(), field)
    nf.computeToPose(d, _c_params(p), bl.make_pose(40.0, 0.2, 1.0))                        # off the grid: nothing is reached
    assert (nf.cells() == nm.UNREACHED).all()
    for bad in (nm.Params(0.2, 2.0, 1.0, obstacle_gain=4096), nm.Params(0.2, 2.0, 1.0, obstacle_gain=-1), nm.Params(0.2, 2.0, 1.0, reach_cells=-1),
                nm.Params(0.2, 2.0, -1.0), nm.Params(0.2, 2.0, float("nan"))):
        rc = gpu_ctx.lib.bl_navfield_compute(nf.h, d.h, C.byref(_c_params(bad)), None, 0)
        assert rc == _capi.BL_ERR_ARG, vars(bad)
    fresh = bl.NavigationField(gpu_ctx)
    out = np.zeros(4, np.uint32)
    assert gpu_ctx.lib.bl_navfield_download(fresh.h, out.ctypes.data) == _capi.BL_ERR_STATE      # nothing computed yet
    assert gpu_ctx.lib.bl_navfield_compute(fresh.h, bl.ObstacleDistanceGrid(ctx=gpu_ctx).h, C.byref(_c_params(p)), None, 0) == _capi.BL_ERR_ARG
    fresh.close()


def test_recompute_leaves_no_stale_tiles(maps, gpu_ctx):
    """Other goals on the same handle, then the same handle after bl_dist_set_distances on a changed map (and a smaller one)."""
    name = "astar_maze"
    m = maps[name]
    p = nm.Params(0.1, 1.0, 1.0)
    cp = _c_params(p)
    g = bl.OccupancyGrid.from_cells(m["cells"], m["origin"], m["mpc"], cellsPerMeter=CPM, ctx=gpu_ctx)
    d = bl.ObstacleDistanceGrid(ctx=gpu_ctx)
    d.setDistances(g)
    f = bl.NavigationField(gpu_ctx)
    l1 = cpu._l1(name)
    trav, pen = nm.tables(nm.dist_table(200, 200), p)
    ga, gb = [cpu.cases()[name][2][0]], cpu._spread_cells(l1, trav, 3, 9)
    for goals in (ga, gb, ga):
        f.compute(d, cp, goals)
        assert np.array_equal(f.cells(), nm.dijkstra(l1, trav, pen, goals, 0))
    cells2 = m["cells"].copy()
    cells2[60:140, 100] = 100                                # a new wall across the middle
    cells2[95:105, 100] = m["cells"][95:105, 100]
    g.upload(cells2)
    d.setDistances(g)
    l1b = nm.l1_distances(cells2)
    f.compute(d, cp, ga)
    assert np.array_equal(f.cells(), nm.dijkstra(l1b, trav, pen, ga, 0))
    small = cpu.ragged_cells()
    g2 = bl.OccupancyGrid.from_cells(small, (-4.0, -5.0), 0.05, cellsPerMeter=CPM, ctx=gpu_ctx)
    d.setDistances(g2)
    l1c = cpu._l1("ragged")
    tr2, pe2 = nm.tables(nm.dist_table(173, 211), p)
    goals = cpu.cases()["ragged"][2]
    f.compute(d, cp, goals)
    assert f.shape() == (173, 211) and np.array_equal(f.cells(), nm.dijkstra(l1c, tr2, pe2, goals, 0))
    f.close()


def _large_case(gpu_ctx, cells, p, goals, nstarts, seed):
    h, w = cells.shape
    origin, mpc = (np.float32(-50.0), np.float32(-50.0)), np.float32(0.05)
    g = bl.OccupancyGrid.from_cells(cells, origin, mpc, cellsPerMeter=CPM, ctx=gpu_ctx)
    d = bl.ObstacleDistanceGrid(ctx=gpu_ctx)
    d.setDistances(g)
    l1 = nm.l1_distances(cells)
    f = nm.dist_table(w, h)
    assert np.array_equal(d.cells().view(np.uint32), np.where(l1 == nm.NONE16, np.float32(-1.0), f[np.minimum(l1, len(f) - 1)]).view(np.uint32))
    trav, pen = nm.tables(f, p)
    nf = bl.NavigationField(gpu_ctx)
    nf.compute(d, _c_params(p), goals)
    field = nf.cells()
    why = nm.certificate(field, l1, trav, pen, goals, p.reach_cells)
    assert why is None, why
    st = nf.stats()
    print("%d x %d: %s" % (w, h, st))
    assert st["rounds"] <= st["traversable"] + 1 and st["reached"] == int((field != nm.UNREACHED).sum()) and st["reached"] > w * h // 4
    cache = nm.descend_cache(l1, trav, pen, goals, p.reach_cells)
    pcell = nm.cell_tables(l1, trav, pen)[1]
    ys, xs = np.nonzero(field != nm.UNREACHED)
    rng = np.random.default_rng(seed)
    pick = rng.choice(len(xs), nstarts, replace=False)
    starts = [bl.make_pose(float(origin[0]) + (xs[i] + 0.5) * float(mpc), float(origin[1]) + (ys[i] + 0.5) * float(mpc), 0.1 * k, utime=k)
              for k, i in enumerate(pick)]
    cap = 8192
    (buf, lens), labels, costs = nf.paths(starts, cap_each=cap, raw=True)
    checked = 0
    for k in range(nstarts):
        assert lens[k] >= 1 and costs[k] == field[ys[pick[k]], xs[pick[k]]]
        if lens[k] > cap:
            continue
        cpu.check_path_properties(buf[k, :lens[k]], int(labels[k]), int(costs[k]), field, l1, trav, pen, goals, p.reach_cells, origin, mpc, cache=cache,
                                  pcell=pcell)
        checked += 1
    assert checked >= nstarts * 3 // 4, checked
    gain_too_high = _c_params(nm.Params(p.minDistanceToObstacle, p.maxDistanceWithCost, 1.0, obstacle_gain=4095))
    if w * h * (14 + 4095) > 2 ** 32 - 2:
        g32 = np.array(goals, np.int32)
        assert gpu_ctx.lib.bl_navfield_compute(nf.h, d.h, C.byref(gain_too_high), g32.ctypes.data, len(g32)) == _capi.BL_ERR_ARG
    nf.close()
    d.close()
    g.close()


def test_large_tiled_maze_2000(maps, gpu_ctx):
    world = synth.tile_world(maps["astar_maze"]["cells"], 2000)
    p = nm.Params(0.1, 1.0, 1.0)
    l1 = nm.l1_distances(world)
    trav, _ = nm.tables(nm.dist_table(2000, 2000), p)
    _large_case(gpu_ctx, world, p, [cpu._far_cell(l1, trav)], 1000, 21)


def test_large_grid_width_not_a_multiple_of_the_tile(maps, gpu_ctx):
    world = synth.tile_world(maps["astar_convex"]["cells"], 1530)[:1333, :1501].copy()
    world[-1, :] = 127
    world[:, -1] = 127
    p = nm.Params(0.2, 2.0, 2.0, obstacle_gain=200, reach_cells=2)
    l1 = nm.l1_distances(world)
    trav, _ = nm.tables(nm.dist_table(1501, 1333), p)
    goals = cpu._spread_cells(l1, trav, 4, 5) + [(-7, 3)]
    _large_case(gpu_ctx, world, p, goals, 1000, 22)
