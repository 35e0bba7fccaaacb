"""Path shortcutting on the GPU (bl_shortcut_*, botlab_amd/csrc/bl_shortcut.hip) against its model (tests/path_shortcut_model.py):
kept indices, counts, both costs and, where m <= 512, the matrix of edges, all byte for byte.  The input paths are built on the CPU;
the only device objects are the grid, its distance grid and the shortcut handle."""
import numpy as np
import pytest

import botlab_amd as bl
import helpers
import nav_field_model as nm
import path_shortcut_model as psm
import test_path_shortcut_model_cpu as cpu

pytestmark = pytest.mark.gpu
CPM = helpers.CPM_DEFAULT
_dev = {}


def _dist(world, ctx):
    """The distance grid of a model world on the device, once per world."""
    key = id(world)
    if key not in _dev:
        g = bl.OccupancyGrid.from_cells(world.cells, world.origin, world.mpc, cellsPerMeter=CPM, ctx=ctx)
        d = bl.ObstacleDistanceGrid(ctx=ctx)
        d.setDistances(g)
        _dev[key] = (d, g, world)
    return _dev[key][0]


@pytest.fixture(scope="module")
def sc(gpu_ctx):
    s = bl.PathShortcut(gpu_ctx)
    yield s
    s.close()


def _compare(sc, ctx, world, p, paths, matrix=True):
    """Everything the device hands back for `paths` against the model; returns the model's (keep, cost, input cost) per path."""
    d = _dist(world, ctx)
    okc = world.ok(p.clearance)
    sc.set_params(p.clearance, p.max_span, p.waypoint_cost)
    keeps, costs = sc.cells(d, paths)
    staged = all(psm.window_staged(q) for q in paths)
    assert sc.debugPath() == (0 if staged else 1)
    out = []
    for k, q in enumerate(paths):
        ek, ec, ei = psm.shortcut(okc, q, p)
        out.append((ek, ec, ei))
        assert keeps[k].dtype == np.int32 and keeps[k].tobytes() == ek.tobytes(), (k, len(q), keeps[k][:8], ek[:8])
        assert (int(costs[k, 0]), int(costs[k, 1])) == (ec, ei), (k, costs[k], ec, ei)
        if matrix and len(q) <= 512:
            got = sc.visible(d, q)
            assert sc.debugPath() == (0 if psm.window_staged(q) else 1)
            exp = psm.visible_matrix(okc, q, p.max_span)
            bad = np.argwhere(got != exp)
            assert len(bad) == 0, (k, len(bad), bad[0])
    return out


# ---------------------------------------------------------------------------------------------------------------- lengths and spans
@pytest.mark.parametrize("m", [0, 1, 2, 3, 63, 64, 65, 511, 512])
def test_path_lengths_and_spans_on_the_ragged_grid(gpu_ctx, sc, m):
    world = cpu.ragged_world()
    assert (world.h, world.w) == (117, 203)
    q = cpu.walk(np.random.default_rng(100 + m), world.w, world.h, m, turn=0.1)
    res = []
    for span in sorted({1, 2, 63, 64, 65, max(m, 1)}):
        r = _compare(sc, gpu_ctx, world, psm.Params(0.2, span, 1024), [q], matrix=span in (2, 64, max(m, 1)))
        res.append(len(r[0][0]))
        if span == 1:
            assert r[0][0].tolist() == list(range(m))
    print("m", m, "kept per span", res)
    assert m < 63 or res[-1] < m


@pytest.mark.parametrize("wc", [0, 1024, 1048576])
def test_waypoint_costs_and_ties(gpu_ctx, sc, wc):
    world = cpu.room_world()
    rng = np.random.default_rng(7)
    corridor = cpu.line((10, 50), (60, 50))
    r = _compare(sc, gpu_ctx, world, psm.Params(0.2, 16, wc), [corridor, cpu.walk(rng, world.w, world.h, 200), cpu.polyline([(20, 20), (180, 30), (170, 180)])])
    if wc == 0:
        assert r[0][0].tolist() == [0, 2, 18, 34, 50]                # every chain costs the same: each step to the smallest i in reach
    else:
        assert len(r[0][0]) == 5                                     # 50 steps at spans of 16: four segments at the least


def test_serpentine_of_8192_cells_and_one_too_many(gpu_ctx, sc):
    world = cpu.room_world()
    q = cpu.serpentine(world.w, world.h, 8192)
    r = _compare(sc, gpu_ctx, world, psm.Params(0.2, 64, 1024), [q])
    assert 8192 // 64 <= len(r[0][0]) < 1000 and sc.lastDeviceMs()[0] > 0
    with pytest.raises(bl.BotlabHipError, match="status 2"):
        sc.cells(_dist(world, gpu_ctx), [cpu.serpentine(world.w, world.h, 8193)])


# ---------------------------------------------------------------------------------------------------------------- both window paths
def test_window_in_lds_and_grids_read_directly(gpu_ctx, sc):
    world = cpu.large_world()
    assert (world.h, world.w) == (752, 1008)
    rng = np.random.default_rng(3)
    big = cpu.polyline([(10, 10), (739, 400), (300, 739), (739, 739)])          # bounding box 730 x 730: 92 B x 730 > 64 KiB
    assert not psm.window_staged(big) and len(big) <= psm.MAX_POINTS
    _compare(sc, gpu_ctx, world, psm.Params(0.2, 96, 1024), [big])
    assert sc.debugPath() == 1
    inner = cpu.walk(rng, world.w, world.h, 300, start=(500, 300))
    _compare(sc, gpu_ctx, world, psm.Params(0.2, 96, 1024), [inner])
    assert sc.debugPath() == 0
    mixed = [inner, big, cpu.walk(rng, world.w, world.h, 50)]                  # one wide path: the whole call reads the grids
    assert [psm.window_staged(q) for q in mixed] == [True, False, True]
    _compare(sc, gpu_ctx, world, psm.Params(0.2, 40, 1024), mixed, matrix=False)
    assert sc.debugPath() == 1
    # one box just on either side of the limit: 512 x 715 cells is 64 B x 715 = 45 760, 1008 x 512 is 128 B x 512 = 65 536 exactly,
    # 1008 x 513 one row more
    at = cpu.polyline([(0, 100), (1007, 300), (0, 611)])
    over = cpu.polyline([(0, 100), (1007, 300), (0, 612)])
    assert psm.window_staged(at) and not psm.window_staged(over)
    for q, path in ((at, 0), (over, 1)):
        _compare(sc, gpu_ctx, world, psm.Params(0.3, 33, 512), [q], matrix=False)
        assert sc.debugPath() == path
        assert (sc.visible(_dist(world, gpu_ctx), q[-400:]) == psm.visible_matrix(world.ok(0.3), q[-400:], 33)).all()


# ---------------------------------------------------------------------------------------------------------------- geometry
def test_borders_axes_diagonals_and_repeated_cells(gpu_ctx, sc):
    world = cpu.ragged_world()
    w, h = world.w, world.h
    border = cpu.polyline([(0, 0), (w - 1, 0), (w - 1, h - 1), (0, h - 1), (0, 1)])           # y = 0, x = W - 1, y = H - 1, x = 0
    diag = cpu.polyline([(5, 5), (100, 100), (195, 5), (110, 90)])                           # |DX| == |DY|: corner crossings
    rng = np.random.default_rng(9)
    rep = np.repeat(cpu.walk(rng, w, h, 60), rng.integers(1, 4, 60), axis=0)                   # repeated cells
    stand = np.tile(np.array([[40, 40]], np.int32), (20, 1))                                   # one cell twenty times
    jumps = rng.integers(0, (w, h), (120, 2)).astype(np.int32)                                 # steps of any size and direction
    for clearance in (0.2, 0.0, -1.0):                                                         # n >= 3, n >= 1, every cell with a distance
        _compare(sc, gpu_ctx, world, psm.Params(clearance, 48, 300), [border[:512], diag, rep, stand, jumps])
    _compare(sc, gpu_ctx, world, psm.Params(0.2, 8192, 0), [border[-300:], stand])


def test_strip_crossed_end_to_end(gpu_ctx, sc):
    world = cpu.strip_world()
    assert (world.h, world.w) == (24, 4000)
    q = np.array([(0, 20), (3999, 21), (3999, 23), (0, 22), (1, 22), (3998, 1)], np.int32)      # the largest L: 3999 cells and a bit
    r = _compare(sc, gpu_ctx, world, psm.Params(0.2, 8, 0), [q, cpu.line((0, 12), (3999, 12))])
    assert r[0][2] >= 2 * psm.length(3999, 1) and len(r[1][0]) == 501


def test_map_without_an_occupied_cell_is_the_identity(gpu_ctx, sc):
    world = cpu.empty_world()
    assert not world.ok(-1.0).any()
    q = cpu.walk(np.random.default_rng(2), world.w, world.h, 90)
    r = _compare(sc, gpu_ctx, world, psm.Params(-1.0, 64, 1024), [q])
    assert r[0][0].tolist() == list(range(90)) and r[0][1] == r[0][2]


@pytest.mark.parametrize("P", [1, 2, 300])
def test_many_paths_of_mixed_lengths_in_one_call(gpu_ctx, sc, P):
    world = cpu.ragged_world()
    rng = np.random.default_rng(40 + P)
    lens = [int(v) for v in rng.integers(2, 31, P)]
    for k, v in ((0, 0), (1, 1), (7, 0), (8, 1), (299, 1)):
        if k < P and P > 2:
            lens[k] = v
    paths = [cpu.walk(rng, world.w, world.h, n, turn=0.15) for n in lens]
    r = _compare(sc, gpu_ctx, world, psm.Params(0.2, 6, 700), paths, matrix=False)
    assert P < 300 or sum(len(k) for k, _, _ in r) < sum(lens)
    keeps, costs = sc.cells(_dist(world, gpu_ctx), [])
    assert keeps == [] and costs.shape == (0, 2)


# ---------------------------------------------------------------------------------------------------------------- poses
def test_poses_on_the_obstacle_map(gpu_ctx, sc, maps):
    world, poses = cpu.map_case(maps)
    d = _dist(world, gpu_ctx)
    p = psm.Params(0.2, 64, 1024)
    sc.set_params(p.clearance, p.max_span, p.waypoint_cost)
    exp, ec, ei = psm.shortcut_poses(world.ok(0.2), poses, world.origin, CPM, p)
    path = [bl.Pose(int(q["utime"]), float(q["x"]), float(q["y"]), float(q["theta"])) for q in poses]
    got, cost = sc.shortcut(d, path, return_cost=True)
    assert len(got) == len(exp) < len(poses) and (int(cost[0]), int(cost[1])) == (ec, ei)
    for k in range(len(exp)):
        assert bytes(got[k]) == exp[k].tobytes()[:24], (k, got[k], exp[k])
    many, costs = sc.poses(d, [path, path[:1], [], path[5:40]])
    assert [bytes(q) for q in many[0]] == [bytes(q) for q in got] and len(many[1]) == 1 and many[2] == [] and bytes(many[1][0]) == bytes(path[0])
    e3, c3, i3 = psm.shortcut_poses(world.ok(0.2), poses[5:40], world.origin, CPM, p)
    assert [bytes(q) for q in many[3]] == [e3[k].tobytes()[:24] for k in range(len(e3))] and (int(costs[3, 0]), int(costs[3, 1])) == (c3, i3)
    off = list(path)
    off[3] = bl.make_pose(1e6, 0.0, 0.0)
    with pytest.raises(bl.BotlabHipError, match="status 2"):
        sc.shortcut(d, off)
    planner = bl.MotionPlanner(ctx=gpu_ctx)
    planner.distances_ = d
    assert [bytes(q) for q in planner.shortcutPath(path, 0.2, 64, 1024)] == [bytes(q) for q in got]


# ---------------------------------------------------------------------------------------------------------------- errors
def test_error_returns(gpu_ctx):
    world = cpu.empty_world()
    d = _dist(world, gpu_ctx)
    q = cpu.line((1, 1), (30, 20))
    fresh = bl.PathShortcut(gpu_ctx)
    try:
        assert fresh.debugPath() == -1
        for call in (lambda: fresh.cells(d, [q]), lambda: fresh.visible(d, q), lambda: fresh.lastDeviceMs()):
            with pytest.raises(bl.BotlabHipError, match="status 4"):                  # before set_params: BL_ERR_STATE
                call()
        for bad in (dict(clearance=float("nan")), dict(clearance=float("inf")), dict(max_span=0), dict(max_span=8193), dict(waypoint_cost=-1),
                    dict(waypoint_cost=1048577)):
            with pytest.raises(bl.BotlabHipError, match="status 2"):
                fresh.set_params(**dict(dict(clearance=0.2, max_span=64, waypoint_cost=0), **bad))
        assert fresh.params is None
        fresh.set_params(0.2, 8192, 1048576)
        with pytest.raises(bl.BotlabHipError, match="status 2"):
            fresh.set_params(0.2, 8193, 0)
        keeps, costs = fresh.cells(d, [q])                                            # the refused call left the parameters alone
        assert keeps[0].tolist() == list(range(len(q))) and int(costs[0, 0]) == int(costs[0, 1]) > 1048576 * (len(q) - 1)
        for bad in ([(0, 0), (-1, 0)], [(0, 0), (world.w, 0)], [(0, world.h)], [(0, -1), (0, 0)]):
            with pytest.raises(bl.BotlabHipError, match="status 2"):
                fresh.cells(d, [q, np.array(bad, np.int32)])
            with pytest.raises(bl.BotlabHipError, match="status 2"):
                fresh.visible(d, np.array(bad, np.int32))
        with pytest.raises(bl.BotlabHipError, match="status 2"):
            fresh.visible(d, np.zeros((513, 2), np.int32))
        with pytest.raises(bl.BotlabHipError, match="status 2"):
            fresh.cells(d, [q[:2]] * 4097)
        unset = bl.ObstacleDistanceGrid(ctx=gpu_ctx)
        with pytest.raises(bl.BotlabHipError, match="status 2"):                      # a distance grid never transformed
            fresh.cells(unset, [q])
        assert fresh.lastDeviceMs()[0] > 0
    finally:
        fresh.close()
