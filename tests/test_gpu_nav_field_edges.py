"""The navigation field (bl_navfield_*, botlab_amd/csrc/bl_navfield.hip) on the hand-built grids of tests/nav_field_cases.py: the
second tile of a workgroup, grids of one tile and less, the corner rule across a tile corner, more than a hundred rounds, paths
longer than the caller's buffer, start poses at the grid's low edge, and the limits of the arguments.  The reference is the model's
Dijkstra, bit for bit; on the 1.08 M-cell grid, where that is too slow for the suite, the model's Bellman certificate, which only
the solution passes.  tests/test_nav_field_cases_cpu.py shows that each case is what it claims to be."""
import ctypes as C

import numpy as np
import pytest

import botlab_amd as bl
from botlab_amd import _capi
import nav_field_cases as nc
import nav_field_model as nm

pytestmark = pytest.mark.gpu
FIELDS = ("utime", "x", "y", "theta")


def _c_params(p):
    return _capi.NavFieldParams(p.minDistanceToObstacle, p.maxDistanceWithCost, p.distanceCostExponent, p.obstacle_gain, p.reach_cells)


_dists = {}


def _dist(world_name, ctx):
    """One device distance grid per world for the whole module; its floats are the model's f[n(c)]."""
    if world_name not in _dists:
        w = nc.world(world_name)
        g = bl.OccupancyGrid.from_cells(w.cells, w.origin, nc.MPC, cellsPerMeter=nc.CPM, ctx=ctx)
        d = bl.ObstacleDistanceGrid(ctx=ctx)
        d.setDistances(g)
        assert np.array_equal(d.cells().view(np.uint32), nc.expected_floats(world_name).view(np.uint32)), world_name
        _dists[world_name] = (g, d)
    return _dists[world_name][1]


@pytest.fixture(scope="module")
def nf(gpu_ctx):
    f = bl.NavigationField(gpu_ctx)
    yield f
    f.close()


def _poses(starts):
    return [bl.make_pose(s[1], s[2], s[3], utime=s[0]) for s in starts]


def _compute_and_check_field(nf, ctx, name):
    """compute the case; field and counts equal the model's.  Returns the device's field and its stats."""
    c = nc.case(name)
    l1, trav, pen, goals, p, field = nc.solved(name)
    nf.compute(_dist(c.world, ctx), _c_params(p), goals)
    got = nf.cells()
    assert got.dtype == np.uint32 and got.shape == field.shape and np.array_equal(got, field), (name, int((got != field).sum()))
    st = nf.stats()
    tcell, _ = nm.cell_tables(l1, trav, pen)
    mask, _ = nm.goal_set(tcell, goals, p.reach_cells)
    assert st["traversable"] == int(tcell.sum()) and st["reached"] == int((field != nm.UNREACHED).sum()) and st["goal_set"] == int(mask.sum()), (name, st)
    assert st["rounds"] <= st["traversable"] + 1
    return got, st


def _check_paths(nf, name, cap):
    """the paths from the case's starts equal the model's descents: poses as bytes, length, label, cost"""
    c = nc.case(name)
    (buf, lens), labels, costs = nf.paths(_poses(c.starts), cap_each=cap, raw=True)
    model = nc.model_paths(name)
    assert len(model) == len(c.starts) == len(lens)
    for i, (poses, label, cost) in enumerate(model):
        assert lens[i] == len(poses) and labels[i] == label and costs[i] == cost, (name, i, lens[i], len(poses), labels[i], label, costs[i], cost)
        assert len(poses) <= cap
        for k in FIELDS:
            assert buf[i, :lens[i]][k].tobytes() == poses[k].tobytes(), (name, i, k)
    return model


def test_small_grids_on_one_handle(gpu_ctx, nf):
    """Every shape in turn on ONE handle, shrinking and growing, and 33 x 33 once more at the end: nothing of a larger grid is left."""
    for h, w in nc.SMALL_SHAPES + [(33, 33)]:
        name = nc.small_name(h, w)
        got, st = _compute_and_check_field(nf, gpu_ctx, name)
        assert nf.shape() == (w, h)
        print(name, st)
        ring = [(x, y) for y in range(-1, h + 1) for x in range(-1, w + 1)]              # every cell and the cells just off the grid
        q = np.array(ring, np.int32)
        inside = (q[:, 0] >= 0) & (q[:, 0] < w) & (q[:, 1] >= 0) & (q[:, 1] < h)
        assert int((~inside).sum()) == 2 * (w + h) + 4
        exp = np.full(len(q), nm.UNREACHED, np.uint32)
        exp[inside] = got[q[inside, 1], q[inside, 0]]
        assert np.array_equal(nf.gather(q), exp), name
        if nc.case(name).starts:
            _check_paths(nf, name, 128)
        if (h, w) == (1, 1):
            assert (got == nm.UNREACHED).all() and st["reached"] == 0 and st["goal_set"] == 0
            paths, labels, costs = nf.paths([bl.make_pose(*[float(v) for v in nc.pose_at(nc.ORIGIN, 0.5, 0.5)[1:3]], 0.0)])
            assert len(paths[0]) == 1 and labels[0] == -1 and costs[0] == nm.UNREACHED


@pytest.mark.parametrize("size,cx,cy", [(s, cx, cy) for s in sorted(nc.CORNERS) for cx, cy in nc.CORNERS[s]])
def test_corner_rule_across_a_tile_corner(gpu_ctx, nf, size, cx, cy):
    for d in range(4):
        k = nc.corner_cells(cx, cy, d)
        for pattern in nc.PATTERNS:
            name = nc.corner_name(size, cx, cy, d, pattern)
            _compute_and_check_field(nf, gpu_ctx, name)
            (poses, _, _), = _check_paths(nf, name, 64)
            assert (nc.path_moves(poses)[0] == k["d"]) == (pattern == "open")           # (the model's move, which the device's equals)


@pytest.fixture(scope="module")
def big(gpu_ctx):
    c = nc.case("big")
    trav, pen = nc.tables("big", c.params)
    return _dist("big", gpu_ctx), nc.l1("big"), trav, pen, c.goals, c.params


def test_more_tiles_than_workgroups(gpu_ctx, nf, big):
    """1056 tiles listed for round 1, 1024 workgroups: 32 of them take a second tile."""
    d, l1, trav, pen, goals, p = big
    nf.compute(d, _c_params(p), goals)
    field = nf.cells()
    why = nm.certificate(field, l1, trav, pen, goals, 0)
    assert why is None, why
    st = nf.stats()
    print("big:", st)
    tcell, _ = nm.cell_tables(l1, trav, pen)
    assert st["goal_set"] == 1056 and st["reached"] == int((field != nm.UNREACHED).sum()) and st["traversable"] == int(tcell.sum())
    assert st["rounds"] <= st["traversable"] + 1
    nf.compute(d, _c_params(p), goals[::-1])                                             # the same goal set, listed the other way round
    assert np.array_equal(nf.cells(), field)


def test_guard_edge_on_the_big_grid(gpu_ctx, nf, big):
    """1081344 cells: obstacle_gain 3957 is the last one whose costs cannot wrap, 3958 is refused and leaves no field."""
    d, l1, _, _, goals, _ = big
    e = nc.case("big_gain_edge")
    assert e.params.obstacle_gain == nc.GAIN_LAST_OK and e.params.distanceCostExponent == 0.0
    trav, pen = nc.tables("big", e.params)
    nf.compute(d, _c_params(e.params), goals)
    field = nf.cells()
    why = nm.certificate(field, l1, trav, pen, goals, 0)
    assert why is None, why
    st = nf.stats()
    print("big, gain %d:" % nc.GAIN_LAST_OK, st, "largest value", int(field[field != nm.UNREACHED].max()))
    assert st["goal_set"] == 1056 and st["reached"] == int((field != nm.UNREACHED).sum())
    over = nm.Params(0.05, 0.45, 0.0, obstacle_gain=nc.GAIN_LAST_OK + 1)
    g32 = np.array(goals, np.int32)
    lib = gpu_ctx.lib
    assert lib.bl_navfield_compute(nf.h, d.h, C.byref(_c_params(over)), g32.ctypes.data, len(g32)) == _capi.BL_ERR_ARG
    out = np.zeros(4, np.uint32)
    assert lib.bl_navfield_download(nf.h, out.ctypes.data) == _capi.BL_ERR_STATE         # the refused compute left the handle not computed
    assert not out.any()


@pytest.mark.parametrize("name", ["strip", "strip_t"])
def test_strip_needs_more_rounds_than_the_growing_groups(gpu_ctx, nf, name):
    """131 tiles in a line, the goal in the first: the last cannot be listed before round 130, which is past the groups of 4, 8, 16,
    32 and 64 rounds (124 in all), in a second group of 64."""
    got, st = _compute_and_check_field(nf, gpu_ctx, name)
    print(name, st)
    assert 130 <= st["rounds"] <= st["traversable"] + 1


def test_serpentine(gpu_ctx, nf):
    got, st = _compute_and_check_field(nf, gpu_ctx, "serpentine")
    print("serpentine", st)
    model = _check_paths(nf, "serpentine", 2048)
    poses = model[nc.FAR_START][0]
    assert len(poses) == 2015 and all(dx == 0 or dy == 0 for dx, dy in nc.path_moves(poses))


def _raw_paths(ctx, nf, starts, cap, fill=0xA5):
    """bl_navfield_paths into buffers filled with a pattern: (bytes of the pose buffer as (n, cap, 24), lens, labels, costs)"""
    n = len(starts)
    s = (_capi.Pose * max(n, 1))(*starts)
    buf = np.full((max(n, 1), cap, bl.POSE_DTYPE.itemsize), fill, np.uint8)
    lens = np.full(max(n, 1), -77, np.int32)
    labels = np.full(max(n, 1), -77, np.int32)
    costs = np.full(max(n, 1), 77, np.uint32)
    rc = ctx.lib.bl_navfield_paths(nf.h, s, n, buf.ctypes.data, cap, lens.ctypes.data, labels.ctypes.data, costs.ctypes.data)
    return rc, buf, lens, labels, costs


@pytest.mark.parametrize("name", ["strip", "serpentine"])
def test_paths_longer_than_the_buffer(gpu_ctx, nf, name):
    """70 starts at once, one of them L poses from the goal: at every cap_each the lengths, labels and costs are the whole path's, the
    first min(L, cap) poses the model's, and the caller's slots behind them untouched."""
    _compute_and_check_field(nf, gpu_ctx, name)
    c = nc.case(name)
    model = nc.model_paths(name)
    starts = _poses(c.starts)
    L = len(model[nc.FAR_START][0])
    for cap in (1, 2, L - 1, L, L + 1):
        rc, buf, lens, labels, costs = _raw_paths(gpu_ctx, nf, starts, cap)
        assert rc == _capi.BL_OK
        cut = 0
        for i, (poses, label, cost) in enumerate(model):
            assert lens[i] == len(poses) and labels[i] == label and costs[i] == cost, (name, cap, i, lens[i], len(poses))
            kept = min(len(poses), cap)
            got = buf[i, :kept].reshape(-1).view(bl.POSE_DTYPE)
            for k in FIELDS:
                assert got[k].tobytes() == poses[:kept][k].tobytes(), (name, cap, i, k)
            assert (buf[i, kept:] == 0xA5).all(), (name, cap, i)
            cut += len(poses) > cap
        assert (cut > 0) == (cap < L) and (cap > 2 or cut >= 60)
        assert lens[nc.FAR_START] == L


def test_start_poses_at_the_low_edge(gpu_ctx, nf):
    _compute_and_check_field(nf, gpu_ctx, "edge_starts")
    model = _check_paths(nf, "edge_starts", 128)
    for (_, want), (poses, label, cost) in zip(nc.EDGE_STARTS, model):
        if want is None or want == (20, 20):
            assert len(poses) == 1 and label == -1 and cost == nm.UNREACHED
        else:
            assert len(poses) > 1 and label == 0


def test_reach_and_the_remaining_arguments(gpu_ctx, nf):
    lib = gpu_ctx.lib
    d = _dist("open40", gpu_ctx)
    # reach 1024: every window covers the whole grid
    got, st = _compute_and_check_field(nf, gpu_ctx, "reach_all")
    assert st["goal_set"] == st["traversable"] == 1599 and int(got[20, 20]) == nm.UNREACHED and (np.delete(got.ravel(), 20 * 40 + 20) == 0).all()
    c = nc.case("reach_all")
    (buf, lens), labels, costs = nf.paths(_poses(c.starts), cap_each=4, raw=True)
    on_source = np.arange(1600) == 20 * 40 + 20
    assert (lens == 1).all() and (labels[~on_source] == 1).all() and labels[on_source] == -1      # (100, 100) is skipped; of (5, 5) and (6, 6) the lower index
    assert (costs[~on_source] == 0).all() and costs[on_source] == nm.UNREACHED
    _check_paths(nf, "reach_all", 4)
    # reach 1025 is refused
    g32 = np.array(c.goals, np.int32)
    too_far = nm.Params(0.05, 0.45, 1.0, obstacle_gain=50, reach_cells=1025)
    assert lib.bl_navfield_compute(nf.h, d.h, C.byref(_c_params(too_far)), g32.ctypes.data, len(g32)) == _capi.BL_ERR_ARG
    # reach 3 at two corners of the grid: clipped windows
    _compute_and_check_field(nf, gpu_ctx, "reach_clipped")
    _check_paths(nf, "reach_clipped", 128)
    # n == 0: nothing is written
    rc, buf, lens, labels, costs = _raw_paths(gpu_ctx, nf, [], 3)
    assert rc == _capi.BL_OK and (buf == 0xA5).all() and lens[0] == -77 and labels[0] == -77 and costs[0] == 77
    assert len(nf.paths([])[0]) == 0
    out = np.full(3, 77, np.uint32)
    q = np.zeros((1, 2), np.int32)
    assert lib.bl_navfield_gather(nf.h, q.ctypes.data, 0, out.ctypes.data) == _capi.BL_OK and (out == 77).all()
    assert lib.bl_navfield_gather(nf.h, None, 0, None) == _capi.BL_OK and len(nf.gather(np.zeros((0, 2), np.int32))) == 0


def test_paths_after_the_distance_grid_was_resized(gpu_ctx):
    """A field answers for its distance grid only until that grid is transformed to another size: BL_ERR_STATE."""
    w = nc.world("open40")
    g = bl.OccupancyGrid.from_cells(w.cells, w.origin, nc.MPC, cellsPerMeter=nc.CPM, ctx=gpu_ctx)
    d = bl.ObstacleDistanceGrid(ctx=gpu_ctx)
    d.setDistances(g)
    f = bl.NavigationField(gpu_ctx)
    c = nc.case("edge_starts")
    f.compute(d, _c_params(c.params), c.goals)
    start = [bl.make_pose(0.5, 0.5, 0.0)]
    rc, buf, lens, _, _ = _raw_paths(gpu_ctx, f, start, 128)
    assert rc == _capi.BL_OK and lens[0] > 1
    for other in ("small_33x33", "small_65x31"):                                          # a smaller grid, then a larger one
        w2 = nc.world(other)
        g2 = bl.OccupancyGrid.from_cells(w2.cells, w.origin, nc.MPC, cellsPerMeter=nc.CPM, ctx=gpu_ctx)
        d.setDistances(g2)
        rc, buf, lens, labels, costs = _raw_paths(gpu_ctx, f, start, 128)
        assert rc == _capi.BL_ERR_STATE and (buf == 0xA5).all() and lens[0] == -77, other
        g2.close()
    f.compute(d, _c_params(c.params), [(3, 3)])                                           # computed again, it answers again
    rc, buf, lens, _, _ = _raw_paths(gpu_ctx, f, start, 128)
    assert rc == _capi.BL_OK and lens[0] >= 1
    f.close()
    d.close()
    g.close()
