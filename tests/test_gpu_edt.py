"""The Euclidean distance grid on the GPU (bl_dist_create_euclidean, botlab_amd/csrc/bl_edt.hip) against its model (tests/edt_model.py):
every comparison is np.array_equal on the codes of bl_dist_download_codes, no tolerance and no cell left out."""
import ctypes as C

import numpy as np
import pytest

import botlab_amd as bl
from botlab_amd import _capi
import edt_model as em
import helpers
import nav_field_model as nm

pytestmark = pytest.mark.gpu
CPM = helpers.CPM_DEFAULT
ORIGIN = (np.float32(-5.0), np.float32(-5.0))


def _grid(ctx, cells, mpc=0.05):
    return bl.OccupancyGrid.from_cells(np.ascontiguousarray(cells, np.int8), ORIGIN, np.float32(mpc), cellsPerMeter=CPM, ctx=ctx)


def _codes(ctx, cells, R, mpc=0.05):
    g = _grid(ctx, cells, mpc)
    d = bl.ObstacleDistanceGrid(ctx=ctx, metric="euclidean", max_cells=R)
    d.setDistances(g)
    out = d.codes()
    d.close()
    g.close()
    return out


def _hip_runtime():
    """The HIP runtime this process already runs on (never a second one)."""
    with open("/proc/self/maps") as maps_file:
        for line in maps_file:
            if "libamdhip64" in line:
                return C.CDLL(line.split()[-1])
    raise AssertionError("no HIP runtime is loaded")


def _free(h, w):
    return np.full((h, w), -50, np.int8)


def _check(ctx, cells, R):
    got, exp = _codes(ctx, cells, R), em.codes(cells, R)
    assert got.dtype == np.uint16 and got.shape == exp.shape
    assert np.array_equal(got, exp), (cells.shape, R, int((got != exp).sum()), np.argwhere(got != exp)[:4].tolist())
    return got


@pytest.mark.parametrize("shape", [(1, 1), (1, 37), (37, 1), (63, 65), (130, 129)])
def test_small_and_tile_edge_shapes(gpu_ctx, shape):
    """(h, w): 1 x 1, 1 x 37, 37 x 1, 65 x 63 and 129 x 130 cells (width x height): none, all, corners, random."""
    h, w = shape
    rng = np.random.default_rng(h * 1000 + w)
    for R in (1, 3, 64, 254):
        none = _free(h, w)
        assert (_check(gpu_ctx, none, R) == em.NONE16).all()
        assert (_check(gpu_ctx, np.full((h, w), 100, np.int8), R) == 0).all()
        for cy, cx in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):
            c = none.copy()
            c[cy, cx] = 0                                                          # log-odds 0 is a source
            _check(gpu_ctx, c, R)
        for density in (0.001, 0.03, 0.5):
            _check(gpu_ctx, np.where(rng.random((h, w)) < density, 77, -3).astype(np.int8), R)


def test_golden_maps(maps, gpu_ctx):
    """All 14 golden maps (200 x 200 and 300 x 300) at R = 64."""
    sizes = set()
    for name in helpers.ALL_MAPS:
        cells = maps[name]["cells"]
        sizes.add(cells.shape)
        _check(gpu_ctx, cells, 64)
    assert len(helpers.ALL_MAPS) == 14 and sizes == {(200, 200), (300, 300)}


def test_single_source_disc(gpu_ctx):
    c = _free(300, 300)
    c[150, 150] = 100
    got = _check(gpu_ctx, c, 64)
    yy, xx = np.mgrid[0:300, 0:300]
    d2 = (yy - 150) ** 2 + (xx - 150) ** 2
    assert np.array_equal(got, np.where(d2 <= 64 * 64, d2, 64 * 64 + 1).astype(np.uint16))
    assert got[150, 214] == 4096 and got[150, 215] == 4097 and got[86, 150] == 4096 and got[85, 150] == 4097


def test_sparse_700_x_900_at_the_largest_cap(gpu_ctx):
    rng = np.random.default_rng(5)
    cells = np.where(rng.random((900, 700)) < 2e-4, 100, -50).astype(np.int8)
    got = _check(gpu_ctx, cells, 254)
    assert int(got.max()) > 64 * 64 and (got == 0).sum() == (cells >= 0).sum() > 50     # distances a smaller cap would have cut


def test_513_x_257_at_the_smallest_caps(gpu_ctx):
    rng = np.random.default_rng(6)
    cells = np.where(rng.random((257, 513)) < 0.01, 100, -50).astype(np.int8)
    for R in (1, 2, 3):
        got = _check(gpu_ctx, cells, R)
        assert int(got.max()) == R * R + 1


@pytest.mark.parametrize("R", [3, 64, 254])
def test_sources_exactly_at_and_one_past_the_halo(gpu_ctx, R):
    """A lone source R rows (columns) from a cell gives it R^2; R + 1 away gives FAR.  The cell rows (columns) sit at multiples of 64
    less one, plus nothing and plus one, so that whatever the tile height one of them has its source in the halo's last row."""
    n = 64 * 9 + 3
    for base in (64 * 4 - 1, 64 * 4, 64 * 4 + 1, 64 * 5 - 1, 64 * 5 + 1):
        for sign in (-1, 1):
            for gap in (R, R + 1):
                src = base + sign * gap
                assert 0 <= src < n
                for cells in (_free(n, 70), _free(70, n)):
                    rows = cells.shape[0] == n
                    if rows:
                        cells[src, 33] = 100
                    else:
                        cells[33, src] = 100
                    got = _check(gpu_ctx, cells, R)
                    at = got[base, 33] if rows else got[33, base]
                    assert at == (R * R if gap == R else R * R + 1), (R, base, sign, gap, rows)


def test_handle_life_source_word_and_sizes(maps, gpu_ctx):
    d = bl.ObstacleDistanceGrid(ctx=gpu_ctx, metric="euclidean", max_cells=64)
    assert d.metric() == ("euclidean", 64)
    with_src = maps["astar_maze"]["cells"]
    g = _grid(gpu_ctx, with_src)
    free = _grid(gpu_ctx, _free(200, 200))
    for grid, cells in ((g, with_src), (free, _free(200, 200)), (g, with_src)):      # a source word that is not reset shows in the second
        d.setDistances(grid)
        assert np.array_equal(d.codes(), em.codes(cells, 64))
    assert (em.codes(_free(200, 200), 64) == em.NONE16).all()
    big = maps["astar_narrow"]["cells"]
    assert big.shape == (300, 300)
    gb = _grid(gpu_ctx, big)
    d.setDistances(gb)                                                              # a larger map, then a smaller one
    assert d.shape() == big.shape[::-1] and np.array_equal(d.codes(), em.codes(big, 64))
    small = with_src[:57, :131].copy()
    gs = _grid(gpu_ctx, small)
    d.setDistances(gs)
    assert d.shape() == (131, 57) and np.array_equal(d.codes(), em.codes(small, 64))
    st = d.stats()
    assert st["full"] == 5 and st["incremental"] == 0 and st["unchanged"] == 0       # every call transforms the whole map
    assert d.bound()[0] is False
    d.forget()                                                                      # harmless
    d.setDistances(gs)
    assert np.array_equal(d.codes(), em.codes(small, 64)) and d.stats()["full"] == 6
    for x in (d, g, free, gb, gs):
        x.close()


@pytest.mark.parametrize("order", ["l1_first", "euclidean_first"])
def test_l1_and_euclidean_grids_on_one_map(maps, gpu_ctx, order):
    cells = maps["obstacle_slam_10mx10m_5cm"]["cells"]
    g = _grid(gpu_ctx, cells)
    l1 = bl.ObstacleDistanceGrid(ctx=gpu_ctx)
    eu = bl.ObstacleDistanceGrid(ctx=gpu_ctx, metric="euclidean", max_cells=64)
    for d in ((l1, eu) if order == "l1_first" else (eu, l1)):
        d.setDistances(g)
    assert l1.metric() == ("l1", 0)
    fresh = bl.ObstacleDistanceGrid(ctx=gpu_ctx)
    fresh.setDistances(g)
    assert l1.cells().tobytes() == fresh.cells().tobytes()
    assert np.array_equal(l1.codes(), nm.l1_distances(cells)) and np.array_equal(eu.codes(), em.codes(cells, 64))
    assert l1.table().tobytes() == nm.dist_table(200, 200).tobytes()                 # bl_dist_table of an L1 grid: width + height + 1
    for x in (l1, eu, fresh, g):
        x.close()


@pytest.mark.parametrize("mpc", [0.05, 0.1])
def test_float_view_and_table(maps, gpu_ctx, mpc):
    cells = maps["astar_narrow"]["cells"]
    h, w = cells.shape
    R = 20
    g = _grid(gpu_ctx, cells, mpc)
    d = bl.ObstacleDistanceGrid(ctx=gpu_ctx, metric="euclidean", max_cells=R)
    d.setDistances(g)
    f = d.table()
    assert f.dtype == np.float32 and f.tobytes() == em.table(R, mpc).tobytes()
    code = d.codes()
    assert np.array_equal(code, em.codes(cells, R)) and (code == R * R + 1).any()
    exp = em.floats(code, f)
    assert d.cells().tobytes() == exp.tobytes()
    rng = np.random.default_rng(8)
    q = np.stack([rng.integers(-3, w + 3, 400), rng.integers(-3, h + 3, 400)], axis=1).astype(np.int32)
    out = np.zeros(400, np.float32)
    _capi.check(gpu_ctx.lib.bl_dist_gather(d.h, q.ctypes.data, 400, out.ctypes.data))
    inside = (q[:, 0] >= 0) & (q[:, 0] < w) & (q[:, 1] >= 0) & (q[:, 1] < h)
    assert np.isnan(out[~inside]).all() and out[inside].tobytes() == exp[q[inside, 1], q[inside, 0]].tobytes()
    # the device pointer: the floats follow every later transform
    ptr = gpu_ctx.lib.bl_dist_device_ptr(d.h)
    assert ptr
    flipped = cells[::-1].copy()
    g.upload(flipped)
    d.setDistances(g)
    gpu_ctx.sync()
    host = np.empty((h, w), np.float32)
    assert _hip_runtime().hipMemcpy(C.c_void_p(host.ctypes.data), C.c_void_p(ptr), C.c_size_t(host.nbytes), 2) == 0      # hipMemcpyDeviceToHost
    assert host.tobytes() == em.floats(em.codes(flipped, R), f).tobytes()
    # no source: -1 everywhere
    g.upload(_free(h, w))
    d.setDistances(g)
    assert (d.codes() == em.NONE16).all() and (d.cells() == np.float32(-1.0)).all()
    d.close()
    g.close()


def test_create_refuses_caps_outside_1_to_254(gpu_ctx):
    for bad in (0, 255, -1, 70000):
        h = C.c_void_p()
        assert gpu_ctx.lib.bl_dist_create_euclidean(gpu_ctx.h, bad, C.byref(h)) == _capi.BL_ERR_ARG, bad
        assert b"max_cells" in gpu_ctx.lib.bl_last_error()
    for ok in (1, 254):
        d = bl.ObstacleDistanceGrid(ctx=gpu_ctx, metric="euclidean", max_cells=ok)
        assert d.metric() == ("euclidean", ok)
        d.close()


def test_l1_only_calls_refuse_a_euclidean_grid(maps, gpu_ctx):
    """The search and what is defined through it, and the particle filter's seeding, return BL_ERR_ARG with a text that says why; the
    handle stays usable.  (The replanner, the planner lanes and the explorer make their own L1 grids: they take no bl_dist.)"""
    lib = gpu_ctx.lib
    m = maps["obstacle_slam_10mx10m_5cm"]
    g = bl.OccupancyGrid.from_cells(m["cells"], m["origin"], m["mpc"], cellsPerMeter=CPM, ctx=gpu_ctx)
    d = bl.ObstacleDistanceGrid(ctx=gpu_ctx, metric="euclidean", max_cells=64)
    d.setDistances(g)
    start, goal = bl.make_pose(0.0, 0.0, 0.0), bl.make_pose(-0.35, 0.2, 0.0)
    sp = bl.SearchParams(0.2, 2.0, 1.0)
    buf, n, stats = (bl.Pose * 64)(), C.c_int(), (C.c_int64 * 6)()
    lens = (C.c_int * 2)()
    goals = (bl.Pose * 2)(goal, goal)
    pf = bl.ParticleFilter(256, ctx=gpu_ctx)
    pf.initializeFilterAtPose(start, seed=1)                                         # (its device pose is the start of one of the searches)
    fr = bl.Frontiers.from_lists(gpu_ctx, [np.array([[0.5, 0.5], [0.55, 0.5]], np.float32)])
    st = _capi.MotionPlannerState(0.2, sp, 1, bl.make_pose(1e9, 1e9, 0.0))
    chosen = bl.Pose()
    rec = _capi.PfRecoveryParams(0.001, 0.1, 1.0, 0.5, 0.0, 1)
    calls = {
        "bl_astar_search": lambda: lib.bl_astar_search(gpu_ctx.h, d.h, C.byref(start), C.byref(goal), C.byref(sp), buf, 64, C.byref(n), stats),
        "bl_astar_search_async": lambda: lib.bl_astar_search_async(gpu_ctx.h, d.h, C.byref(start), C.byref(goal), C.byref(sp)),
        "bl_astar_search_async_dev_start": lambda: lib.bl_astar_search_async_dev_start(gpu_ctx.h, d.h, pf.poseDevicePtr(), C.byref(goal), C.byref(sp)),
        "bl_astar_search_batch": lambda: lib.bl_astar_search_batch(gpu_ctx.h, d.h, C.byref(start), goals, 2, C.byref(sp), buf, 32, lens, stats),
        "bl_plan_path_to_frontier": lambda: lib.bl_plan_path_to_frontier(gpu_ctx.h, fr.h, C.byref(start), d.h, C.byref(st), buf, 64, C.byref(n),
                                                                         C.byref(chosen), stats),
        "bl_pf_init_uniform": lambda: lib.bl_pf_init_uniform(pf.h, g.h, d.h, 0.1, 0, 1),
        "bl_pf_set_recovery": lambda: lib.bl_pf_set_recovery(pf.h, g.h, d.h, C.byref(rec)),
    }
    exp = em.codes(m["cells"], 64)
    for name, call in calls.items():
        assert call() == _capi.BL_ERR_ARG, name
        msg = lib.bl_last_error()
        assert b"L1" in msg and b"Euclidean" in msg, (name, msg)
        assert np.array_equal(d.codes(), exp), name                                 # the handle is as usable as before
    # nothing was left pending on the ctx, and the same calls go through on an L1 grid of the same map
    l1 = bl.ObstacleDistanceGrid(ctx=gpu_ctx)
    l1.setDistances(g)
    assert len(bl.search_for_path(start, goal, l1, sp)) > 1
    pf.initializeFilterUniformly(g, l1, 0.1, seed=1)
    d.setDistances(g)
    assert np.array_equal(d.codes(), exp)
    for x in (pf, fr, l1, d, g):
        x.close()


def test_field_refuses_a_cost_range_beyond_the_cap(maps, gpu_ctx):
    m = maps["obstacle_slam_10mx10m_5cm"]
    g = bl.OccupancyGrid.from_cells(m["cells"], m["origin"], m["mpc"], cellsPerMeter=CPM, ctx=gpu_ctx)
    d = bl.ObstacleDistanceGrid(ctx=gpu_ctx, metric="euclidean", max_cells=20)          # f[R^2] = (float)(20 * 0.05) = 1 m
    d.setDistances(g)
    f = d.table()
    nf = bl.NavigationField(gpu_ctx)
    goal = np.array([[100, 100]], np.int32)

    def rc(min_d, max_d):
        return gpu_ctx.lib.bl_navfield_compute(nf.h, d.h, C.byref(_capi.NavFieldParams(min_d, max_d, 1.0, 50, 0)), goal.ctypes.data, 1)
    assert rc(0.2, float(f[400]) * (1 + 1e-12)) == _capi.BL_ERR_ARG and b"maxDistanceWithCost" in gpu_ctx.lib.bl_last_error()
    assert rc(0.2, 2.0) == _capi.BL_ERR_ARG
    assert rc(0.2, float(f[400])) == _capi.BL_OK                                        # at the cap: every priced cell has its true distance
    assert rc(0.2, 0.1) == _capi.BL_OK                                                  # no penalty at all (max <= min): nothing is priced
    assert rc(3.0, 2.0) == _capi.BL_OK
    trav, pen = nf.tables()
    assert len(trav) == 402 and not trav.any()
    l1 = bl.ObstacleDistanceGrid(ctx=gpu_ctx)
    l1.setDistances(g)
    assert gpu_ctx.lib.bl_navfield_compute(nf.h, l1.h, C.byref(_capi.NavFieldParams(0.2, 2.0, 1.0, 50, 0)), goal.ctypes.data, 1) == _capi.BL_OK
    assert len(nf.tables()[0]) == 401                                                   # an L1 grid's table length is what it was
    for x in (nf, l1, d, g):
        x.close()
