"""The view-gain kernel (bl_viewgain_*, botlab_amd/csrc/bl_viewgain.hip) against the model (tests/view_gain_model.py), for equality:
the definition is integer arithmetic.  Gains are compared on the LIBRARY's ray table, and the table itself with the model's, so a
difference in cos / sin / lround cannot hide in the gains."""
import ctypes as C

import numpy as np
import pytest

import botlab_amd as bl
from botlab_amd import _capi
import helpers
import view_gain_model as vm

pytestmark = pytest.mark.gpu
MAPS = ["obstacle_slam_10mx10m_5cm", "convex_10mx10m_5cm", "drive_square_10mx10m_5cm", "astar_maze"]
CPM = helpers.CPM_DEFAULT


def _grid(cells, ctx):
    h, w = cells.shape
    return bl.OccupancyGrid.from_cells(cells, (np.float32(-w * 0.025), np.float32(-h * 0.025)), 0.05, cellsPerMeter=CPM, ctx=ctx)


@pytest.fixture(scope="module")
def explored(maps):
    out = {}
    for name in MAPS:
        cells, _ = vm.partially_explored(maps[name]["cells"])
        out[name] = (cells, vm.near_frontier_candidates(cells, 3))
    return out


@pytest.mark.parametrize("r,k", [(60, 360), (1, 8), (255, 4096), (100, 360), (17, 1), (255, 1), (1, 1), (33, 77)])
def test_ray_table_equals_the_model(gpu_ctx, r, k):
    vg = bl.ViewGain(r, k, ctx=gpu_ctx)
    try:
        assert np.array_equal(vg.rayEnds(), vm.ray_ends(r, k))
    finally:
        vg.close()


@pytest.mark.parametrize("r,k", [(60, 360), (1, 8), (255, 720), (20, 1), (100, 360), (7, 4096)])
def test_every_candidate_equals_the_model(gpu_ctx, explored, r, k):
    vg = bl.ViewGain(r, k, ctx=gpu_ctx)
    p = vm.Params(r, k)
    try:
        ends = vg.rayEnds()
        for name in MAPS:
            cells, cands = explored[name]
            g = _grid(cells, gpu_ctx)
            got = vg.compute(g, cands)
            g.close()
            want = vm.gains(cells, p, cands, ends)
            bad = np.flatnonzero(got != want)
            assert len(bad) == 0, (name, r, k, len(bad), cands[bad[:5]].tolist(), got[bad[:5]].tolist(), want[bad[:5]].tolist())
            print(name, "R", r, "K", k, "candidates", len(cands), "gain", int(got.min()), "..", int(got.max()))
    finally:
        vg.close()


def test_largest_window_and_fan(gpu_ctx, explored):
    """R = 255 and K = 4096 together: the largest bitmap and the most rays."""
    vg = bl.ViewGain(255, 4096, ctx=gpu_ctx)
    try:
        cells, cands = explored["astar_maze"]
        g = _grid(cells, gpu_ctx)
        assert np.array_equal(vg.compute(g, cands), vm.gains(cells, vm.Params(255, 4096), cands, vg.rayEnds()))
        g.close()
    finally:
        vg.close()


def test_seen_windows_are_equal_as_bytes(gpu_ctx, explored):
    for r, k in [(60, 360), (255, 720), (1, 8)]:
        vg = bl.ViewGain(r, k, ctx=gpu_ctx)
        p = vm.Params(r, k)
        wt = vm.walks(vg.rayEnds())
        for name in MAPS:
            cells, cands = explored[name]
            g = _grid(cells, gpu_ctx)
            for x, y in cands[::max(len(cands) // 12, 1)]:
                got = vg.debugSeen(g, int(x), int(y))
                want = vm.seen_mask(cells, p, wt, int(x), int(y))
                assert got.tobytes() == want.tobytes(), (name, r, k, int(x), int(y), int(got.sum()), int(want.sum()))
            assert not vg.debugSeen(g, -3, 5).any()
            g.close()
        vg.close()


def test_class_thresholds(gpu_ctx, maps):
    cells = maps["obstacle_slam_10mx10m_5cm"]["cells"]
    g = _grid(cells, gpu_ctx)
    h, w = cells.shape
    cands = np.array([(x, y) for y in range(3, h, 13) for x in range(5, w, 11)], np.int32)
    for occ, lo, hi in [(0, 0, 0), (20, -10, 10), (127, -128, 127), (-128, -128, 127), (-1, 0, 0), (50, 1, 50)]:
        vg = bl.ViewGain(40, 180, occ, lo, hi, ctx=gpu_ctx)
        want = vm.gains(cells, vm.Params(40, 180, occ, lo, hi), cands, vg.rayEnds())
        assert np.array_equal(vg.compute(g, cands), want), (occ, lo, hi)
        vg.close()
    g.close()


def test_off_grid_blocking_and_duplicate_candidates(gpu_ctx, explored):
    cells, cands = explored["drive_square_10mx10m_5cm"]
    h, w = cells.shape
    g = _grid(cells, gpu_ctx)
    vg = bl.ViewGain(60, 360, ctx=gpu_ctx)
    p = vm.Params(60, 360)
    by, bx = np.nonzero(cells > 0)
    q = [(-1, 0), (0, -1), (w, 0), (0, h), (-2 ** 31, 2 ** 31 - 1), (0, 0), (w - 1, h - 1), (0, h - 1), (w - 1, 0)]
    q += [(int(bx[i]), int(by[i])) for i in range(0, len(bx), max(len(bx) // 20, 1))]            # on blocking cells
    q += [tuple(int(v) for v in cands[0])] * 5 + [tuple(int(v) for v in cands[-1])] * 3         # duplicates
    got = vg.compute(g, np.array(q, np.int64).astype(np.int32))
    want = vm.gains(cells, p, q, vg.rayEnds())
    assert np.array_equal(got, want)
    assert not got[:5].any() and len(set(got[-8:-3].tolist())) == 1
    vg.close()
    g.close()


def test_calls_and_errors(gpu_ctx, explored):
    lib = gpu_ctx.lib
    cells, cands = explored["astar_maze"]
    g = _grid(cells, gpu_ctx)
    h = C.c_void_p()
    assert lib.bl_viewgain_create(gpu_ctx.h, C.byref(h)) == 0
    out = np.zeros(4, np.uint32)
    q = np.ascontiguousarray(cands[:4], dtype=np.int32)
    n = C.c_int()
    # before set_params
    assert lib.bl_viewgain_compute(h, g.h, q.ctypes.data, 4, out.ctypes.data) == _capi.BL_ERR_STATE
    assert lib.bl_viewgain_ray_ends(h, None, C.byref(n)) == _capi.BL_ERR_STATE
    assert lib.bl_viewgain_debug_seen(h, g.h, 1, 1, out.ctypes.data) == _capi.BL_ERR_STATE
    for bad in [(0, 360, 0, 0, 0), (256, 360, 0, 0, 0), (60, 0, 0, 0, 0), (60, 4097, 0, 0, 0), (60, 360, 128, 0, 0), (60, 360, 0, 1, 0),
                (60, 360, 0, -129, 0), (60, 360, 0, 0, 128)]:
        assert lib.bl_viewgain_set_params(h, C.byref(_capi.ViewGainParams(*bad))) == _capi.BL_ERR_ARG, bad
    assert lib.bl_viewgain_compute(h, g.h, q.ctypes.data, 4, out.ctypes.data) == _capi.BL_ERR_STATE
    assert lib.bl_viewgain_set_params(h, C.byref(_capi.ViewGainParams(60, 360, 0, 0, 0))) == 0
    assert lib.bl_viewgain_compute(h, g.h, None, 0, None) == 0                                  # n = 0
    assert lib.bl_viewgain_compute(h, g.h, q.ctypes.data, -1, out.ctypes.data) == _capi.BL_ERR_ARG
    assert lib.bl_viewgain_compute(h, g.h, q.ctypes.data, 4, out.ctypes.data) == 0
    assert np.array_equal(out, vm.gains(cells, vm.Params(60, 360), cands[:4]))
    lib.bl_viewgain_destroy(h)
    vg = bl.ViewGain(60, 360, ctx=gpu_ctx)
    assert len(vg.compute(g, np.zeros((0, 2), np.int32))) == 0
    vg.close()
    g.close()
    with pytest.raises(bl.BotlabHipError):
        bl.ViewGain(0, 360, ctx=gpu_ctx)


def test_new_params_on_one_handle(gpu_ctx, explored):
    cells, cands = explored["obstacle_slam_10mx10m_5cm"]
    g = _grid(cells, gpu_ctx)
    vg = bl.ViewGain(60, 360, ctx=gpu_ctx)
    a = vg.compute(g, cands)
    vg.setParams(25, 90)
    b = vg.compute(g, cands)
    assert np.array_equal(b, vm.gains(cells, vm.Params(25, 90), cands, vg.rayEnds())) and not np.array_equal(a, b)
    assert vg.debugSeen(g, int(cands[0][0]), int(cands[0][1])).shape == (51, 51)
    vg.setParams(120, 1000, 10, -5, 5)                              # grows the table and the window
    assert np.array_equal(vg.compute(g, cands), vm.gains(cells, vm.Params(120, 1000, 10, -5, 5), cands, vg.rayEnds()))
    vg.setParams(60, 360)
    assert np.array_equal(vg.compute(g, cands), a)
    vg.close()
    g.close()


def test_larger_calls_on_one_handle(gpu_ctx, explored):
    """The handle's buffers are reallocated by a larger call: 5 candidates and then all 84 (candidates and gains), a 21 x 21 window
    and then an 81 x 81 one (the bitmap of debugSeen), each against the model."""
    cells, cands = explored["astar_maze"]
    assert len(cands) > 5
    g = _grid(cells, gpu_ctx)
    vg = bl.ViewGain(10, 90, ctx=gpu_ctx)
    try:
        for r, k in [(10, 90), (40, 180)]:
            vg.setParams(r, k)
            p, ends = vm.Params(r, k), vg.rayEnds()
            for part in (cands[:5], cands):
                assert np.array_equal(vg.compute(g, part), vm.gains(cells, p, part, ends)), (r, k, len(part))
            x, y = int(cands[7][0]), int(cands[7][1])
            got = vg.debugSeen(g, x, y)
            assert got.shape == (2 * r + 1, 2 * r + 1) and got.tobytes() == vm.seen_mask(cells, p, vm.walks(ends), x, y).tobytes(), (r, k)
    finally:
        vg.close()
        g.close()


def test_map_reuploaded_and_reshaped(gpu_ctx, explored, maps):
    vg = bl.ViewGain(60, 360, ctx=gpu_ctx)
    p = vm.Params(60, 360)
    cells, cands = explored["convex_10mx10m_5cm"]
    g = _grid(cells, gpu_ctx)
    assert np.array_equal(vg.compute(g, cands), vm.gains(cells, p, cands))
    other = explored["drive_square_10mx10m_5cm"][0]
    assert other.shape == cells.shape and not np.array_equal(other, cells)
    g.upload(other)                                                 # the same grid, other contents
    assert np.array_equal(vg.compute(g, cands), vm.gains(other, p, cands))
    g.close()
    small = np.ascontiguousarray(cells[40:150, 30:171])             # a smaller grid of another aspect
    gs = _grid(small, gpu_ctx)
    cs = vm.near_frontier_candidates(small, 3)
    extra = np.array([(small.shape[1] - 1, small.shape[0] - 1), (small.shape[1], 0), (0, small.shape[0]), (150, 100)], np.int64)
    cs = np.concatenate([cs, extra])
    assert np.array_equal(vg.compute(gs, cs), vm.gains(small, p, cs))
    gs.close()
    vg.close()


def test_large_partially_explored_map(gpu_ctx, maps):
    """2000 x 2000 tiling of the maze, known inside a disc of 700 cells: every near-frontier candidate at R = 100; a seeded sample of
    250 against the model, all of them against the number of unknown cells in their window."""
    from botlab_amd import synth
    side, r = 2000, 100
    world = synth.tile_world(maps["astar_maze"]["cells"], side)
    yy, xx = np.ogrid[:side, :side]
    cells = np.where((xx - side // 2) ** 2 + (yy - side // 2) ** 2 <= 700 ** 2, world, 0).astype(np.int8)
    cands = vm.near_frontier_candidates(cells, 3)
    assert len(cands) >= 2000
    g = _grid(cells, gpu_ctx)
    vg = bl.ViewGain(r, 360, ctx=gpu_ctx)
    p = vm.Params(r, 360)
    got = vg.compute(g, cands)
    pick = np.sort(np.random.default_rng(20261017).choice(len(cands), 250, replace=False))
    want = vm.gains(cells, p, cands[pick], vg.rayEnds())
    assert np.array_equal(got[pick], want)
    # the window bound for all of them, from a summed-area table of the unknown cells
    sat = np.zeros((side + 1, side + 1), np.int64)
    sat[1:, 1:] = np.cumsum(np.cumsum(cells == 0, axis=0), axis=1)
    x0, x1 = np.maximum(cands[:, 0] - r, 0), np.minimum(cands[:, 0] + r, side - 1) + 1
    y0, y1 = np.maximum(cands[:, 1] - r, 0), np.minimum(cands[:, 1] + r, side - 1) + 1
    bound = sat[y1, x1] - sat[y0, x1] - sat[y1, x0] + sat[y0, x0] - (cells[cands[:, 1], cands[:, 0]] == 0)
    assert np.all(got.astype(np.int64) <= bound)
    assert all(int(bound[i]) == vm.window_bound(cells, p, int(cands[i][0]), int(cands[i][1])) for i in pick[:20])
    print("candidates", len(cands), "gain", int(got.min()), "..", int(got.max()), "zero", int((got == 0).sum()))
    assert got.max() > 0
    vg.close()
    g.close()
