"""The clearance grid on the device (bl_clearance_*, botlab_amd/csrc/bl_clearance.hip) against its model (tests/clearance_model.py):
every entry after a build and after an update.  All for equality.

The shapes are the smallest that reach each path of the two kernels: a single cell; a single row and a single column; a grid
inside one 64-cell word; 65 x 63 and 130 x 70, whose rows take two and three words, the last one partly filled; 300 x 10 with cap
255, where the cap exceeds the height and a row reads all four neighbouring words on a side."""
import ctypes as C

import numpy as np
import pytest

import botlab_amd as bl
import clearance_model as cm

pytestmark = pytest.mark.gpu
F32 = np.float32
MPC = F32(0.05)
CPM = F32(1.0 / np.float64(MPC))
SHAPES = [(1, 1), (1, 37), (37, 1), (8, 8), (65, 63), (130, 70)]              # width, height


def cells_of(w, h, seed=0, density=0.04):
    """Mostly free, a few cells occupied at 1, 2 and above, and as many at 0: occ_min - 1 for occ_min 1, and the cells at 1 for 2."""
    rng = np.random.default_rng(1000 * w + h + seed)
    cells = np.full((h, w), -20, np.int8)
    u = rng.random((h, w))
    cells[u < 4 * density] = 0
    cells[u < 3 * density] = 1
    cells[u < 2 * density] = 2
    cells[u < density] = rng.integers(3, 128, (h, w)).astype(np.int8)[u < density]
    n = w * h
    if n >= 8:                                                                # one of each kind whatever the draw
        cells.flat[n // 5], cells.flat[2 * n // 5], cells.flat[3 * n // 5], cells.flat[4 * n // 5] = 0, 1, 2, 90
    return cells


def grid_of(ctx, cells):
    return bl.OccupancyGrid.from_cells(np.ascontiguousarray(cells, np.int8), (F32(0), F32(0)), MPC, cellsPerMeter=CPM, ctx=ctx)


def same(got, exp, what=""):
    bad = np.argwhere(got != exp)
    assert got.shape == exp.shape and len(bad) == 0, (what, len(bad), bad[:4].tolist(), got[tuple(bad[0])], exp[tuple(bad[0])])


def check_build(ctx, cells, cap, occ_min=1, cl=None):
    own = cl is None
    cl = bl.ClearanceGrid(ctx, cap) if own else cl
    grid = grid_of(ctx, cells)
    try:
        cl.build(grid, occ_min)
        h, w = cells.shape
        assert cl.info() == dict(width=w, height=h, cap=cap, occ_min=occ_min, built=1, bytes=w * h)
        exp = cm.grid(cells, occ_min, cap)
        same(cl.read(), exp, (w, h, cap, occ_min))
        if w > 2 and h > 2:                                                   # a window inside
            same(cl.read(1, 2 % h, w - 2, h - 2), exp[2 % h:2 % h + h - 2, 1:w - 1])
        assert cl.lastDeviceMs() > 0
        return exp
    finally:
        grid.close()
        if own:
            cl.close()


@pytest.mark.parametrize("cap", [1, 2, 64, 255])
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_build_equals_the_model(gpu_ctx, shape, cap):
    w, h = shape
    for occ_min in (1, 2):
        cells = cells_of(w, h)
        if w * h > 1:
            assert (cells == occ_min - 1).any() and (cells >= occ_min).any()
        exp = check_build(gpu_ctx, cells, cap, occ_min)
        assert np.array_equal(exp == 0, cells >= occ_min)


def test_cap_beyond_the_height_and_four_words_a_side(gpu_ctx):
    cells = np.full((10, 300), -20, np.int8)
    cells[4, 2] = 50                                                          # the far end of the row lies 297 cells away: capped
    exp = check_build(gpu_ctx, cells, 255)
    assert exp[4, 299] == 255 and exp[9, 257] == 255 and exp[0, 256] == 254 and exp[4, 2] == 0
    cells[7, 299] = 1
    exp = check_build(gpu_ctx, cells, 255)                                    # read from the left for some cells, from the right for others
    assert exp[0, 150] == 148 and exp[0, 151] == 148 and exp[0, 152] == 147
    check_build(gpu_ctx, cells_of(300, 10, density=0.002), 255)
    check_build(gpu_ctx, cells_of(300, 10, seed=1, density=0.002), 200)


@pytest.mark.parametrize("cap", [1, 64, 255])
def test_all_free_all_occupied_and_the_corners(gpu_ctx, cap):
    for w, h in ((65, 63), (130, 70)):
        assert (check_build(gpu_ctx, np.full((h, w), 0, np.int8), cap) == cap).all()
        assert (check_build(gpu_ctx, np.full((h, w), 1, np.int8), cap, occ_min=2) == cap).all()
        assert (check_build(gpu_ctx, np.full((h, w), 1, np.int8), cap) == 0).all()
        for cy, cx in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):
            cells = np.full((h, w), -20, np.int8)
            cells[cy, cx] = 127
            exp = check_build(gpu_ctx, cells, cap)
            assert exp[h - 1 - cy, w - 1 - cx] == min(cap, max(w, h) - 1)


def test_caps_refused_and_a_handle_rebuilt_on_another_shape(gpu_ctx):
    for bad in (0, 256, -1, 1000):
        h = C.c_void_p()
        assert gpu_ctx.lib.bl_clearance_create(gpu_ctx.h, bad, C.byref(h)) == 2 and not h.value
    cl = bl.ClearanceGrid(gpu_ctx, 7)
    try:
        assert cl.info() == dict(width=0, height=0, cap=7, occ_min=0, built=0, bytes=0)
        ms = C.c_float()
        assert gpu_ctx.lib.bl_clearance_last_device_ms(cl.h, C.byref(ms)) == 4
        with pytest.raises(bl.BotlabHipError, match="status 4"):
            cl.read(0, 0, 1, 1)
        grid = grid_of(gpu_ctx, cells_of(8, 8))
        try:
            for occ_min in (0, 128, -3):
                with pytest.raises(bl.BotlabHipError, match="status 2"):
                    cl.build(grid, occ_min)
            assert cl.info()["built"] == 0
        finally:
            grid.close()
        check_build(gpu_ctx, cells_of(65, 63), 7, cl=cl)
        for box in ((0, 0, 66, 1), (64, 62, 1, 2), (-1, 0, 1, 1), (0, 0, 0, 1), (0, 0, 1, 0)):
            with pytest.raises(bl.BotlabHipError, match="status 2"):
                cl.read(*box)
        check_build(gpu_ctx, cells_of(8, 8), 7, cl=cl)                        # a smaller shape
        check_build(gpu_ctx, cells_of(130, 70), 7, occ_min=2, cl=cl)          # a larger one, another occ_min
        check_build(gpu_ctx, cells_of(1, 37), 7, cl=cl)
    finally:
        cl.close()


def changed(cells, edits):
    """The cells with (x, y, value) written, and the inclusive bounding box of the edits."""
    new = cells.copy()
    for x, y, v in edits:
        new[y, x] = v
    xs, ys = [e[0] for e in edits], [e[1] for e in edits]
    return new, (min(xs), min(ys), max(xs), max(ys))


@pytest.mark.parametrize("cap", [3, 64, 255])
def test_update_equals_a_fresh_build(gpu_ctx, cap):
    w, h = 130, 70
    cells = cells_of(w, h, density=0.01)
    cells[30:34, 60:70] = -20
    cl, grid = bl.ClearanceGrid(gpu_ctx, cap), grid_of(gpu_ctx, cells)
    try:
        cl.build(grid, 1)
        same(cl.read(), cm.grid(cells, 1, cap))
        occ = np.argwhere(cells >= 1)
        free = np.argwhere(cells < 1)
        steps = [("inside", [(64, 31, 100), (66, 33, 90)]),
                 ("inside-freed", [(int(occ[len(occ) // 2][1]), int(occ[len(occ) // 2][0]), -20)]),
                 ("corner", [(0, 0, 100), (1, 1, 100)]),
                 ("far-corner", [(w - 1, h - 1, 100), (w - 2, h - 2, 5)]),
                 ("both-ways", [(int(x), int(y), -20) for y, x in occ[[0, -1]]] + [(int(x), int(y), 100) for y, x in free[[7, -9]]])]
        for name, edits in steps:
            new, box = changed(cells, edits)
            assert ((new >= 1) != (cells >= 1)).any()
            grid.upload(new)
            fresh = cm.grid(new, 1, cap)
            assert not np.array_equal(fresh, cm.grid(cells, 1, cap))
            if cap == 3 and name != "both-ways":                              # the widened box is a part of the grid: the rest must stay
                assert cm.widened(box, cap, w, h) != (0, 0, w - 1, h - 1)
            cl.update(grid, *box)
            same(cl.read(), fresh, name)
            cells = new
        # boxes clipped on each side, one at a time and all at once
        for k, (edit, box) in enumerate([((0, 35, 100), (-7, 35, 0, 35)), ((w - 1, 36, 100), (w - 1, 36, w + 50, 36)),
                                         ((64, 0, 100), (64, -2 ** 31, 64, 0)), ((65, h - 1, 100), (65, h - 1, 65, 2 ** 31 - 1))]):
            new, _ = changed(cells, [edit])
            grid.upload(new)
            cl.update(grid, *box)
            same(cl.read(), cm.grid(new, 1, cap), ("clipped", k))
            cells = new
        new, _ = changed(cells, [(0, 40, -20 if cells[40, 0] >= 1 else 100), (w - 1, 41, 100), (60, 0, 100), (61, h - 1, 100), (64, 35, 100)])
        grid.upload(new)
        cl.update(grid, -5, -1000, w + 5, 2 ** 31 - 1)
        fresh = cm.grid(new, 1, cap)
        same(cl.read(), fresh, "clipped on all sides")
        # the boxes that change nothing: empty, or wholly outside
        new2, _ = changed(new, [(5, 5, 100), (120, 60, 100)])
        assert not np.array_equal(cm.grid(new2, 1, cap), fresh)
        grid.upload(new2)
        for box in ((3, 3, 2, 5), (0, 4, 5, 3), (-9, -9, -1, -1), (w, 0, w + 5, 5), (0, h, 5, h + 5), (-2 ** 31, 0, -1, h - 1)):
            cl.update(grid, *box)
        same(cl.read(), fresh, "nothing computed")
        cl.update(grid, 0, 0, w - 1, h - 1)                                   # the whole grid
        same(cl.read(), cm.grid(new2, 1, cap), "whole grid")
        # a map of another shape: refused, the grid stays
        other = grid_of(gpu_ctx, cells_of(65, 63))
        try:
            keep = cl.read()
            with pytest.raises(bl.BotlabHipError, match="status 2"):
                cl.update(other, 0, 0, 5, 5)
            same(cl.read(), keep)
            assert cl.info()["built"] == 1
        finally:
            other.close()
    finally:
        cl.close()
        grid.close()


def test_update_before_build_is_refused(gpu_ctx):
    cl, grid = bl.ClearanceGrid(gpu_ctx), grid_of(gpu_ctx, cells_of(8, 8))
    try:
        assert cl.info()["cap"] == 64
        with pytest.raises(bl.BotlabHipError, match="status 4"):
            cl.update(grid, 0, 0, 1, 1)
    finally:
        cl.close()
        grid.close()
