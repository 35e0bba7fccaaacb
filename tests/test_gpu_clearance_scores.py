"""The beam model scored by leaps over a clearance grid (bl_clearance_scores, bl_clearance_debug_cast; k_beam_leap, bl_beam.hip).
The yardstick is tests/beam_model.py: debug_leap column by column against beam_model.cast, the rounds against the leap model
(tests/clearance_model.py), the scores and units against beam_model.scores / units, and on a 200 x 200 map against the device's own
cast.  All for equality."""
import ctypes as C
import math

import numpy as np
import pytest

import botlab_amd as bl
import beam_cases as bc
import beam_edge_cases as ec
import beam_model as bm
import clearance_model as cm
import helpers
from test_gpu_beam import KEYS, beam_of, grid_of, scan_of

pytestmark = pytest.mark.gpu
F32 = np.float32
COLS = ("first", "K", "z", "zstar", "p", "rounds")
_GRIDS = {}


def model_grid(c, cap):
    """The model's clearance grid of a case, built once and kept."""
    key = (c["cells"].tobytes(), c["cells"].shape, c["params"]["occ_min"], cap)
    if key not in _GRIDS:
        _GRIDS[key] = cm.grid(c["cells"], c["params"]["occ_min"], cap)
        _GRIDS[key].setflags(write=False)
    return _GRIDS[key]


def check_leap(ctx, c, cap=64, casts=None, beam=None, grid=None, cl=None, exp=None):
    """The beam case scored by leaps on the device beside the model: the grid, the scores, the units and debug_leap of the poses
    `casts` (default: the first 6).  Returns (scores, units, the model's per-ray values of the poses cast)."""
    own_b, own_g, own_c = beam is None, grid is None, cl is None
    beam = beam_of(ctx, c) if own_b else beam
    grid = grid_of(ctx, c) if own_g else grid
    cl = bl.ClearanceGrid(ctx, cap) if own_c else cl
    try:
        if own_c:
            cl.build(grid, c["params"]["occ_min"])
        D = model_grid(c, cap)
        assert np.array_equal(cl.read(), D)
        t = beam.tables(c["cpm"])
        exp = bm.scores(c["cells"], c["origin"], c["cpm"], c["ranges"], c["thetas"], c["poses"], c["params"], t) if exp is None else exp
        got = beam.scores_leap(cl, scan_of(c), c["poses"])
        bad = np.flatnonzero(got != exp)
        assert len(bad) == 0, (len(bad), int(bad[0]), int(got[bad[0]]), int(exp[bad[0]]))
        u = beam.units(len(c["poses"]))
        assert np.array_equal(u, bm.units(exp, c["params"]["span"], bl.BeamModel.unitTable()))
        if len(c["poses"]):
            assert beam.lastDeviceMs() > 0 and beam.debugPath() == 1
        rays = bm.used_rays(c["ranges"], c["thetas"], c["params"])
        assert beam.ctx.lib.bl_beam_last_rays(beam.h) == len(rays[0])
        seen = {}
        for i in (range(min(6, len(c["poses"]))) if casts is None else casts):
            g = beam.debug_leap(cl, scan_of(c), c["poses"][i])
            e = cm.cast(c["cells"], D, c["origin"], c["cpm"], rays, c["poses"][i], c["params"], t)
            for col in COLS:
                want = e[col] if e is not None else np.zeros(len(rays[0]), np.int64)
                assert np.array_equal(g[col], want), (i, col, g[col].tolist(), want.tolist())
            seen[i] = e
        assert np.array_equal(beam.units(len(c["poses"])), u)                 # a debug call leaves the last call's units and count alone
        return got, u, seen
    finally:
        if own_b:
            beam.close()
        if own_g:
            grid.close()
        if own_c:
            cl.close()


# ---------------------------------------------------------------------------------------------------------------- poses and rays
@pytest.mark.parametrize("cap", [1, 5, 64])
@pytest.mark.parametrize("w,h,occ_min", [(64, 48, 1), (64, 48, 2), (130, 70, 1)])
def test_conditions(gpu_ctx, w, h, occ_min, cap):
    """Walks leaving the grid, a pose on an occupied cell (first = 0), NaN and off-grid poses, dropped rays, max readings with and
    without an expected hit, returns short of, at and behind it."""
    c = bc.conditions(w, h, occ_min=occ_min)
    c = dict(c, ranges=np.concatenate([c["ranges"], [F32(0.5)]]).astype(np.float32),
             thetas=np.concatenate([c["thetas"], [F32("nan")]]).astype(np.float32))         # a ray that `has` drops for every pose
    s, u, seen = check_leap(gpu_ctx, c, cap=cap, casts=range(len(c["poses"])))
    assert (s == bm.OFF_GRID).sum() == 4 and s[0] == s[9]
    t = bm.make_tables(c["params"], c["cpm"])
    rays = bm.used_rays(c["ranges"], c["thetas"], c["params"])
    on = [e for e in seen.values() if e is not None]
    assert len(on) == len(c["poses"]) - 4
    assert all(e["rounds"][-1] == -1 and e["p"][-1] == 0 for e in on)
    first, K = np.concatenate([e["first"][:-1] for e in on]), np.concatenate([e["K"][:-1] for e in on])
    assert (first == 0).any() and (first == K).any() and ((first > 0) & (first < K)).any()
    mx = np.concatenate([np.stack([e["zstar"][rays[2]], e["p"][rays[2]]]) for e in on], axis=1)
    assert (mx[0] >= 0).any() and (mx[0] < 0).any() and set(mx[1].tolist()) == {t["max_blocked"], t["max_free"]}
    rounds = np.concatenate([e["rounds"][:-1] for e in on])
    if cap == 1:                                                              # every cell up to the hit is read
        assert np.array_equal(rounds[first < K], first[first < K] + 1)
    else:
        assert rounds.sum() < np.concatenate([np.minimum(e["first"][:-1] + 1, e["K"][:-1]) for e in on]).sum()


def golden_case(n=257):
    m = helpers.load_reference_maps()["obstacle_slam_10mx10m_5cm"]
    rng = np.random.default_rng(257)
    h, w = m["cells"].shape
    assert (h, w) == (200, 200)
    th = (2.0 * math.pi * np.arange(290) / 290.0).astype(np.float32)
    rg = rng.uniform(0.2, 5.6, 290).astype(np.float32)                        # returns and max readings
    ox, oy = float(m["origin"][0]), float(m["origin"][1])
    poses = np.stack([rng.uniform(ox - 0.1, ox + w * 0.05 + 0.1, n), rng.uniform(oy - 0.1, oy + h * 0.05 + 0.1, n), rng.uniform(-3.1, 3.1, n)], axis=1)
    return bc.case(m["cells"], rg, th, poses.astype(np.float32), origin=m["origin"], max_range=5.0)


@pytest.mark.parametrize("cap", [16, 64, 255])
def test_scores_and_units_equal_the_device_cast_on_a_200x200_map(gpu_ctx, cap):
    c = golden_case()
    beam, grid, cl = beam_of(gpu_ctx, c), grid_of(gpu_ctx, c), bl.ClearanceGrid(gpu_ctx, cap)
    try:
        a = beam.scores(grid, scan_of(c), c["poses"])
        ua = beam.units(len(c["poses"]))
        cl.build(grid, c["params"]["occ_min"])
        b = beam.scores_leap(cl, scan_of(c), c["poses"])
        ub = beam.units(len(c["poses"]))
        assert np.array_equal(a, b) and np.array_equal(ua, ub)
        assert (a == bm.OFF_GRID).any() and (a != bm.OFF_GRID).sum() > 200 and len(set(ua.tolist())) > 3
        D = model_grid(c, cap)
        assert np.array_equal(cl.read(), D)
        t = beam.tables(c["cpm"])
        rays = bm.used_rays(c["ranges"], c["thetas"], c["params"])
        i = int(np.flatnonzero(a != bm.OFF_GRID)[0])
        g, e = beam.debug_leap(cl, scan_of(c), c["poses"][i]), cm.cast(c["cells"], D, c["origin"], c["cpm"], rays, c["poses"][i], c["params"], t)
        d = beam.debug_cast(grid, scan_of(c), c["poses"][i])
        for col in COLS:
            assert np.array_equal(g[col], e[col]), col
            assert col == "rounds" or np.array_equal(g[col], d[col]), col
    finally:
        cl.close()
        beam.close()
        grid.close()


@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, 257])
def test_pose_counts(gpu_ctx, n):
    c = bc.many_poses(n)
    s, u, _ = check_leap(gpu_ctx, c, casts=range(min(n, 2)))
    if n >= 63:
        assert (s == bm.OFF_GRID).any() and (u == 2 ** 20).sum() >= 1


@pytest.mark.parametrize("rays,stride,dropped", [(1, 1, 0), (63, 1, 0), (64, 1, 3), (65, 1, 0), (65, 3, 2), (290, 3, 0), (4096, 1, 0)])
def test_ray_counts(gpu_ctx, rays, stride, dropped):
    c = bc.ray_count(rays, stride=stride, dropped_every=dropped)
    assert len(bm.used_rays(c["ranges"], c["thetas"], c["params"])[0]) == (rays + stride - 1) // stride
    check_leap(gpu_ctx, c, casts=[0, 2] if rays < 4096 else [0])


def test_too_many_rays_refused_and_every_ray_dropped(gpu_ctx):
    c = bc.ray_count(4097)
    beam, grid, cl = beam_of(gpu_ctx, c), grid_of(gpu_ctx, c), bl.ClearanceGrid(gpu_ctx, 64)
    try:
        cl.build(grid, 1)
        with pytest.raises(bl.BotlabHipError, match="status 2"):
            beam.scores_leap(cl, scan_of(c), c["poses"])
        d = bc.ray_count(5)
        d["ranges"] = np.array([0.0, 0.15, -2.0, float("nan"), float("inf")], np.float32)
        d["poses"] = np.concatenate([d["poses"], [bc.centre(-5, 2)]]).astype(np.float32)
        s, u, _ = check_leap(gpu_ctx, d, beam=beam, grid=grid, cl=cl)
        assert s.tolist() == [0, 0, 0, bm.OFF_GRID] and u.tolist() == [2 ** 20] * 3 + [1]
        e = dict(d, ranges=np.zeros(0, np.float32), thetas=np.zeros(0, np.float32))
        s, u, _ = check_leap(gpu_ctx, e, beam=beam, grid=grid, cl=cl)
        assert s.tolist() == [0, 0, 0, bm.OFF_GRID]
    finally:
        cl.close()
        beam.close()
        grid.close()


# ---------------------------------------------------------------------------------------------------------------- walk edges
DIRS = [(1, 0), (0, 1), (-1, 0), (0, -1), (1, 1), (-1, 1), (-1, -1), (1, -1)]


def star_case(at_far_cell):
    """41 x 41 free cells, the pose at the centre of (20, 20) with heading 0, eight max readings along the axes and the diagonals with
    a reach of 10 cells: K = 10 on each.  One cell of each walk is occupied: the far cell itself (excluded from the walk: unseen) or
    the walk's last cell, k = K - 1 (seen)."""
    cells = np.full((41, 41), -20, np.int8)
    th = np.array([-math.atan2(dy, dx) for dx, dy in DIRS], np.float32)
    rg = np.full(8, 9.0, np.float32)
    c = bc.case(cells, rg, th, [bc.centre(20, 20)], max_range=10 * bc.MPC)
    rays = bm.used_rays(c["ranges"], c["thetas"], c["params"])
    mx, my, ok = cm.far_cells(c["origin"], c["cpm"], rays, c["poses"][0], c["params"])
    assert ok.all()
    for i, (dx, dy) in enumerate(DIRS):
        step = 10 if at_far_cell else 9
        on_axis = dx == 0 or dy == 0
        if on_axis:
            assert (int(mx[i]), int(my[i])) == (20 + 10 * dx, 20 + 10 * dy)
            cells[20 + step * dy, 20 + step * dx] = 100
        else:                                                                 # (the far cell of a diagonal is 7 cells off on both axes)
            assert abs(int(mx[i]) - 20) == abs(int(my[i]) - 20) == 7
            step = 7 if at_far_cell else 6
            cells[20 + step * dy, 20 + step * dx] = 100
    return dict(c, cells=cells)


@pytest.mark.parametrize("cap", [1, 3, 64])
@pytest.mark.parametrize("at_far_cell", [True, False])
def test_obstacle_at_the_far_cell_unseen_and_one_before_it_seen(gpu_ctx, cap, at_far_cell):
    c = star_case(at_far_cell)
    _, _, seen = check_leap(gpu_ctx, c, cap=cap, casts=[0])
    e = seen[0]
    assert e["K"].tolist() == [10] * 4 + [7] * 4
    assert e["first"].tolist() == (e["K"].tolist() if at_far_cell else (e["K"] - 1).tolist())
    assert (e["p"] == bm.make_tables(c["params"], c["cpm"])["max_free" if at_far_cell else "max_blocked"]).all()


def test_a_leap_that_lands_on_the_occupied_cell_and_one_that_would_pass_the_far_cell(gpu_ctx):
    cells = np.full((9, 40), -20, np.int8)
    cells[4, 17] = 100
    th = np.array([0.0, math.pi], np.float32)                                 # along +x towards the cell, along -x over the border
    c = bc.case(cells, [5.0, 5.0], th, [bc.centre(3, 4), bc.centre(3, 4, math.pi), bc.centre(25, 4)], max_range=20 * bc.MPC)
    _, _, seen = check_leap(gpu_ctx, c, cap=7, casts=[0, 1, 2])
    assert seen[0]["first"].tolist() == [14, 19] and seen[0]["K"].tolist() == [20, 19]        # (-16.5 truncates to cell -16: K = 19)
    assert seen[0]["rounds"].tolist() == [3, 1]                               # 0 -> 7 -> 14: the leap lands on the cell; 0 -> 4, outside
    assert seen[1]["rounds"].tolist() == [1, 3]
    assert seen[2]["first"].tolist() == [20, 8] and seen[2]["rounds"].tolist() == [3, 3]      # 0 -> 7 -> 14 -> 21 > K; 0 -> 7 -> 8, the cell
    d = dict(c, params=bm.params(**dict(c["params"], max_range=10 * bc.MPC)))
    _, _, seen = check_leap(gpu_ctx, d, cap=7, casts=[0])
    assert seen[0]["first"].tolist() == [10, 9] and seen[0]["rounds"].tolist() == [2, 1]      # 0 -> 7 -> 14 > K = 10: first = K


@pytest.mark.parametrize("at_far_cell", [True, False])
def test_far_cell_of_a_4096_cell_walk(gpu_ctx, at_far_cell):
    c = ec.corridor_end(4104, at_far_cell)
    _, _, seen = check_leap(gpu_ctx, c, cap=255, casts=[0, 1])
    assert all(int(e["K"].max()) == 4096 for e in seen.values())


# ---------------------------------------------------------------------------------------------------------------- long walks
def test_open_field_with_a_reach_of_2000_cells(gpu_ctx):
    cells = np.full((3, 2100), -20, np.int8)
    c = ec.case(cells, [30.0, 150.0], [0.0, 0.0], [ec.centre(1, 1), ec.centre(50, 1, 0.002)], max_range=2000 * bc.MPC, lam=0.001, sigma_cells=100.0)
    _, _, seen = check_leap(gpu_ctx, c, cap=255, casts=[0, 1])
    assert seen[0]["K"].tolist() == [2000, 2000] and seen[0]["first"].tolist() == [2000, 2000] and seen[0]["rounds"].tolist() == [8, 8]
    _, _, seen = check_leap(gpu_ctx, c, cap=15, casts=[0])
    assert seen[0]["rounds"].tolist() == [134, 134]


@pytest.mark.parametrize("wall", [None, 4096, 4097])
def test_a_walk_of_4096_cells_on_a_4100x3_grid(gpu_ctx, wall):
    cells = np.full((3, 4100), -20, np.int8)
    if wall is not None:
        cells[:, wall] = 100                                                  # the walk's last cell (k = 4095), or the far cell
    c = ec.case(cells, [100.0, ec.LONG_RANGE], [0.0, 0.0], [ec.centre(1, 1)], **ec.LONG)
    _, _, seen = check_leap(gpu_ctx, c, cap=255, casts=[0])
    assert seen[0]["K"].tolist() == [4096, 4096]
    assert seen[0]["first"].tolist() == ([4095, 4095] if wall == 4096 else [4096, 4096])
    assert seen[0]["rounds"].tolist() == ([17, 17] if wall is None else [seen[0]["rounds"][0]] * 2) and seen[0]["rounds"][0] >= 17


def test_a_ray_grazing_a_wall_for_40_cells(gpu_ctx):
    cells = np.full((12, 64), -20, np.int8)
    cells[5, :] = 100
    c = bc.case(cells, [1.0, 5.0], [0.0, 0.0], [bc.centre(2, 6), bc.centre(2, 4), bc.centre(2, 8)], max_range=40 * bc.MPC)
    _, _, seen = check_leap(gpu_ctx, c, cap=64, casts=[0, 1, 2])
    for i in (0, 1):                                                          # every leap is one cell
        assert seen[i]["K"].tolist() == [40, 40] and seen[i]["first"].tolist() == [40, 40] and seen[i]["rounds"].tolist() == [40, 40]
    assert seen[2]["rounds"].tolist() == [14, 14]                             # three rows from the wall: leaps of 3


# ---------------------------------------------------------------------------------------------------------------- units and state
def test_span_edges_and_ties(gpu_ctx):
    c = bc.many_poses(65)
    c = dict(c, poses=np.concatenate([c["poses"], c["poses"][:3]]).astype(np.float32))            # ties
    beam, grid, cl = beam_of(gpu_ctx, c), grid_of(gpu_ctx, c), bl.ClearanceGrid(gpu_ctx, 64)
    try:
        cl.build(grid, 1)
        S, _, _ = check_leap(gpu_ctx, c, beam=beam, grid=grid, cl=cl, casts=[])
        assert S[65:].tolist() == S[:3].tolist()
        on = np.sort(S[S != bm.OFF_GRID])
        gap = int(on[-1] - on[len(on) // 2])
        assert gap > 1
        k = int(np.flatnonzero(S == on[len(on) // 2])[0])
        for span in (gap - 1, gap, gap + 1, 1, 1 << 40):
            d = dict(c, params=bm.params(**dict(c["params"], span=span)))
            beam.setParams(**{q: d["params"][q] for q in KEYS})
            _, u, _ = check_leap(gpu_ctx, d, beam=beam, grid=grid, cl=cl, casts=[], exp=S)
            assert int(u[k]) == (1 if span <= gap else int(bl.BeamModel.unitTable()[255]) if span == gap + 1 else int(u[k]))
            assert u[65:].tolist() == u[:3].tolist()
    finally:
        cl.close()
        beam.close()
        grid.close()


def test_state_refusals(gpu_ctx):
    c = bc.conditions(64, 48)
    beam, grid, cl = beam_of(gpu_ctx, c), grid_of(gpu_ctx, c), bl.ClearanceGrid(gpu_ctx, 64)
    try:
        with pytest.raises(cm.StateError):
            cm.check_state(False, 0, c["params"])
        with pytest.raises(bl.BotlabHipError, match="status 4"):
            beam.scores_leap(cl, scan_of(c), c["poses"])                      # not built
        with pytest.raises(bl.BotlabHipError, match="status 4"):
            beam.debug_leap(cl, scan_of(c), c["poses"][0])
        cl.build(grid, 1)
        with pytest.raises(bl.BotlabHipError, match="status 4"):
            beam.units(len(c["poses"]))                                       # the refusals above scored nothing
        check_leap(gpu_ctx, c, beam=beam, grid=grid, cl=cl, casts=[0])
        p = bm.params(**dict(c["params"], occ_min=2))                         # another occ_min than the grid's
        beam.setParams(**{q: p[q] for q in KEYS})
        with pytest.raises(cm.StateError):
            cm.check_state(True, 1, p)
        with pytest.raises(bl.BotlabHipError, match="status 4"):
            beam.scores_leap(cl, scan_of(c), c["poses"])
        cl.build(grid, 2)
        check_leap(gpu_ctx, dict(c, params=p), beam=beam, grid=grid, cl=cl, casts=[1])
        far = bm.params(**dict(c["params"], occ_min=2, max_range=3.0))        # another reach needs no rebuild
        beam.setParams(**{q: far[q] for q in KEYS})
        check_leap(gpu_ctx, dict(c, params=far), beam=beam, grid=grid, cl=cl, casts=[0])
        h = C.c_void_p()
        assert gpu_ctx.lib.bl_beam_create(gpu_ctx.h, C.byref(h)) == 0           # a beam model without parameters
        try:
            ls = scan_of(c).as_c()
            assert gpu_ctx.lib.bl_clearance_scores(h, cl.h, C.byref(ls), None, 0, None) == 4
            assert gpu_ctx.lib.bl_clearance_debug_cast(h, cl.h, C.byref(ls), None, None, None, None, None, None, None) == 4
        finally:
            gpu_ctx.lib.bl_beam_destroy(h)
    finally:
        cl.close()
        beam.close()
        grid.close()
