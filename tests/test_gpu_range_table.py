"""The range table on the device (bl_rangetable_*, botlab_amd/csrc/bl_rangetable.hip) and the beam model scored through it
(k_beam_lookup, bl_beam.hip) against their model (tests/range_table_model.py) on the library's own directions and tables: every entry
after a build and after an update, and the scores, the units and bl_rangetable_debug_lookup column by column.  All for equality."""
import ctypes as C
import math

import numpy as np
import pytest

import botlab_amd as bl
import beam_cases as bc
import beam_model as bm
import range_table_cases as rc
import range_table_model as rm
from test_gpu_beam import KEYS, beam_of, grid_of, scan_of

pytestmark = pytest.mark.gpu
F32 = np.float32
_TABLES = {}


def model_table(c, D, hn):
    """The model's table of a case on the directions D: the case's own when they are the model's, else (or for a beam case, which
    carries none) built once and kept."""
    if "table" in c and c.get("hn") == hn and np.array_equal(D, c["D"]):
        return c["table"]
    key = (c["cells"].tobytes(), c["cells"].shape, D.tobytes(), c["params"]["occ_min"])
    if key not in _TABLES:
        _TABLES[key] = rm.build(c["cells"], D.astype(np.int64), c["params"]["occ_min"])
        _TABLES[key].setflags(write=False)
    return _TABLES[key]


def check_build(ctx, c, rt=None, hn=None):
    """Build the case's table on the device and compare every entry and the info with the model.  Returns the model's table."""
    hn = hn or c["hn"]
    own = rt is None
    rt = bl.RangeTable(ctx, hn) if own else rt
    beam, grid = beam_of(ctx, c), grid_of(ctx, c)
    try:
        rt.build(beam, grid)
        h, w = c["cells"].shape
        reach = bm.reach_cells(c["params"], c["cpm"])
        assert rt.info() == dict(width=w, height=h, headings=hn, reach=reach, occ_min=c["params"]["occ_min"], built=1, bytes=2 * w * h * hn)
        D = rt.directions()
        exp = model_table(c, D, hn)
        got = rt.read()
        bad = np.argwhere(got != exp)
        assert len(bad) == 0, (len(bad), bad[:4].tolist(), got[tuple(bad[0])], exp[tuple(bad[0])])
        if w > 2 and h > 2:                                                   # a rectangle of rows inside
            assert np.array_equal(rt.read(1, 2 % h, w - 2, h - 2), exp[2 % h:2 % h + h - 2, 1:w - 1])
        assert rt.lastDeviceMs() > 0
        return exp
    finally:
        beam.close()
        grid.close()
        if own:
            rt.close()


@pytest.mark.parametrize("reach", [1, 3, 100, 1000, 4096])
@pytest.mark.parametrize("hn", [64, 128, 256, 512, 1024])
def test_directions_equal_the_models(gpu_ctx, reach, hn):
    c = rc.build_case(np.full((1, 1), -20, np.int8), hn, reach)
    rt, beam, grid = bl.RangeTable(gpu_ctx, hn), beam_of(gpu_ctx, c), grid_of(gpu_ctx, c)
    try:
        with pytest.raises(bl.BotlabHipError, match="status 4"):
            rt.directions()
        rt.build(beam, grid)
        assert np.array_equal(rt.directions(), rm.directions(reach, hn))
    finally:
        rt.close()
        beam.close()
        grid.close()


@pytest.mark.parametrize("case", [
    lambda: rc.single_cell(False, 1), lambda: rc.single_cell(True, 3),
    lambda: rc.strip(1, 37, 1024, 3), lambda: rc.strip(37, 1, 1024, 100), lambda: rc.strip(37, 1, 64, 1), lambda: rc.strip(1, 37, 128, 100),
    lambda: rc.room(65, 63, 128, 100), lambda: rc.room(65, 63, 128, 100, occ_min=2), lambda: rc.room(65, 63, 64, 3, occ_min=2),
    lambda: rc.room(130, 70, 64, 3), lambda: rc.room(130, 70, 64, 100), lambda: rc.room(130, 70, 128, 3),
    lambda: rc.long_reach(), lambda: rc.uniform(True), lambda: rc.uniform(False), lambda: rc.far_cell(), lambda: rc.far_cell(1024, 9)],
    ids=["1x1-free", "1x1-occupied", "1x37-Hn1024-r3", "37x1-Hn1024-r100", "37x1-r1", "1x37-Hn128-r100", "65x63-Hn128-r100", "65x63-occ2",
         "65x63-r3-occ2", "130x70-r3", "130x70-r100", "130x70-Hn128", "8x8-r4096-Hn1024", "all-occupied", "all-free", "far-cell", "far-cell-Hn1024"])
def test_build_equals_the_model(gpu_ctx, case):
    check_build(gpu_ctx, case())


def test_rebuild_on_one_handle_and_the_refusals(gpu_ctx):
    for bad in (0, 32, 63, 96, 2048, -64):
        h = C.c_void_p()
        assert gpu_ctx.lib.bl_rangetable_create(gpu_ctx.h, bad, C.byref(h)) == 2 and not h.value
    rt = bl.RangeTable(gpu_ctx, 64)
    try:
        assert rt.info() == dict(width=0, height=0, headings=64, reach=0, occ_min=0, built=0, bytes=0)
        ms = C.c_float()
        assert gpu_ctx.lib.bl_rangetable_last_device_ms(rt.h, C.byref(ms)) == 4
        with pytest.raises(bl.BotlabHipError, match="status 4"):
            rt.read(0, 0, 1, 1)
        # W * H * Hn above 2^31 entries: with Hn a power of two the least such product is (2^25 + 1) * 64; nothing is allocated
        big = bl.OccupancyGrid.from_cells(np.zeros((2761, 12153), np.int8), (F32(0), F32(0)), rc.MPC, cellsPerMeter=rc.CPM, ctx=gpu_ctx)
        assert 2761 * 12153 == 2 ** 25 + 1
        c = rc.room(130, 70, 64, 3)
        beam = beam_of(gpu_ctx, c)
        try:
            with pytest.raises(bl.BotlabHipError, match="status 2"):
                rt.build(beam, big)
            assert rt.info()["bytes"] == 0 and rt.info()["built"] == 0
            exp = check_build(gpu_ctx, c, rt=rt)
            with pytest.raises(bl.BotlabHipError, match="status 2"):
                rt.build(beam, big)                                           # the handle keeps the table it had
            assert rt.info()["built"] == 1 and np.array_equal(rt.read(), exp)
            with pytest.raises(bl.BotlabHipError, match="status 2"):
                rt.read(0, 0, 131, 1)
            with pytest.raises(bl.BotlabHipError, match="status 2"):
                rt.read(129, 69, 1, 2)
        finally:
            beam.close()
            big.close()
        check_build(gpu_ctx, rc.far_cell(), rt=rt)                            # another shape, another reach
        check_build(gpu_ctx, rc.room(65, 63, 64, 3, occ_min=2), rt=rt)        # another occ_min
        check_build(gpu_ctx, rc.room(130, 70, 64, 100), rt=rt)                # a larger table again
    finally:
        rt.close()


BOXES = {"inside": [(30, 30, None), (33, 28, None)], "corner": [(0, 0, -20), (1, 1, None)], "far-corner": [(64, 62, -20), (63, 61, None)]}


def several(cells):
    """Three occupied cells inside the walls turned free and three free ones turned occupied, far apart."""
    inner = np.zeros(cells.shape, bool)
    inner[2:-2, 2:-2] = True
    occ, free = np.argwhere(inner & (cells >= 1)), np.argwhere(inner & (cells < 1))
    assert len(occ) >= 3 and len(free) >= 3
    return ([(int(x), int(y), -20) for y, x in occ[[0, len(occ) // 2, -1]]] + [(int(x), int(y), 100) for y, x in free[[7, len(free) // 2, -9]]])


@pytest.mark.parametrize("reach,hn", [(7, 64), (100, 64)])
def test_update_equals_a_fresh_build(gpu_ctx, reach, hn):
    c = rc.room(65, 63, hn, reach)
    rt, beam, grid = bl.RangeTable(gpu_ctx, hn), beam_of(gpu_ctx, c), grid_of(gpu_ctx, c)
    try:
        rt.build(beam, grid)
        D = rt.directions().astype(np.int64)
        cells, table = c["cells"], model_table(c, D, hn)
        assert np.array_equal(rt.read(), table)
        for name, edits in list(BOXES.items()) + [("several", None)]:
            new, box = rc.changed(dict(c, cells=cells), edits if edits else several(cells))
            assert ((new >= 1) != (cells >= 1)).any()
            if name == "several":                                             # cells turned free as well as occupied
                assert ((new < 1) & (cells >= 1)).sum() == 3 and ((new >= 1) & (cells < 1)).sum() == 3
            grid.upload(new)
            fresh = rm.build(new, D, 1)
            assert not np.array_equal(fresh, table)
            if reach == 7 and name != "several":                              # the widened box is a part of the grid: the rest must stay
                assert rm.widened(box, reach, 65, 63) != (0, 0, 64, 62)
            rt.update(grid, *box)
            got = rt.read()
            bad = np.argwhere(got != fresh)
            assert len(bad) == 0, (name, len(bad), bad[:4].tolist())
            cells, table = new, fresh
        # boxes clipped on all four sides, the whole grid, and the ones that change nothing
        new, _ = rc.changed(dict(c, cells=cells), [(0, 31, -20), (64, 31, -20), (32, 0, -20), (32, 62, -20), (32, 31, None)])
        grid.upload(new)
        fresh = rm.build(new, D, 1)
        rt.update(grid, -5, -1000, 70, 2 ** 31 - 1)
        assert np.array_equal(rt.read(), fresh)
        new2, _ = rc.changed(dict(c, cells=new), [(5, 5, None), (60, 58, None)])
        grid.upload(new2)
        for box in ((3, 3, 2, 5), (0, 4, 5, 3), (-9, -9, -1, -1), (65, 0, 70, 5), (0, 63, 5, 70), (-2 ** 31, 0, -1, 62)):
            rt.update(grid, *box)                                             # empty or wholly outside: nothing is computed
        assert np.array_equal(rt.read(), fresh)
        rt.update(grid, 0, 0, 64, 62)
        assert np.array_equal(rt.read(), rm.build(new2, D, 1))
        # a map of another shape: refused, the table stays
        other = grid_of(gpu_ctx, rc.far_cell())
        try:
            keep = rt.read()
            with pytest.raises(bl.BotlabHipError, match="status 2"):
                rt.update(other, 0, 0, 5, 5)
            assert np.array_equal(rt.read(), keep)
        finally:
            other.close()
    finally:
        rt.close()
        beam.close()
        grid.close()


def test_update_before_build_is_refused(gpu_ctx):
    c = rc.uniform(False)
    rt, grid = bl.RangeTable(gpu_ctx, 64), grid_of(gpu_ctx, c)
    try:
        with pytest.raises(bl.BotlabHipError, match="status 4"):
            rt.update(grid, 0, 0, 1, 1)
    finally:
        rt.close()
        grid.close()


# ---------------------------------------------------------------------------------------------------------------- scores
def check_scores(ctx, c, hn=256, lookups=None, beam=None, grid=None, rt=None):
    """The beam case scored by table on the device beside the model: scores, units and debug_lookup of the poses `lookups` (default:
    the first 6).  Returns (scores, units, the model's table)."""
    own_b, own_g, own_t = beam is None, grid is None, rt is None
    beam = beam_of(ctx, c) if own_b else beam
    grid = grid_of(ctx, c) if own_g else grid
    rt = bl.RangeTable(ctx, hn) if own_t else rt
    try:
        if own_t:
            rt.build(beam, grid)
        t = beam.tables(c["cpm"])
        table = model_table(c, rt.directions(), hn)
        exp = rm.scores(table, c["origin"], c["cpm"], c["ranges"], c["thetas"], c["poses"], c["params"], t)
        got = beam.scores_table(rt, scan_of(c), c["poses"])
        bad = np.flatnonzero(got != exp)
        assert len(bad) == 0, (len(bad), int(bad[0]), int(got[bad[0]]), int(exp[bad[0]]))
        u = beam.units(len(c["poses"]))
        assert np.array_equal(u, bm.units(exp, c["params"]["span"], bl.BeamModel.unitTable()))
        if len(c["poses"]):
            assert beam.lastDeviceMs() > 0 and beam.debugPath() == 1
        rays = bm.used_rays(c["ranges"], c["thetas"], c["params"])
        for i in (range(min(6, len(c["poses"]))) if lookups is None else lookups):
            g = beam.debug_lookup(rt, scan_of(c), c["poses"][i])
            e = rm.lookup(table, c["origin"], c["cpm"], rays, c["poses"][i], c["params"], t)
            for col in ("h", "z", "zstar", "p"):
                want = e[col] if e is not None else np.zeros(len(rays[0]), np.int64)
                assert np.array_equal(g[col], want), (i, col, g[col].tolist(), want.tolist())
        assert np.array_equal(beam.units(len(c["poses"])), u)                 # a debug lookup leaves the last call's units and count alone
        return got, u, table
    finally:
        if own_b:
            beam.close()
        if own_g:
            grid.close()
        if own_t:
            rt.close()


def with_odd_thetas(c):
    """The case with two more rays whose thetas are not finite: dropped for every pose, as `has` drops them for the cast."""
    return dict(c, ranges=np.concatenate([c["ranges"], [F32(0.5), F32(0.7)]]).astype(np.float32),
                thetas=np.concatenate([c["thetas"], [F32("nan"), F32("inf")]]).astype(np.float32))


@pytest.mark.parametrize("hn", [64, 256, 1024])
@pytest.mark.parametrize("occ_min", [1, 2])
def test_conditions(gpu_ctx, hn, occ_min):
    """Max readings with and without an expected hit, returns short of, at and behind it, NaN and off-grid poses, dropped rays."""
    c = with_odd_thetas(bc.conditions(64, 48, occ_min=occ_min))
    s, u, table = check_scores(gpu_ctx, c, hn=hn, lookups=range(len(c["poses"])))
    assert (s == bm.OFF_GRID).sum() == 4 and s[0] == s[9]
    t = bm.make_tables(c["params"], c["cpm"])
    rays = bm.used_rays(c["ranges"], c["thetas"], c["params"])
    seen = [rm.lookup(table, c["origin"], c["cpm"], rays, p, c["params"], t) for p in c["poses"]]
    seen = [e for e in seen if e is not None]
    mx = np.concatenate([np.stack([e["zstar"][rays[2]], e["p"][rays[2]]]) for e in seen], axis=1)
    assert (mx[0] >= 0).any() and (mx[0] < 0).any() and set(mx[1].tolist()) == {t["max_blocked"], t["max_free"]}
    assert all((e["p"][-2:] == 0).all() and (e["h"][-2:] == -1).all() for e in seen)          # the two rays without an angle
    ret = np.concatenate([np.stack([e["z"][~rays[2]][:-2], e["zstar"][~rays[2]][:-2]]) for e in seen], axis=1)
    ret = ret[:, ret[1] >= 0]
    assert (ret[0] < ret[1]).any() and (ret[0] > ret[1]).any()


def test_two_walls(gpu_ctx):
    for hn in (64, 256):
        s, u, _ = check_scores(gpu_ctx, bc.two_walls(), hn=hn)
        assert s[0] > s[1] and u.tolist() == [2 ** 20, 1]


@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, 257])
def test_pose_counts(gpu_ctx, n):
    c = bc.many_poses(n)
    s, u, _ = check_scores(gpu_ctx, c, lookups=range(min(n, 2)))
    if n >= 31:
        assert (s == bm.OFF_GRID).any() and (u == 2 ** 20).sum() >= 1


@pytest.mark.parametrize("rays,stride,dropped", [(1, 1, 0), (63, 1, 0), (64, 1, 3), (65, 1, 0), (65, 3, 2), (290, 3, 0), (4096, 1, 0)])
def test_ray_counts(gpu_ctx, rays, stride, dropped):
    c = bc.ray_count(rays, stride=stride, dropped_every=dropped)
    assert len(bm.used_rays(c["ranges"], c["thetas"], c["params"])[0]) == (rays + stride - 1) // stride
    check_scores(gpu_ctx, c, lookups=[0, 2] if rays < 4096 else [0])


def test_too_many_rays_refused_and_every_ray_dropped(gpu_ctx):
    c = bc.ray_count(4097)
    beam, grid, rt = beam_of(gpu_ctx, c), grid_of(gpu_ctx, c), bl.RangeTable(gpu_ctx, 256)
    try:
        rt.build(beam, grid)
        with pytest.raises(bl.BotlabHipError, match="status 2"):
            beam.scores_table(rt, scan_of(c), c["poses"])
        d = bc.ray_count(5)
        d["ranges"] = np.array([0.0, 0.15, -2.0, float("nan"), float("inf")], np.float32)
        d["poses"] = np.concatenate([d["poses"], [bc.centre(-5, 2)]]).astype(np.float32)
        s, u, _ = check_scores(gpu_ctx, d, beam=beam, grid=grid, rt=rt)
        assert s.tolist() == [0, 0, 0, bm.OFF_GRID] and u.tolist() == [2 ** 20] * 3 + [1]
        e = dict(d, ranges=np.zeros(0, np.float32), thetas=np.zeros(0, np.float32))
        s, u, _ = check_scores(gpu_ctx, e, beam=beam, grid=grid, rt=rt)
        assert s.tolist() == [0, 0, 0, bm.OFF_GRID]
    finally:
        rt.close()
        beam.close()
        grid.close()


def test_span_edges_ties_and_hit_cut_reached_exactly(gpu_ctx):
    c = bc.many_poses(65)
    c = dict(c, poses=np.concatenate([c["poses"], c["poses"][:3]]).astype(np.float32))            # ties
    beam, grid, rt = beam_of(gpu_ctx, c), grid_of(gpu_ctx, c), bl.RangeTable(gpu_ctx, 256)
    try:
        rt.build(beam, grid)
        S, _, table = check_scores(gpu_ctx, c, beam=beam, grid=grid, rt=rt, lookups=[])
        assert S[65:].tolist() == S[:3].tolist()
        on = np.sort(S[S != bm.OFF_GRID])
        gap = int(on[-1] - on[len(on) // 2])
        assert gap > 1
        k = int(np.flatnonzero(S == on[len(on) // 2])[0])
        for span in (gap - 1, gap, gap + 1, 1, 1 << 40):
            d = dict(c, params=bm.params(**dict(c["params"], span=span)))
            beam.setParams(**{q: d["params"][q] for q in KEYS})
            _, u, _ = check_scores(gpu_ctx, d, beam=beam, grid=grid, rt=rt, lookups=[])
            assert int(u[k]) == (1 if span <= gap else int(bl.BeamModel.unitTable()[255]) if span == gap + 1 else int(u[k]))
        # |z - z*| of some ray as hit_cut, and one either side
        t = bm.make_tables(c["params"], c["cpm"])
        rays = bm.used_rays(c["ranges"], c["thetas"], c["params"])
        i = next(i for i in range(len(c["poses"])) if S[i] != bm.OFF_GRID)
        g = rm.lookup(table, c["origin"], c["cpm"], rays, c["poses"][i], c["params"], t)
        dz = np.abs(g["z"] - g["zstar"])[(g["z"] >= 0) & (g["zstar"] >= 0)]
        cut = int(dz[(dz >= 2) & (dz <= 1022)][0])
        for hc in (cut - 1, cut, cut + 1):
            d = dict(c, params=bm.params(**dict(c["params"], hit_cut=hc)))
            beam.setParams(**{q: d["params"][q] for q in KEYS})
            check_scores(gpu_ctx, d, beam=beam, grid=grid, rt=rt, lookups=[i])
    finally:
        rt.close()
        beam.close()
        grid.close()


def test_short_clamp_needs_a_long_reach(gpu_ctx):
    """Short[min(z >> 2, 1023)]: z >> 2 reaches 1023 only for a return beyond 1023 cells, so the reach is 2000 cells -- on an 8 x 8 grid,
    since z comes from the range alone.  Without the clamp the index would leave the table."""
    cells = np.full((8, 8), -20, np.int8)
    cells[4, 6] = 100
    cell = rc.MPC
    rg = np.array([1022.9 * cell, 1023.0 * cell, 1023.3 * cell, 1500 * cell, 1999.4 * cell, 2100 * cell, 3.5 * cell, 5 * cell], np.float32)
    th = np.array([1.0, 2.0, 3.0, -1.0, -2.0, 0.5, 0.0, 0.0], np.float32)
    c = bc.case(cells, rg, th, [bc.centre(2, 4), bc.centre(1, 1, 0.3)], max_range=rc.range_for(2000), lam=0.001)
    s, u, table = check_scores(gpu_ctx, c, hn=64)
    t = bm.make_tables(c["params"], c["cpm"])
    assert t["short"][1022] > t["short"][1023] > 1000                         # (a decay slow enough for the clamp to show in p)
    e = rm.lookup(table, c["origin"], c["cpm"], bm.used_rays(c["ranges"], c["thetas"], c["params"]), c["poses"][0], c["params"], t)
    assert {1022, 1023, 1500} <= set((e["z"] >> 2).tolist()) and (e["z"] >> 2).max() > 1023
    assert e["zstar"][6] == 16 and e["z"][6] < e["zstar"][6] < e["z"][7] and e["z"][5] == -1 and (e["zstar"][:5] == -1).all()


def test_state_refusals(gpu_ctx):
    c = bc.conditions(64, 48)
    beam, grid, rt = beam_of(gpu_ctx, c), grid_of(gpu_ctx, c), bl.RangeTable(gpu_ctx, 256)
    try:
        with pytest.raises(bl.BotlabHipError, match="status 4"):
            beam.scores_table(rt, scan_of(c), c["poses"])                     # not built
        with pytest.raises(bl.BotlabHipError, match="status 4"):
            beam.debug_lookup(rt, scan_of(c), c["poses"][0])
        rt.build(beam, grid)
        with pytest.raises(bl.BotlabHipError, match="status 4"):
            beam.units(len(c["poses"]))                                       # the refusals above scored nothing
        check_scores(gpu_ctx, c, beam=beam, grid=grid, rt=rt, lookups=[0])
        for change in (dict(occ_min=2), dict(max_range=1.6), dict(max_range=300.0)):
            p = bm.params(**dict(c["params"], **change))
            beam.setParams(**{q: p[q] for q in KEYS})
            with pytest.raises(rm.StateError):
                rm.check_state(True, 1, 30, c["cpm"], p)
            with pytest.raises(bl.BotlabHipError, match="status 4"):
                beam.scores_table(rt, scan_of(c), c["poses"])
        same = bm.params(**dict(c["params"], max_range=1.46, sigma_cells=2.0))                  # another range, the same reach: accepted
        beam.setParams(**{q: same[q] for q in KEYS})
        rm.check_state(True, 1, 30, c["cpm"], same)
        check_scores(gpu_ctx, dict(c, params=same), beam=beam, grid=grid, rt=rt, lookups=[0])
        h = C.c_void_p()
        assert gpu_ctx.lib.bl_beam_create(gpu_ctx.h, C.byref(h)) == 0           # a beam model without parameters
        try:
            ls = scan_of(c).as_c()
            assert gpu_ctx.lib.bl_rangetable_scores(h, rt.h, C.byref(ls), None, 0, None) == 4
            assert gpu_ctx.lib.bl_rangetable_build(rt.h, h, grid.h) == 4
        finally:
            gpu_ctx.lib.bl_beam_destroy(h)
    finally:
        rt.close()
        beam.close()
        grid.close()


def test_cast_and_table_alternate_on_one_handle(gpu_ctx):
    """Both scoring forms through one handle's buffers, closing launches and state, turn and turn about: 1 pose, 33 (two workgroups,
    the second with one pose) and none; 65 used rays (a lane takes two) and none; a debug call of either form between two scoring
    calls.  After every call the scores and units are the model's, a wrong count is refused and the device time answers."""
    cells = bc.room(16, 12)
    cells[3:9, 6] = 100
    cells[8, 9:13] = 100
    cells[2, 11] = 1
    rg, th = bc.octant_scan(65, r0=0.16, dr=0.04)
    rng = np.random.default_rng(11)
    poses = np.stack([rng.uniform(-0.05, 16 * rc.MPC + 0.05, 33), rng.uniform(-0.05, 12 * rc.MPC + 0.05, 33), rng.uniform(-3.1, 3.1, 33)], axis=1)
    poses[0], poses[32] = bc.centre(3, 4, 0.4), bc.centre(12, 3, -2.0)
    c = bc.case(cells, rg, th, poses, max_range=0.5)
    none = dict(c, ranges=np.array([0.1, float("nan"), 0.0], np.float32), thetas=np.zeros(3, np.float32))
    assert len(bm.used_rays(c["ranges"], c["thetas"], c["params"])[0]) == 65 and len(bm.used_rays(none["ranges"], none["thetas"], c["params"])[0]) == 0
    beam, grid, rt = beam_of(gpu_ctx, c), grid_of(gpu_ctx, c), bl.RangeTable(gpu_ctx, 64)
    try:
        rt.build(beam, grid)
        t = beam.tables(c["cpm"])
        table = rm.build(c["cells"], rt.directions().astype(np.int64), c["params"]["occ_min"])
        U = bl.BeamModel.unitTable()

        def units_answer(exp, n):
            assert np.array_equal(beam.units(n), bm.units(exp, c["params"]["span"], U))
            with pytest.raises(bl.BotlabHipError, match="status 2"):
                beam.units(n + 1)
            assert beam.lastDeviceMs() > 0

        def score(form, d, n):
            p = d["poses"][:n]
            if form == "cast":
                got = beam.scores(grid, scan_of(d), p)
                exp = bm.scores(d["cells"], d["origin"], d["cpm"], d["ranges"], d["thetas"], p, d["params"], t)
            else:
                got = beam.scores_table(rt, scan_of(d), p)
                exp = rm.scores(table, d["origin"], d["cpm"], d["ranges"], d["thetas"], p, d["params"], t)
            assert got.tolist() == exp.tolist(), (form, n)
            units_answer(exp, n)
            return exp

        rays = bm.used_rays(c["ranges"], c["thetas"], c["params"])
        s33 = score("cast", c, 33)
        assert (s33 == bm.OFF_GRID).any() and (s33 != bm.OFF_GRID).sum() > 20 and s33[32] != bm.OFF_GRID
        s1 = score("table", c, 1)
        g = beam.debug_cast(grid, scan_of(c), c["poses"][32])                 # a debug call of the other form in between
        e = bm.cast(c["cells"], c["origin"], c["cpm"], rays, c["poses"][32], c["params"], t)
        assert all(np.array_equal(g[k], e[k]) for k in ("first", "K", "z", "zstar", "p")) and (e["first"] < e["K"]).any()
        units_answer(s1, 1)                                                   # ... leaves the scoring call before it standing
        score("cast", c, 0)
        st = score("table", c, 33)
        g = beam.debug_lookup(rt, scan_of(c), c["poses"][0])
        e = rm.lookup(table, c["origin"], c["cpm"], rays, c["poses"][0], c["params"], t)
        assert all(np.array_equal(g[k], e[k]) for k in ("h", "z", "zstar", "p")) and (e["zstar"] >= 0).any()
        units_answer(st, 33)
        assert score("cast", none, 1).tolist() == [0]
        sn = score("table", none, 33)
        assert set(sn.tolist()) == {0, bm.OFF_GRID}
        assert beam.debug_cast(grid, scan_of(none), c["poses"][0])["p"].tolist() == []
        units_answer(sn, 33)
        score("table", c, 0)
        assert score("cast", c, 33).tolist() == s33.tolist()
        assert score("cast", c, 1).tolist() == s33[:1].tolist()
        assert score("table", c, 33).tolist() == st.tolist()
    finally:
        rt.close()
        beam.close()
        grid.close()
