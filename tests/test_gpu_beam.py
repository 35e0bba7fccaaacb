"""The beam model on the device (bl_beam_*, botlab_amd/csrc/bl_beam.hip) against its model (tests/beam_model.py) on the library's own
tables: the scores of every pose, the units, and the per-ray values of bl_beam_debug_cast column by column."""
import numpy as np
import pytest

import botlab_amd as bl
import beam_cases as bc
import beam_model as bm

pytestmark = pytest.mark.gpu
F32 = np.float32
KEYS = ("max_range", "occ_min", "sigma_cells", "z_hit", "z_short", "z_max", "z_rand", "lam", "blocked_factor", "hit_cut", "span", "ray_stride")


def scan_of(c):
    return bl.LidarScan(c["ranges"], c["thetas"], np.zeros(len(c["ranges"]), np.int64))


def grid_of(ctx, c):
    return bl.OccupancyGrid.from_cells(c["cells"], c["origin"], c["mpc"], cellsPerMeter=c["cpm"], ctx=ctx)


def beam_of(ctx, c):
    return bl.BeamModel(ctx=ctx, **{k: c["params"][k] for k in KEYS})


def same_tables(got, exp):
    for k in ("hit", "short", "lt"):
        assert np.array_equal(got[k], exp[k]), k
    assert {k: got[k] for k in ("rand", "max_free", "max_blocked", "ln2", "reach")} == {k: exp[k] for k in ("rand", "max_free", "max_blocked", "ln2", "reach")}


def check(ctx, c, casts=None, path=None, beam=None, grid=None):
    """The case on the device beside the model: tables, scores, units, and debug_cast of the poses `casts` (default: the first 6).
    path: what bl_beam_debug_path must say after the scores call.  Returns (scores, units)."""
    own_b, own_g = beam is None, grid is None
    beam = beam_of(ctx, c) if own_b else beam
    grid = grid_of(ctx, c) if own_g else grid
    try:
        t = beam.tables(c["cpm"])
        same_tables(t, bm.make_tables(c["params"], c["cpm"]))
        U = bl.BeamModel.unitTable()
        exp = bm.scores(c["cells"], c["origin"], c["cpm"], c["ranges"], c["thetas"], c["poses"], c["params"], t)
        got = beam.scores(grid, scan_of(c), c["poses"])
        bad = np.flatnonzero(got != exp)
        assert len(bad) == 0, (len(bad), int(bad[0]), int(got[bad[0]]), int(exp[bad[0]]))
        if path is not None and len(c["poses"]):
            assert beam.debugPath() == path
        u = beam.units(len(c["poses"]))
        assert np.array_equal(u, bm.units(exp, c["params"]["span"], U))
        rays = bm.used_rays(c["ranges"], c["thetas"], c["params"])
        for i in (range(min(6, len(c["poses"]))) if casts is None else casts):
            g = beam.debug_cast(grid, scan_of(c), c["poses"][i])
            e = bm.cast(c["cells"], c["origin"], c["cpm"], rays, c["poses"][i], c["params"], t)
            for col in ("first", "K", "z", "zstar", "p"):
                want = e[col] if e is not None else np.zeros(len(rays[0]), np.int64)
                assert np.array_equal(g[col], want), (i, col, g[col].tolist(), want.tolist())
        assert np.array_equal(beam.units(len(c["poses"])), u)             # a debug cast leaves the last call's units and count alone
        return got, u
    finally:
        if own_b:
            beam.close()
        if own_g:
            grid.close()


@pytest.mark.parametrize("w,h,occ_min", [(64, 48, 1), (64, 48, 2), (130, 70, 1), (37, 23, 1)])
def test_conditions_staged_and_direct(gpu_ctx, w, h, occ_min):
    c = bc.conditions(w, h, occ_min=occ_min)
    a, _ = check(gpu_ctx, c, casts=range(len(c["poses"])), path=1)      # the default: the grid read directly
    assert (a == bm.OFF_GRID).sum() == 4 and a[0] == a[9]                 # off the grid, NaN, inf; a tie between equal poses
    beam = beam_of(gpu_ctx, c)
    try:
        beam.debugSet(stage_windows=True)
        b, _ = check(gpu_ctx, c, casts=range(len(c["poses"])), path=0, beam=beam)
        beam.debugSet(stage_windows=True, window_bytes=4096)              # 130 x 70 does not fit; the small grids' windows do
        d, _ = check(gpu_ctx, c, casts=[0, 1], path=(1 if w * h > 4096 else 0), beam=beam)
        assert np.array_equal(a, b) and np.array_equal(a, d)
    finally:
        beam.close()


@pytest.mark.parametrize("reach", [63, 64, 65, 130])
@pytest.mark.parametrize("wall", [False, True])
def test_walk_lengths(gpu_ctx, reach, wall):
    w, h = (130, 70) if reach == 130 else (64, 48)
    c = bc.open_field(w, h, reach, wall_x=(w - 7 if wall else None))
    t = bm.make_tables(c["params"], c["cpm"])
    g = bm.cast(c["cells"], c["origin"], c["cpm"], bm.used_rays(c["ranges"], c["thetas"], c["params"]), c["poses"][0], c["params"], t)
    assert reach in g["K"].tolist()
    assert (g["first"] == g["K"]).all() != wall
    check(gpu_ctx, c)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_pose_counts(gpu_ctx, n):
    c = bc.many_poses(n)
    s, u = check(gpu_ctx, c, casts=range(min(n, 2)))
    if n >= 63:
        assert (s == bm.OFF_GRID).any() and (u == 1).sum() >= (s == bm.OFF_GRID).sum() and (u == 2 ** 20).sum() >= 1
    if n == 257:                                                          # scattered over a 64 x 48 grid: 2 KB windows, staged where they fit
        beam = beam_of(gpu_ctx, c)
        beam.debugSet(stage_windows=True, window_bytes=2048)
        try:
            check(gpu_ctx, bc.many_poses(257, seed=9), casts=[], beam=beam)
            print("257 scattered poses, 2 KB windows: path", beam.debugPath())
            check(gpu_ctx, c, casts=[], beam=beam, path=None)
            beam.debugSet(stage_windows=True)
            check(gpu_ctx, c, casts=[], beam=beam, path=0)                # the whole 64 x 48 grid fits every workgroup's window
        finally:
            beam.close()


def test_one_launch_with_both_paths(gpu_ctx):
    """130 x 70, a reach of 10 cells, 2 KB windows: the first workgroup's 32 poses stand within two cells of each other (a window of
    about 27 x 27), the second's are scattered over the grid (no window fits)."""
    c = bc.conditions(130, 70, max_range=0.5)
    rng = np.random.default_rng(4)
    near = [bc.centre(64 + k % 2, 35 + (k // 2) % 2, 0.2 * k) for k in range(32)]
    far = [bc.centre(int(rng.integers(1, 129)), int(rng.integers(1, 69)), float(rng.uniform(-3, 3))) for _ in range(32)]
    far[0], far[1] = bc.centre(1, 1), bc.centre(128, 68)
    c = dict(c, poses=np.array(near + far, np.float32))
    beam = beam_of(gpu_ctx, c)
    try:
        beam.debugSet(stage_windows=True, window_bytes=2048)
        check(gpu_ctx, c, casts=[0, 33], path=2, beam=beam)
    finally:
        beam.close()


@pytest.mark.parametrize("rays,stride,dropped", [(1, 1, 0), (63, 1, 0), (64, 1, 3), (65, 1, 0), (290, 1, 5), (65, 3, 2), (290, 3, 0), (4096, 1, 0)])
def test_ray_counts(gpu_ctx, rays, stride, dropped):
    c = bc.ray_count(rays, stride=stride, dropped_every=dropped)
    assert len(bm.used_rays(c["ranges"], c["thetas"], c["params"])[0]) == (rays + stride - 1) // stride
    check(gpu_ctx, c, casts=[0, 2] if rays < 4096 else [0])


def test_too_many_rays_refused_and_every_ray_dropped(gpu_ctx):
    c = bc.ray_count(4097)
    with pytest.raises(bm.ArgError):
        bm.used_rays(c["ranges"], c["thetas"], c["params"])
    beam, grid = beam_of(gpu_ctx, c), grid_of(gpu_ctx, c)
    try:
        with pytest.raises(bl.BotlabHipError, match="status 2"):
            beam.scores(grid, scan_of(c), c["poses"])
        c3 = bc.ray_count(4097, stride=3)                                # 1366 used rays
        check(gpu_ctx, c3, casts=[0])
        d = bc.ray_count(5)
        d["ranges"] = np.array([0.0, 0.15, -2.0, float("nan"), float("inf")], np.float32)
        d["poses"] = np.concatenate([d["poses"], [bc.centre(-5, 2)]]).astype(np.float32)
        s, u = check(gpu_ctx, d, beam=beam, grid=grid)
        assert s.tolist() == [0, 0, 0, bm.OFF_GRID] and u.tolist() == [2 ** 20] * 3 + [1]
        e = dict(d, ranges=np.zeros(0, np.float32), thetas=np.zeros(0, np.float32))
        s, u = check(gpu_ctx, e, beam=beam, grid=grid)
        assert s.tolist() == [0, 0, 0, bm.OFF_GRID]
    finally:
        beam.close()
        grid.close()


def test_two_walls(gpu_ctx):
    c = bc.two_walls()
    s, u = check(gpu_ctx, c)
    assert s[0] > s[1] and u.tolist() == [2 ** 20, 1]


def test_span_edges_and_hit_cut_reached_exactly(gpu_ctx):
    c = bc.many_poses(65)
    t = bm.make_tables(c["params"], c["cpm"])
    S = bm.scores(c["cells"], c["origin"], c["cpm"], c["ranges"], c["thetas"], c["poses"], c["params"], t)
    on = np.sort(S[S != bm.OFF_GRID])
    gap = int(on[-1] - on[len(on) // 2])
    assert gap > 1
    grid = grid_of(gpu_ctx, c)
    try:
        for span in (gap - 1, gap, gap + 1, 1, 1 << 40):
            d = dict(c, params=bm.params(**dict(c["params"], span=span)))
            _, u = check(gpu_ctx, d, casts=[], grid=grid)
            k = int(np.flatnonzero(S == on[len(on) // 2])[0])
            assert int(u[k]) == (1 if span <= gap else int(bl.BeamModel.unitTable()[255]) if span == gap + 1 else int(u[k]))
        # |z - z*| of some ray of pose 0 as hit_cut, and one either side
        rays = bm.used_rays(c["ranges"], c["thetas"], c["params"])
        i = next(i for i in range(len(c["poses"])) if S[i] != bm.OFF_GRID)
        g = bm.cast(c["cells"], c["origin"], c["cpm"], rays, c["poses"][i], c["params"], t)
        d = np.abs(g["z"] - g["zstar"])[(g["z"] >= 0) & (g["zstar"] >= 0)]
        cut = int(d[(d >= 2) & (d <= 1022)][0])
        for hc in (cut - 1, cut, cut + 1):
            check(gpu_ctx, dict(c, params=bm.params(**dict(c["params"], hit_cut=hc))), casts=[i], grid=grid)
    finally:
        grid.close()


def test_handle_parameters_maps_and_errors(gpu_ctx):
    c = bc.conditions(64, 48)
    lib = gpu_ctx.lib
    h = __import__("ctypes").c_void_p()
    assert lib.bl_beam_create(gpu_ctx.h, __import__("ctypes").byref(h)) == 0
    grid = grid_of(gpu_ctx, c)
    out = np.zeros(len(c["poses"]), np.int64)
    hp = np.zeros(len(c["poses"]), bl.POSE_DTYPE)
    ls = scan_of(c).as_c()
    import ctypes as C
    assert lib.bl_beam_scores(h, grid.h, C.byref(ls), hp.ctypes.data, len(hp), out.ctypes.data) == 4      # no parameters yet
    assert lib.bl_beam_tables(h, C.c_float(20.0), None, None, None, None) == 4
    assert lib.bl_beam_debug_path(h) == -1 and lib.bl_beam_last_rays(h) == -1
    assert lib.bl_beam_units(h, out.ctypes.data, 1) == 4
    ms = C.c_float()
    assert lib.bl_beam_last_device_ms(h, C.byref(ms)) == 4
    lib.bl_beam_destroy(h)
    beam = beam_of(gpu_ctx, c)
    try:
        before = beam.tables(c["cpm"])
        for bad in (dict(z_rand=0.0), dict(z_max=0.0), dict(blocked_factor=0.0), dict(z_hit=1.5, z_rand=0.6), dict(hit_cut=0),
                    dict(hit_cut=1024), dict(span=0), dict(ray_stride=0), dict(ray_stride=65), dict(occ_min=128), dict(sigma_cells=0.0),
                    dict(max_range=0.15), dict(max_range=float("nan")), dict(lam=-1.0)):
            p = bm.params(**dict(c["params"], **bad))
            assert not bm.params_ok(p), bad
            with pytest.raises(bl.BotlabHipError, match="status 2"):
                beam.setParams(**{k: p[k] for k in KEYS})
        same_tables(beam.tables(c["cpm"]), before)                        # the handle keeps its own
        check(gpu_ctx, c, beam=beam, grid=grid)
        # new parameters on one handle
        c2 = dict(c, params=bm.params(**dict(c["params"], sigma_cells=2.5, z_hit=0.5, lam=0.3, hit_cut=17, ray_stride=2, occ_min=2, max_range=0.9)))
        beam.setParams(**{k: c2["params"][k] for k in KEYS})
        check(gpu_ctx, c2, beam=beam, grid=grid)
        # the same grid uploaded again with other contents, then a smaller one
        c3 = dict(c2, cells=np.ascontiguousarray(np.where(c2["cells"] > 0, -20, c2["cells"])[::-1, ::-1]))
        c3["cells"][20:24, 10:50] = 100
        grid.upload(c3["cells"])
        check(gpu_ctx, c3, beam=beam, grid=grid)
        c4 = bc.conditions(37, 23)
        c4 = dict(c4, params=c2["params"])
        check(gpu_ctx, c4, beam=beam)
        with pytest.raises(bl.BotlabHipError, match="status 2"):
            beam.units(len(c4["poses"]) + 1)                               # not the last call's count
        # a reach beyond 4096 cells is refused by the call, not by set_params
        far = bm.params(**dict(c["params"], max_range=300.0))
        beam.setParams(**{k: far[k] for k in KEYS})
        with pytest.raises(bl.BotlabHipError, match="status 2"):
            beam.scores(grid, scan_of(c), c["poses"])
        with pytest.raises(bl.BotlabHipError, match="status 2"):
            beam.tables(c["cpm"])
        assert beam.lastDeviceMs() > 0
    finally:
        beam.close()
        grid.close()
