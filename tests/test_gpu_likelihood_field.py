"""The likelihood field on the GPU (bl_lfield_*, botlab_amd/csrc/bl_lfield.hip) against its model (tests/likelihood_field_model.py), and
the particle filter and the scan matcher on a field against their own oracles given the model field as the map.  Every device
comparison is np.array_equal: no tolerance, no cell left out."""
import ctypes as C

import numpy as np
import pytest

import botlab_amd as bl
from botlab_amd import _capi, synth
import helpers
import likelihood_field_model as lm
import scan_match_model as sm
import scan_match_prior_model as smp

pytestmark = pytest.mark.gpu
CPM = helpers.CPM_DEFAULT
ORIGIN = (np.float32(-5.0), np.float32(-5.0))
MPC = np.float32(0.05)


def _grid(ctx, cells, origin=ORIGIN, mpc=MPC):
    return bl.OccupancyGrid.from_cells(np.ascontiguousarray(cells, np.int8), origin, np.float32(mpc), cellsPerMeter=CPM, ctx=ctx)


def _check(ctx, lf_by_key, cells, sigma, R, occ_min=1, peak=127):
    """One compute against the model; the handles are kept per parameter set, so most computes run on a used handle."""
    assert not lm.near_half(sigma, R, MPC, peak)
    key = (sigma, R, occ_min, peak)
    if key not in lf_by_key:
        lf_by_key[key] = bl.LikelihoodField(sigma=sigma, max_cells=R, occ_min=occ_min, peak=peak, ctx=ctx)
    g = _grid(ctx, cells)
    got = lf_by_key[key].compute(g).cells()
    exp = lm.field(cells, sigma, R, MPC, occ_min, peak)
    g.close()
    assert got.dtype == np.int8 and got.shape == exp.shape
    assert np.array_equal(got, exp), (cells.shape, key, int((got != exp).sum()), np.argwhere(got != exp)[:4].tolist())
    return got


@pytest.fixture()
def fields():
    d = {}
    yield d
    for lf in d.values():
        lf.close()


@pytest.mark.parametrize("shape", [(1, 1), (1, 37), (37, 1), (63, 65), (130, 129)])
def test_small_and_tile_edge_shapes(gpu_ctx, fields, shape):
    h, w = shape
    rng = np.random.default_rng(h * 1000 + w)
    none = np.full((h, w), -50, np.int8)
    inputs = [none, np.zeros((h, w), np.int8), np.full((h, w), 100, np.int8)]       # no source (free, unknown), all sources
    for cy, cx in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):
        c = none.copy()
        c[cy, cx] = 1
        inputs.append(c)
    for density in (0.001, 0.03, 0.5):
        inputs.append(np.where(rng.random((h, w)) < density, 77, rng.integers(-3, 1, (h, w))).astype(np.int8))     # 0 and -1: never sources
    for R in (1, 3, 64):
        for k, cells in enumerate(inputs):
            got = _check(gpu_ctx, fields, cells, 0.1, R)
            if k < 2:
                assert (got == 0).all()
            if k == 2:
                assert (got == 127).all()
    # the two sigma extremes: sources only, and the disc indicator (the FAR edge)
    for cells in inputs[3:]:
        assert np.array_equal(_check(gpu_ctx, fields, cells, 0.01, 3), np.where(cells >= 1, 127, 0))
        got = _check(gpu_ctx, fields, cells, 10.0, 3)
        assert set(np.unique(got).tolist()) <= {0, 127}


@pytest.mark.parametrize("occ_min", [1, 127])
@pytest.mark.parametrize("peak", [1, 127])
def test_threshold_and_peak(gpu_ctx, fields, occ_min, peak):
    """Cells holding exactly occ_min - 1 and occ_min side by side: only the second kind is a source."""
    rng = np.random.default_rng(occ_min + peak)
    for h, w in ((63, 65), (130, 129)):
        cells = rng.choice(np.array([-128, -1, 0, occ_min - 1, occ_min], np.int8), size=(h, w), p=[0.3, 0.2, 0.2, 0.27, 0.03])
        cells[h // 2, w // 2 - 1], cells[h // 2, w // 2] = occ_min - 1, occ_min
        for R in (1, 3, 64):
            got = _check(gpu_ctx, fields, cells, 0.1, R, occ_min, peak)
            assert got.max() == peak and got.min() == 0 and (got[cells >= occ_min] == peak).all()
            if lm.table(0.1, R, MPC, peak)[1] < peak:
                assert np.array_equal(got == peak, cells >= occ_min)


def test_golden_maps_and_table(maps, gpu_ctx, fields):
    """All 14 golden maps at sigma = 0.10, R = 6; table() is the model's table."""
    sizes = set()
    for name in helpers.ALL_MAPS:
        cells = maps[name]["cells"]
        sizes.add(cells.shape)
        _check(gpu_ctx, fields, cells, 0.1, 6)
    assert len(helpers.ALL_MAPS) == 14 and sizes == {(200, 200), (300, 300)}
    for key, lf in fields.items():
        sigma, R, occ_min, peak = key
        assert not lm.near_half(sigma, R, MPC, peak)
        t = lf.table()
        assert t.dtype == np.int8 and np.array_equal(t, lm.table(sigma, R, MPC, peak))
    for sigma, R, peak, mpc in ((0.1, 64, 127, 0.05), (0.25, 20, 100, 0.1), (0.01, 6, 127, 0.05), (10.0, 6, 127, 0.05)):
        assert not lm.near_half(sigma, R, mpc, peak)
        lf = bl.LikelihoodField(sigma=sigma, max_cells=R, peak=peak, ctx=gpu_ctx)
        g = _grid(gpu_ctx, maps["astar_maze"]["cells"], mpc=mpc)
        lf.compute(g)
        assert np.array_equal(lf.table(), lm.table(sigma, R, mpc, peak))
        assert lf.lastDeviceMs() > 0.0
        lf.close()
        g.close()


def test_params_states_and_default_cap(maps, gpu_ctx):
    lib = gpu_ctx.lib
    h = C.c_void_p()
    _capi.check(lib.bl_lfield_create(gpu_ctx.h, C.byref(h)))
    g = _grid(gpu_ctx, maps["astar_maze"]["cells"])
    n, ms = C.c_int(), C.c_float()
    assert lib.bl_lfield_grid(h) is None
    assert lib.bl_lfield_compute(h, g.h) == _capi.BL_ERR_STATE                         # no parameters yet
    assert lib.bl_lfield_table(h, None, C.byref(n)) == _capi.BL_ERR_STATE
    assert lib.bl_lfield_last_device_ms(h, C.byref(ms)) == _capi.BL_ERR_STATE
    good = _capi.LFieldParams(0.1, 6, 1, 127)
    _capi.check(lib.bl_lfield_set_params(h, C.byref(good)))
    for bad in ((0.0, 6, 1, 127), (-0.1, 6, 1, 127), (float("nan"), 6, 1, 127), (float("inf"), 6, 1, 127), (0.1, 0, 1, 127), (0.1, 65, 1, 127),
                (0.1, 6, 0, 127), (0.1, 6, 128, 127), (0.1, 6, 1, 0), (0.1, 6, 1, 128)):
        assert lib.bl_lfield_set_params(h, C.byref(_capi.LFieldParams(*bad))) == _capi.BL_ERR_ARG, bad
    _capi.check(lib.bl_lfield_compute(h, g.h))                                          # the handle kept what it had
    _capi.check(lib.bl_lfield_table(h, None, C.byref(n)))
    assert n.value == 38
    out = np.empty((200, 200), np.int8)
    _capi.check(lib.bl_grid_download(lib.bl_lfield_grid(h), out.ctypes.data))
    assert np.array_equal(out, lm.field(maps["astar_maze"]["cells"], 0.1, 6, MPC))
    lib.bl_lfield_destroy(h)
    lf = bl.LikelihoodField(sigma=0.1, ctx=gpu_ctx)                                      # max_cells None: ceil(3 sigma cpm) = 6 at 5 cm
    f = lf.compute(g)
    assert lf.max_cells == 6 and len(lf.table()) == 38 and f is lf.grid()
    assert (f.width, f.height, f.mpc, f.cpm, f.origin) == (g.width, g.height, g.mpc, g.cpm, g.origin)
    f.close()                                                                           # does not own the handle: a no-op for the library
    f = lf.compute(g)
    assert np.array_equal(f.cells(), out)
    lf.close()
    g.close()


def test_shape_change_on_one_handle(maps, gpu_ctx):
    lf = bl.LikelihoodField(sigma=0.1, max_cells=6, ctx=gpu_ctx)
    a = maps["obstacle_slam_10mx10m_5cm"]["cells"]
    rng = np.random.default_rng(3)
    b = np.where(rng.random((130, 129)) < 0.02, 90, -9).astype(np.int8)
    ga, gb = _grid(gpu_ctx, a), _grid(gpu_ctx, b, origin=(np.float32(-1.0), np.float32(-2.0)))
    fa = lf.compute(ga)
    assert np.array_equal(fa.cells(), lm.field(a, 0.1, 6, MPC)) and lf.compute(ga) is fa
    fb = lf.compute(gb)
    assert (fb.width, fb.height) == (129, 130) and fb.origin == gb.origin
    assert np.array_equal(fb.cells(), lm.field(b, 0.1, 6, MPC))
    fa2 = lf.compute(ga)                                                                # and back, larger again
    assert np.array_equal(fa2.cells(), lm.field(a, 0.1, 6, MPC))
    for x in (lf, ga, gb):
        x.close()


# ------------------------------------------------------------------ the particle filter on a field
from test_gpu_parity import _assert_estimate_bit_equal, _mcl_sequence  # noqa: E402


def _step(oracle, opf, pf, m_frame, k, scan, o, rand, field_cells, field_grid):
    """One update on both sides; resample indices and half-unit likelihoods exact, the pose estimate bit-equal."""
    mpc, origin = m_frame
    t = int(scan.times[-1])
    res = opf.update(oracle.pose(o[0], o[1], o[2], utime=t), scan, field_cells, mpc, CPM, origin, rand)
    pose = pf.updateFilter(bl.make_pose(o[0], o[1], o[2], utime=t), scan, field_grid, rand_value=rand, noise=res["noise"])
    assert pose.utime == res["pose"].utime == t
    if res["moved"]:
        idx, like = pf.debugLast()
        assert np.array_equal(idx, res["idx"]), f"resample indices differ at step {k}"
        assert np.array_equal(like.astype(np.float64) * 0.5, res["raw"]), f"likelihoods differ at step {k}"
        _assert_estimate_bit_equal(pose, res["pose"], k)
    return bool(res["moved"]), res["raw"]


@pytest.mark.parametrize("N", [200, 4096])
def test_filter_on_a_field_matches_the_oracle_on_the_model_field(oracle, maps, gpu_ctx, N):
    m, g, opf, pf, odo, scans, rands, cells = _mcl_sequence(oracle, maps, gpu_ctx, N, 10)
    lf = bl.LikelihoodField(sigma=0.1, max_cells=6, ctx=gpu_ctx)
    fg = lf.compute(g)
    fcells = lm.field(cells, 0.1, 6, m["mpc"])
    moved_updates = 0
    for k, scan in enumerate(scans):
        o = odo[k + 1] if k != 4 else odo[k]              # step 4 repeats the odometry: "robot did not move" branch
        moved, raw = _step(oracle, opf, pf, (m["mpc"], m["origin"]), k, scan, o, rands[k], fcells, fg)
        moved_updates += moved
    assert moved_updates >= 7 and raw.max() > 0
    for x in (pf, lf, g):
        x.close()


@pytest.mark.parametrize("big", [False, True])
def test_filter_sees_a_recomputed_field(oracle, maps, gpu_ctx, big):
    """Three moved updates on the first field, a map update on the real grid, compute on the same handle, three more updates: they
    equal the oracle on the SECOND field.  big: the map inside a 320 x 300 grid, too large to be staged whole in LDS, so that the filter
    cuts its window out of the zero-framed mirror -- which a compute must mark stale."""
    N = 200
    m, g, opf, pf, odo, scans, rands, cells = _mcl_sequence(oracle, maps, gpu_ctx, N, 7)
    mpc, origin = m["mpc"], m["origin"]
    if big:
        g.close()
        wide = np.zeros((300, 320), np.int8)
        wide[50:250, 60:260] = cells
        cells = wide
        origin = (np.float32(-8.0), np.float32(-7.5))                                   # -5 - 60 * 0.05, -5 - 50 * 0.05
        g = _grid(gpu_ctx, cells, origin=origin)
    lf = bl.LikelihoodField(sigma=0.1, max_cells=6, ctx=gpu_ctx)
    fg = lf.compute(g)
    f0 = lm.field(cells, 0.1, 6, mpc)
    assert np.array_equal(fg.cells(), f0)
    moved = [_step(oracle, opf, pf, (mpc, origin), k, scans[k], odo[k + 1], rands[k], f0, fg)[0] for k in range(4)]
    assert moved[1:] == [True, True, True]                                              # (the first update only latches the odometry)
    # a map update from a pose beside the truth, with odds that saturate: walls the rays cross drop to 0, end cells in free space rise
    mapper = bl.Mapping(5.0, 127, 127, ctx=gpu_ctx)
    for k in (3, 4, 5):                                                                 # (the first call only latches the pose)
        mapper.updateMap(scans[k], bl.make_pose(0.3, -0.2, 0.5, utime=int(scans[k].times[-1])), g)
    cells1 = g.cells()
    f1 = lm.field(cells1, 0.1, 6, mpc)
    assert ((cells1 >= 1) != (cells >= 1)).sum() > 50 and (f1 != f0).sum() > 1000
    assert lf.compute(g) is fg
    for k in range(4, 7):
        assert _step(oracle, opf, pf, (mpc, origin), k, scans[k], odo[k + 1], rands[k], f1, fg)[0]
    assert np.array_equal(fg.cells(), f1)
    for x in (pf, lf, mapper, g):
        x.close()


# ------------------------------------------------------------------ the scan matcher on a field
def test_matcher_on_a_field(maps, gpu_ctx):
    m = maps["obstacle_slam_10mx10m_5cm"]
    cells = m["cells"]
    truth = np.where(cells > 0, 127, -127).astype(np.int8)
    g = _grid(gpu_ctx, cells, origin=m["origin"])
    lf = bl.LikelihoodField(sigma=0.1, max_cells=6, ctx=gpu_ctx)
    fg = lf.compute(g)
    fcells = lm.field(cells, 0.1, 6, m["mpc"])
    pose = (-0.75, 0.2, 0.4)
    scan = synth.raycast_scan(truth, m["origin"], 0.05, pose, pose, 123456)
    matcher = bl.ScanMatcher(ctx=gpu_ctx)
    dth = np.float32(np.radians(0.5))
    for off, (nx, ny, nt) in (((0.12, -0.08, 0.03), (4, 4, 12)), ((-0.3, 0.2, -0.1), (10, 3, 20))):
        c = bl.make_pose(pose[0] + off[0], pose[1] + off[1], pose[2] + off[2], utime=7)
        for prior, half_life in ((None, None), ((300, 50, 400, 200), 64)):
            if prior is None:
                res = matcher.match(scan, c, fg, nx=nx, ny=ny, ntheta=nt, dtheta=dth, keep_volume=True)
                ref = sm.match(fcells, m["origin"], m["mpc"], CPM, scan.ranges, scan.thetas, (c.x, c.y, c.theta), nx, ny, nt, dth, 8.0,
                               utime=scan.utime)
            else:
                res, mom = matcher.match_prior(scan, c, fg, prior=prior, half_life=half_life, nx=nx, ny=ny, ntheta=nt, dtheta=dth)
                ref = smp.match(fcells, m["origin"], m["mpc"], CPM, scan.ranges, scan.thetas, (c.x, c.y, c.theta), nx, ny, nt, dth, 8.0,
                                prior=prior, half_life=half_life, utime=scan.utime)
                assert (mom.best_obj, mom.pen_best) == (ref["best_obj"], ref["pen_best"])
            assert np.array_equal(matcher.volume(), ref["volume"])
            got = (res.di, res.dj, res.dk, res.score, res.score_centre, res.ties, res.rays_used, res.accepted, res.pose.utime)
            exp = (ref["di"], ref["dj"], ref["dk"], ref["score"], ref["score_centre"], ref["ties"], ref["rays_used"], ref["accepted"], ref["utime"])
            assert got == exp, (got, exp)
            gp = np.array([res.pose.x, res.pose.y, res.pose.theta], dtype=np.float32)
            ep = np.array([ref["x"], ref["y"], ref["theta"]], dtype=np.float32)
            assert gp.tobytes() == ep.tobytes(), (gp, ep)
    for x in (matcher, lf, g):
        x.close()
