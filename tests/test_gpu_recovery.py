"""Kidnapped-robot recovery on the GPU (bl_pf_set_recovery): the tracker, the injected set and the injected priors bit-equal to the
numpy model (tests/recovery_model.py), the whole update equal to the CPU reference filter run on the reconstructed prior, the three
update paths bit-equal, recovery off / disabled / never firing equal to a filter without it, the argument errors, 1M particles on
4096^2, and re-localisation after a kidnap on the calibrated scenario."""
import math

import numpy as np
import pytest

import global_init_model as gm
import helpers
import oracle_lib
import recovery_model as rm
import botlab_amd as bl
from botlab_amd import _capi, synth

pytestmark = pytest.mark.gpu
REL = 1e-5          # particle poses after an update, as in test_gpu_parity.py
SEED = 0x5EED_0F_2ECE


def _world(maps, size, src="astar_maze"):
    w = synth.tile_world(maps[src]["cells"], size)
    cells = np.where(w > 0, 100, -60).astype(np.int8)
    half = size * 0.05 / 2.0
    return cells, (np.float32(-half), np.float32(-half)), np.float32(0.05)


def _map(maps, name):
    if name.startswith("tile"):
        return _world(maps, int(name[4:]))
    m = maps[name]
    return m["cells"], m["origin"], m["mpc"]


def _scenario(maps, name, steps):
    cells, origin, mpc = _map(maps, name)
    start = gm.CAL_START if name == gm.CAL_MAP else (0.3, 0.3, 0.0)
    truth = np.where(cells > 0, 127, -127).astype(np.int8)
    poses = synth.square_trajectory(start, steps, step_len=0.04, turn=0.1, side=0.3)
    odo = synth.odometry_from_truth(poses, np.random.default_rng(8))
    return cells, origin, mpc, truth, poses, odo, start


def _state_tuple(s):
    return (s["w_slow"], s["w_fast"], s["w_avg"], s["p_inject"], s["updates"], s["primed"])


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("where,n", [(gm.CAL_MAP, 5000), ("tile2000", 20_000)])
def test_forced_injection_equals_model_and_reference(oracle, maps, gpu_ctx, where, n):
    """Strict resampling, host noise: every update's tracker, injected set and injected priors equal the model's, and the whole
    update equals the CPU reference filter run on the prior rebuilt from the reference's resample plus the model's samples."""
    cells, origin, mpc, truth, poses, odo, start = _scenario(maps, where, 10)
    cpm = helpers.CPM_DEFAULT
    g = bl.OccupancyGrid.from_cells(cells, origin, mpc, cellsPerMeter=cpm, ctx=gpu_ctx)
    elig = gm.eligible_cells(cells)
    opf = oracle_lib.OraclePF(oracle, n)
    opf.init_at_pose(oracle.pose(*start, utime=1000), 5)
    pf = bl.ParticleFilter(n, ctx=gpu_ctx)
    pf.setParticles(opf.particles())
    pf.setStrictResampling(True)
    pf.debugEnable(True)
    pf.setRecovery(g, ratio=1e9, maxFraction=0.25, seed=SEED)
    tr = rm.Tracker()
    scan0 = synth.raycast_scan(truth, origin, 0.05, poses[0], poses[0], 1000)
    assert not opf.update(oracle.pose(*odo[0], utime=scan0.utime), scan0, cells, mpc, cpm, origin, 1)["moved"]
    pf.updateFilter(bl.make_pose(*odo[0], utime=scan0.utime), scan0, g, rand_value=1)
    S, sensed, injected_any = 0, False, 0
    for u in range(1, len(poses)):
        scan = synth.raycast_scan(truth, origin, 0.05, poses[u - 1], poses[u], 1000 + 100000 * u)
        rv = 1000 + 37 * u
        t = tr.step(u, S, n, sensed, ratio=1e9, max_fraction=0.25)
        post = opf.particles()
        idx_ref = rm.resample(post["weight"], rv)
        inj = rm.injected_mask(SEED, u, t, n)
        prior = post[idx_ref].copy()
        x, y, th = rm.sample(SEED, elig, cells.shape[1], origin, mpc, np.flatnonzero(inj), u)
        prior["x"][inj], prior["y"][inj], prior["theta"][inj] = x, y, th
        prior["weight"] = 1.0 / n
        opf.set_particles(prior)
        res = opf.update(oracle.pose(*odo[u], utime=scan.utime), scan, cells, mpc, cpm, origin, rm.RAND_MAX // 2)
        assert res["moved"] and np.array_equal(res["idx"], np.arange(n))      # low-variance resampling of equal weights: identity
        pose = pf.updateFilter(bl.make_pose(*odo[u], utime=scan.utime), scan, g, rand_value=rv, noise=res["noise"])
        st = pf.recoveryState()
        assert _state_tuple(st) == tr.as_tuple(), u
        assert st["injected_last"] == int(inj.sum()) and (t == 0) == (st["injected_last"] == 0)
        injected_any += int(inj.sum())
        assert st["injected_total"] == injected_any
        idx, like = pf.debugLast()
        assert np.array_equal(idx == -1, inj), u
        assert np.array_equal(idx[~inj], idx_ref[~inj]), u
        got, exp = pf.particles(), opf.particles()
        for f, v in (("p_x", x), ("p_y", y), ("p_theta", th)):
            assert np.array_equal(_bits(got[f][inj]), _bits(v)), (u, f)
        assert np.array_equal(like.astype(np.float64) * 0.5, res["raw"]), u
        for f in ("x", "y", "theta"):
            assert np.allclose(got[f], exp[f], rtol=REL, atol=1e-7)
        assert np.allclose(got["weight"], exp["weight"], rtol=REL, atol=0)
        assert np.array_equal(_bits([pose.x, pose.y, pose.theta]), _bits([res["pose"].x, res["pose"].y, res["pose"].theta])), u
        S, sensed = int(rm.units_of(res["raw"]).sum()), u > 1
    assert tr.primed and injected_any > 0 and tr.p == 0.25
    pf.close()
    g.close()


def _run_default(maps, gpu_ctx, where, n, steps, noise_seed=17, path="update", recovery="on", ratio=1e9, max_fraction=0.25, debug=True,
                 utime0=1000):
    """Integer-prefix resampling with Philox noise; returns (pf, per-update [(state, idx, parents)], grid)."""
    cells, origin, mpc, truth, poses, odo, start = _scenario(maps, where, steps)
    cpm = helpers.CPM_DEFAULT
    g = bl.OccupancyGrid.from_cells(cells, origin, mpc, cellsPerMeter=cpm, ctx=gpu_ctx)
    mapper = bl.Mapping(5.0, 4, 1, ctx=gpu_ctx)
    pf = bl.ParticleFilter(n, ctx=gpu_ctx)
    pf.setNoiseSeed(noise_seed)
    pf.initializeFilterAtPose(bl.make_pose(*start, utime=utime0), seed=5)
    if debug:
        pf.debugEnable(True)
    if recovery in ("on", "off_again"):
        pf.setRecovery(g, ratio=ratio, maxFraction=max_fraction, seed=SEED)
    if recovery == "off_again":
        pf.setRecovery(None)
    out = []
    for k in range(0, len(poses)):
        scan = synth.raycast_scan(truth, origin, 0.05, poses[max(k - 1, 0)], poses[k], 1000 + 100000 * k)
        od = bl.make_pose(*odo[k], utime=scan.utime)
        if path == "update":
            pose = pf.updateFilter(od, scan, g, rand_value=1000 + k)
            mapper.updateMap(scan, pose, g)
        elif path == "begin_end":
            pf.updateBegin(od, scan, g, 1000 + k)
            pose = pf.updateEnd()
            mapper.updateMap(scan, pose, g)
        else:
            pf.updateBegin(od, scan, g, 1000 + k)
            mapper.updateMapFinishingFilter(scan, pf, od.utime, g)
        if k > 0:
            out.append((pf.recoveryState(), pf.debugLast()[0] if debug else None, pf.particles(), pf.spread()["units_sum"] if debug else None))
    mapper.close()
    return pf, out, g, cells, origin, mpc


@pytest.mark.parametrize("utime0", [1000, 0])
def test_default_mode_equals_model(maps, gpu_ctx, utime0):
    """The integer-prefix rule (and the equal-weight path of the first resampling): tracker, injected set and injected priors.  Started
    at utime 1000 the first update interpolates its scan and its posterior is not folded; started at utime 0 it is."""
    n = 5000
    pf, out, g, cells, origin, mpc = _run_default(maps, gpu_ctx, gm.CAL_MAP, n, 10, utime0=utime0)
    elig = gm.eligible_cells(cells)
    tr = rm.Tracker()
    S, sensed = 0, False
    for u, (st, idx, parts, units_sum) in enumerate(out, start=1):
        t = tr.step(u, S, n, sensed, ratio=1e9, max_fraction=0.25)
        assert _state_tuple(st) == tr.as_tuple(), u
        inj = rm.injected_mask(SEED, u, t, n)
        assert np.array_equal(idx == -1, inj), u
        x, y, th = rm.sample(SEED, elig, cells.shape[1], origin, mpc, np.flatnonzero(inj), u)
        for f, v in (("p_x", x), ("p_y", y), ("p_theta", th)):
            assert np.array_equal(_bits(parts[f][inj]), _bits(v)), (u, f)
        S, sensed = units_sum, rm.folds_next(utime0 if u == 1 else 0)
    assert sum(int(np.sum(o[1] == -1)) for o in out) > 0
    pf.close()
    g.close()


def test_update_paths_bit_equal(maps, gpu_ctx):
    runs = [_run_default(maps, gpu_ctx, gm.CAL_MAP, 4000, 9, path=p, debug=False) for p in ("update", "begin_end", "fused")]
    ref = runs[0][1]
    assert sum(o[0]["injected_last"] for o in ref) > 0
    for pf, out, g, *_ in runs[1:]:
        for a, b in zip(ref, out):
            assert _state_tuple(a[0]) == _state_tuple(b[0]) and a[0]["injected_total"] == b[0]["injected_total"]
            assert a[2].tobytes() == b[2].tobytes()
    for pf, out, g, *_ in runs:
        pf.close()
        g.close()


def test_off_means_today(maps, gpu_ctx):
    """Never enabled, enabled then disabled, and enabled with a ratio so small that p stays 0: bit-equal filters."""
    runs = [_run_default(maps, gpu_ctx, gm.CAL_MAP, 4000, 9, recovery=r, ratio=1e-9, debug=False) for r in ("never", "off_again", "on")]
    ref = runs[0][1]
    for pf, out, g, *_ in runs[1:]:
        for a, b in zip(ref, out):
            assert a[2].tobytes() == b[2].tobytes()
    assert all(o[0]["p_inject"] == 0.0 and o[0]["injected_total"] == 0 for o in runs[2][1])
    assert runs[2][1][-1][0]["primed"] == 1
    for pf, out, g, *_ in runs:
        pf.close()
        g.close()


def test_errors_leave_filter(maps, gpu_ctx):
    """Bad parameters, no eligible cell and a distance grid of another shape: BL_ERR_ARG, and the filter -- particles, tracker and the
    recovery list in force -- is exactly as it was (the next update injects from the old list and continues the old tracker)."""
    n = 5000
    cells, origin, mpc, truth, poses, odo, start = _scenario(maps, gm.CAL_MAP, 5)
    cpm = helpers.CPM_DEFAULT
    g = bl.OccupancyGrid.from_cells(cells, origin, mpc, cellsPerMeter=cpm, ctx=gpu_ctx)
    f = maps["filled"]
    gf = bl.OccupancyGrid.from_cells(f["cells"], f["origin"], f["mpc"], cellsPerMeter=cpm, ctx=gpu_ctx)
    d = bl.ObstacleDistanceGrid(ctx=gpu_ctx)
    d.setDistances(gf)
    pf = bl.ParticleFilter(n, ctx=gpu_ctx)
    pf.setNoiseSeed(17)
    pf.initializeFilterAtPose(bl.make_pose(*start, utime=1000), seed=5)
    pf.debugEnable(True)
    pf.setRecovery(g, ratio=1e9, maxFraction=0.25, seed=SEED)
    scans = [synth.raycast_scan(truth, origin, 0.05, poses[max(k - 1, 0)], poses[k], 1000 + 100000 * k) for k in range(len(poses))]
    for k in range(4):                                       # u = 1, 2, 3: primed at u = 3 and injecting
        pf.updateFilter(bl.make_pose(*odo[k], utime=scans[k].utime), scans[k], g, rand_value=1000 + k)
    before, parts = pf.recoveryState(), pf.particles()
    assert before["primed"] == 1 and before["injected_total"] > 0
    bad = [dict(alphaSlow=0.1, alphaFast=0.1), dict(alphaSlow=0.0), dict(alphaFast=1.5), dict(ratio=0.0), dict(ratio=math.inf),
           dict(ratio=math.nan), dict(maxFraction=-0.1), dict(maxFraction=1.5)]
    for kw in bad:
        with pytest.raises(_capi.BotlabHipError):
            pf.setRecovery(g, **kw)
    with pytest.raises(_capi.BotlabHipError):
        pf.setRecovery(gf, seed=1)                           # no eligible cell
    with pytest.raises(_capi.BotlabHipError):
        pf.setRecovery(g, d, seed=1)                         # a distance grid of another shape
    assert pf.recoveryState() == before and pf.particles().tobytes() == parts.tobytes()
    # the next update: the old tracker goes on (u = 4) and injects from the old list with the old seed
    pf.updateFilter(bl.make_pose(*odo[4], utime=scans[4].utime), scans[4], g, rand_value=1004)
    st = pf.recoveryState()
    assert st["updates"] == 4 and st["p_inject"] == 0.25 and st["injected_total"] == before["injected_total"] + st["injected_last"]
    inj = rm.injected_mask(SEED, 4, rm.threshold(0.25), n)
    idx, _ = pf.debugLast()
    assert np.array_equal(idx == -1, inj)
    x, y, th = rm.sample(SEED, gm.eligible_cells(cells), cells.shape[1], origin, mpc, np.flatnonzero(inj), 4)
    got = pf.particles()
    for fld, v in (("p_x", x), ("p_y", y), ("p_theta", th)):
        assert np.array_equal(_bits(got[fld][inj]), _bits(v)), fld
    # an update pending: BL_ERR_STATE for every recovery call
    assert pf.updateBegin(bl.make_pose(*odo[5], utime=scans[5].utime), scans[5], g, 1005)
    for call in (lambda: pf.setRecovery(g), lambda: pf.setRecovery(None), lambda: pf.recoveryState()):
        with pytest.raises(_capi.BotlabHipError):
            call()
    pf.updateEnd()
    assert pf.recoveryState()["updates"] == 5
    pf.setRecovery(None)
    assert all(v == 0 for v in pf.recoveryState().values())
    params = _capi.C.byref(_capi.PfRecoveryParams(0.001, 0.1, 0.9, 0.1, 0.0, 1))
    # a partial slice: BL_ERR_STATE
    part = bl.ParticleFilter(1000, ctx=gpu_ctx, shard=(0, 500))
    assert gpu_ctx.lib.bl_pf_set_recovery(part.h, g.h, None, params) == 4
    # a composed shard (rank 0 of two, set up for the composed finish): BL_ERR_STATE
    from botlab_amd.sharded import composed_align, shard_bounds
    N = 100_000
    lo, hi, S = shard_bounds(N, 0, 2, composed_align(N))
    comp = bl.ParticleFilter(N, ctx=gpu_ctx, shard=(lo, hi))
    _capi.check(gpu_ctx.lib.bl_pf_shard_setup(comp.h, 0, 2, S))
    assert gpu_ctx.lib.bl_pf_set_recovery(comp.h, g.h, None, params) == 4
    for h in (pf, part, comp, d, g, gf):
        h.close()


def test_scale_4096_1m(maps, gpu_ctx):
    """One update of 1 000 000 particles on 4096^2 injecting a quarter: the injected set and priors equal the model's."""
    n = 1_000_000
    pf, out, g, cells, origin, mpc = _run_default(maps, gpu_ctx, "tile4096", n, 3)
    elig = gm.eligible_cells(cells)
    st, idx, parts, _ = out[-1]
    u = 3
    assert st["updates"] == u and st["primed"] == 1 and st["p_inject"] == 0.25
    inj = rm.injected_mask(SEED, u, rm.threshold(0.25), n)
    assert np.array_equal(idx == -1, inj) and st["injected_last"] == int(inj.sum())
    x, y, th = rm.sample(SEED, elig, cells.shape[1], origin, mpc, np.flatnonzero(inj), u)
    for f, v in (("p_x", x), ("p_y", y), ("p_theta", th)):
        assert np.array_equal(_bits(parts[f][inj]), _bits(v)), f
    pf.close()
    g.close()


@pytest.mark.parametrize("recover", [True, False])
def test_kidnap_recovery(maps, gpu_ctx, recover):
    """N = 100 000, Philox noise, default parameters: after the kidnap of the calibrated scenario (test_kidnap_calibration) the
    filter is back within CAL_EST_TOL with CAL_NEAR_WEIGHT near the truth within KID_KR moved updates; without recovery it is not."""
    n = 100_000
    m = maps[rm.KID_MAP]
    cells, origin, mpc = m["cells"], m["origin"], m["mpc"]
    g = bl.OccupancyGrid.from_cells(cells, origin, mpc, cellsPerMeter=helpers.CPM_DEFAULT, ctx=gpu_ctx)
    truthmap = np.where(cells > 0, 127, -127).astype(np.int8)
    motion, truth, begin = rm.kidnap_truth()
    odo = synth.odometry_from_truth(motion, np.random.default_rng(3))
    pf = bl.ParticleFilter(n, ctx=gpu_ctx)
    pf.setNoiseSeed(17)
    pf.initializeFilterAtPose(bl.make_pose(*rm.KID_START, utime=1000), seed=5)
    if recover:
        pf.setRecovery(g, seed=rm.KID_SEED)
    scan0 = synth.raycast_scan(truthmap, origin, 0.05, truth[0], truth[0], 1000)
    assert not pf.updateBegin(bl.make_pose(*odo[0], utime=scan0.utime), scan0, g, 1)
    pf.updateEnd()
    for k in range(1, len(truth)):
        scan = synth.raycast_scan(truthmap, origin, 0.05, begin[k], truth[k], 1000 + 100000 * k)
        assert pf.updateBegin(bl.make_pose(*odo[k], utime=scan.utime), scan, g, 1000 + k)
        pose = pf.updateEnd()
        if k == rm.KID_K0 and recover:
            assert pf.recoveryState()["injected_total"] == 0          # tracking: p stayed 0
    tr = truth[-1]
    err = math.hypot(pose.x - tr[0], pose.y - tr[1])
    near = gm.near_weight(pf.particles(), tr)
    if recover:
        assert err <= gm.CAL_EST_TOL and near >= gm.CAL_NEAR_WEIGHT, (err, near)
        assert pf.recoveryState()["injected_total"] > 0
    else:
        assert err > rm.KID_LOST and near < 0.1, (err, near)
    pf.close()
    g.close()
