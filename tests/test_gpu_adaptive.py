"""Adaptive particle count on the GPU (bl_pf_set_adaptive, KLD-sampling): with min_particles = capacity the filter is the fixed
filter bit for bit; the count, k_sat and next equal the numpy model (tests/adaptive_model.py) computed from the exported parent
poses; with next != active the resample indices follow the integer and the strict rule, the whole update equals the CPU reference
run on the prior the model rebuilds, and the estimate is the reference's; every update path gives the same bits; errors leave the
filter as it was; recovery composes with it."""
import math

import numpy as np
import pytest

import adaptive_model as am
import global_init_model as gm
import helpers
import oracle_lib
import recovery_model as rm
import botlab_amd as bl
from botlab_amd import synth
from test_gpu_recovery import _bits, _map, _scenario     # the scenarios of the recovery tests

pytestmark = pytest.mark.gpu
REL = 1e-5
SEED = 0x5EED_0F_2ECE
BXY, BTH = 0.1, math.radians(10.0)


def _model_check(pf, model):
    """The state after a resampling update equals the model's count over the exported parent poses."""
    parts = pf.particles()
    model.counted(parts["p_x"], parts["p_y"], parts["p_theta"])
    st = pf.adaptiveState()
    assert (st["active"], st["bins"], st["k_sat"], st["next"]) == (model.active, model.bins, model.ksat, model.next), st
    return st, parts


def _run(maps, gpu_ctx, where, n, steps, path="update", adaptive=None, init="pose", noise_seed=17, debug=True, recovery=False,
         disable_at=None, action_only_at=None):
    """Integer-prefix resampling with Philox noise along the scenario; returns (per-update [(state, particles, debugLast idx)], pf, g)."""
    cells, origin, mpc, truth, poses, odo, start = _scenario(maps, where, steps)
    cpm = helpers.CPM_DEFAULT
    g = bl.OccupancyGrid.from_cells(cells, origin, mpc, cellsPerMeter=cpm, ctx=gpu_ctx)
    mapper = bl.Mapping(5.0, 4, 1, ctx=gpu_ctx)
    planner = bl.AsyncPlanner(ctx=gpu_ctx) if path == "planner" else None
    pf = bl.ParticleFilter(n, ctx=gpu_ctx)
    pf.setNoiseSeed(noise_seed)
    if init == "pose":
        pf.initializeFilterAtPose(bl.make_pose(*start, utime=1000), seed=5)
    else:
        pf.initializeFilterUniformly(g, utime=1000, seed=9)
    if debug:
        pf.debugEnable(True)
    if recovery:
        pf.setRecovery(g, ratio=1e9, maxFraction=0.25, seed=SEED)
    if adaptive is not None:
        pf.setAdaptive(**adaptive)
    out = []
    for k in range(0, len(poses)):
        scan = synth.raycast_scan(truth, origin, 0.05, poses[max(k - 1, 0)], poses[k], 1000 + 100000 * k)
        od = bl.make_pose(*odo[k], utime=scan.utime)
        if k == disable_at:
            pf.setAdaptive(None)
        if k == action_only_at:
            pf.updateFilterActionOnly(od)
        elif path == "update":
            pose = pf.updateFilter(od, scan, g, rand_value=1000 + k)
            mapper.updateMap(scan, pose, g)
        elif path == "begin_end":
            pf.updateBegin(od, scan, g, 1000 + k)
            pose = pf.updateEnd()
            mapper.updateMap(scan, pose, g)
        elif path == "fused":
            pf.updateBegin(od, scan, g, 1000 + k)
            mapper.updateMapFinishingFilter(scan, pf, od.utime, g)
        else:
            pf.updateBegin(od, scan, g, 1000 + k)
            planner.submit_with_map_update_finishing(mapper, scan, pf, od.utime, g, bl.make_pose(start[0] + 0.5, start[1], 0.0))
            planner.fetch()
        if k > 0:
            st = pf.adaptiveState() if adaptive is not None or disable_at is not None else None
            if recovery:
                st["units_sum"] = pf.spread()["units_sum"]
            out.append((st, pf.particles(), pf.debugLast()[0] if debug else None, pf.poseEstimate()))
    if planner is not None:
        planner.close()
    mapper.close()
    return out, pf, g


def _adaptive(min_particles, eps=0.01, z=2.326, bxy=BXY, bth=BTH):
    return dict(minParticles=min_particles, epsilon=eps, z=z, binXY=bxy, binTheta=bth)


def test_fixed_equivalence(maps, gpu_ctx):
    """min_particles = capacity: poses, particles, weights and debugLast bit-identical to the fixed filter."""
    n = 5000
    fixed, pf0, g0 = _run(maps, gpu_ctx, gm.CAL_MAP, n, 8)
    adap, pf1, g1 = _run(maps, gpu_ctx, gm.CAL_MAP, n, 8, adaptive=_adaptive(n))
    for (_, pa, ia, qa), (st, pb, ib, qb) in zip(fixed, adap):
        assert st["active"] == n and st["next"] == n and st["bins"] > 0
        assert pa.tobytes() == pb.tobytes()
        assert np.array_equal(ia, ib)
        assert _bits([qa.x, qa.y, qa.theta]).tobytes() == _bits([qb.x, qb.y, qb.theta]).tobytes()
    for o in (pf0, g0, pf1, g1):
        o.close()


@pytest.mark.parametrize("where,n,init", [("tile200", 100_000, "uniform"), ("tile4096", 1_000_000, "uniform"), (gm.CAL_MAP, 20_000, "pose")])
def test_count_and_bound_parity(maps, gpu_ctx, where, n, init):
    """bins, k_sat and next equal the model's from the exported parent poses: a map-wide cloud on 200^2 / 100k, a map-wide cloud on
    4096^2 / 1M (the count saturates at k_sat), and a converged cloud tracking from the true pose."""
    p = _adaptive(200)
    model = am.CountModel(n, am.Params(200, 0.01, 2.326, BXY, BTH))
    cells, origin, mpc, truth, poses, odo, start = _scenario(maps, where, 4)
    g = bl.OccupancyGrid.from_cells(cells, origin, mpc, cellsPerMeter=helpers.CPM_DEFAULT, ctx=gpu_ctx)
    pf = bl.ParticleFilter(n, ctx=gpu_ctx)
    if init == "pose":
        pf.initializeFilterAtPose(bl.make_pose(*start, utime=1000), seed=5)
    else:
        pf.initializeFilterUniformly(g, utime=1000, seed=9)
    pf.setAdaptive(**p)
    st = pf.adaptiveState()
    assert (st["active"], st["next"], st["bins"], st["counts"]) == (n, n, 0, 0) and st["k_sat"] == model.ksat
    seen = []
    for k in range(len(poses)):
        scan = synth.raycast_scan(truth, origin, 0.05, poses[max(k - 1, 0)], poses[k], 1000 + 100000 * k)
        pf.updateFilter(bl.make_pose(*odo[k], utime=scan.utime), scan, g, rand_value=1000 + k)
        if k == 0:
            continue
        st, _ = _model_check(pf, model)
        assert st["counts"] == k
        seen.append(st)
    if where == "tile4096":
        assert all(s["bins"] == model.ksat and s["next"] == n for s in seen)
    if init == "pose":
        assert seen[-1]["next"] < n // 2
    pf.close()
    g.close()


def test_next_differs_from_active(oracle, maps, gpu_ctx):
    """Shrinking (next < active) and growing (after disabling, next = capacity > active): debugResample equals the integer rule with
    M = next, and in strict mode the reference's rule; the equal-weight closed form right after init_uniform; the whole update equals
    the CPU reference on the rebuilt prior with 3 * next noise floats, and its estimate is the reference's estimatePosteriorPose."""
    n = 20_000
    cells, origin, mpc, truth, poses, odo, start = _scenario(maps, gm.CAL_MAP, 8)
    cpm = helpers.CPM_DEFAULT
    g = bl.OccupancyGrid.from_cells(cells, origin, mpc, cellsPerMeter=cpm, ctx=gpu_ctx)
    pf = bl.ParticleFilter(n, ctx=gpu_ctx)
    pf.initializeFilterUniformly(g, utime=1000, seed=9)
    pf.setAdaptive(**_adaptive(200))
    for rv in (0, 1, 4321, rm.RAND_MAX):                            # closed form: equal weights, next = active = n
        assert np.array_equal(pf.debugResample(rv), am.resample_reference(np.full(n, 1.0 / n), rv, n)), rv
    pf.initializeFilterAtPose(bl.make_pose(*start, utime=1000), seed=5)
    pf.debugEnable(True)
    checked = {"shrink": 0, "grow": 0, "strict": 0}
    for k in range(len(poses)):
        scan = synth.raycast_scan(truth, origin, 0.05, poses[max(k - 1, 0)], poses[k], 1000 + 100000 * k)
        od = bl.make_pose(*odo[k], utime=scan.utime)
        if k == 6:
            pf.setAdaptive(None)                                     # grow: the next update draws the capacity again
        if 2 <= k <= 6:
            st = pf.adaptiveState()
            active, nxt = st["active"], st["next"]
            assert nxt != active
            checked["grow" if nxt > active else "shrink"] += 1
            post = pf.particles()
            idx_gpu, like = pf.debugLast()
            units = rm.units_of(like.astype(np.float64) * 0.5)
            rv = 1000 + 37 * k
            assert np.array_equal(pf.debugResample(rv), am.resample_integer(units, rv, nxt)), k
            if k % 2 == 0:
                pf.setStrictResampling(True)
                want = am.resample_reference(post["weight"], rv, nxt)
                assert np.array_equal(pf.debugResample(rv), want), k
                checked["strict"] += 1
                # the whole update against the reference filter on the prior of nxt particles
                prior = post[want].copy()
                prior["weight"] = 1.0 / nxt
                opf = oracle_lib.OraclePF(oracle, nxt)
                opf.set_particles(prior)
                prev = odo[k - 1]
                assert not opf.update(oracle.pose(*prev, utime=od.utime - 1), scan, cells, mpc, cpm, origin, 1)["moved"]
                res = opf.update(oracle.pose(*odo[k], utime=scan.utime), scan, cells, mpc, cpm, origin, rm.RAND_MAX // 2)
                assert res["moved"] and np.array_equal(res["idx"], np.arange(nxt))
                pose = pf.updateFilter(od, scan, g, rand_value=rv, noise=res["noise"])
                got, exp = pf.particles(), opf.particles()
                assert len(got) == nxt and pf.adaptiveState()["active"] == nxt
                gi, glike = pf.debugLast()
                assert np.array_equal(gi, want) and np.array_equal(glike.astype(np.float64) * 0.5, res["raw"]), k
                for f in ("x", "y", "theta"):
                    assert np.allclose(got[f], exp[f], rtol=REL, atol=1e-7)
                assert np.allclose(got["weight"], exp["weight"], rtol=REL, atol=0)
                est = oracle_lib.OPose()
                oracle.lib.orc_estimate_pose(np.ascontiguousarray(got).ctypes.data, nxt, est)
                assert _bits([pose.x, pose.y, pose.theta]).tobytes() == _bits([est.x, est.y, est.theta]).tobytes(), k
                pf.setStrictResampling(False)
                continue
        pf.updateFilter(od, scan, g, rand_value=1000 + k)
    assert checked["shrink"] >= 2 and checked["grow"] >= 1 and checked["strict"] >= 2, checked
    assert pf.adaptiveState()["active"] == n
    pf.close()
    g.close()


@pytest.mark.parametrize("path", ["begin_end", "fused", "planner"])
def test_update_paths_bit_equal(maps, gpu_ctx, path):
    """update, begin + end, the fused map finish and the planner ride-along: the same counts and the same bits."""
    ref, pf0, g0 = _run(maps, gpu_ctx, gm.CAL_MAP, 8000, 7, adaptive=_adaptive(200), debug=False)
    out, pf1, g1 = _run(maps, gpu_ctx, gm.CAL_MAP, 8000, 7, path=path, adaptive=_adaptive(200), debug=False)
    assert ref[-1][0]["active"] < 8000
    for (sa, pa, _, qa), (sb, pb, _, qb) in zip(ref, out):
        assert sa == sb
        assert pa.tobytes() == pb.tobytes()
        assert _bits([qa.x, qa.y, qa.theta]).tobytes() == _bits([qb.x, qb.y, qb.theta]).tobytes()
    for o in (pf0, g0, pf1, g1):
        o.close()


def test_action_only_and_disable(maps, gpu_ctx):
    """An action-only update keeps active, next and the count; disabling restores the capacity at the next resampling update."""
    n = 8000
    out, pf, g = _run(maps, gpu_ctx, gm.CAL_MAP, n, 8, adaptive=_adaptive(200), action_only_at=4, disable_at=6)
    s3, s4 = out[2][0], out[3][0]                                   # after updates 3 and 4 (4: action only)
    assert s3["active"] < n and (s4["active"], s4["next"], s4["bins"], s4["counts"]) == (s3["active"], s3["next"], s3["bins"], s3["counts"])
    s5, s6 = out[4][0], out[5][0]
    assert s5["counts"] == s3["counts"] + 1
    assert s6["active"] == n and s6["next"] == n and s6["k_sat"] == 0 and len(out[5][1]) == n
    pf.close()
    g.close()


def test_errors_leave_filter(maps, gpu_ctx):
    n = 5000
    cells, origin, mpc, truth, poses, odo, start = _scenario(maps, gm.CAL_MAP, 3)
    g = bl.OccupancyGrid.from_cells(cells, origin, mpc, cellsPerMeter=helpers.CPM_DEFAULT, ctx=gpu_ctx)
    pf = bl.ParticleFilter(n, ctx=gpu_ctx)
    pf.initializeFilterAtPose(bl.make_pose(*start, utime=1000), seed=5)
    pf.setAdaptive(**_adaptive(200))
    for k in range(3):
        scan = synth.raycast_scan(truth, origin, 0.05, poses[max(k - 1, 0)], poses[k], 1000 + 100000 * k)
        pf.updateFilter(bl.make_pose(*odo[k], utime=scan.utime), scan, g, rand_value=1000 + k)
    before, parts = pf.adaptiveState(), pf.particles()
    assert before["active"] < n
    bad = [dict(minParticles=1), dict(minParticles=n + 1), dict(epsilon=0.0), dict(epsilon=float("nan")), dict(z=-1.0),
           dict(binXY=0.0), dict(binTheta=float("inf"))]
    for b in bad:
        kw = _adaptive(200)
        kw.update(b)
        with pytest.raises(RuntimeError):
            pf.setAdaptive(**kw)
        assert pf.adaptiveState() == before
    # an update pending: the state and enabling are refused
    scan = synth.raycast_scan(truth, origin, 0.05, poses[2], poses[3], 1000 + 100000 * 3)
    pf.updateBegin(bl.make_pose(*odo[3], utime=scan.utime), scan, g, 7)
    with pytest.raises(RuntimeError):
        pf.adaptiveState()
    with pytest.raises(RuntimeError):
        pf.setAdaptive(**_adaptive(300))
    pf.updateEnd()
    after = pf.adaptiveState()
    assert after["counts"] == before["counts"] + 1 and after["k_sat"] == before["k_sat"]
    # a sharded filter (a partial slice of the set) is refused
    sh = bl.ParticleFilter(4096, ctx=gpu_ctx, shard=(0, 2048))
    with pytest.raises(RuntimeError):
        sh.setAdaptive(**_adaptive(200))
    sh.close()
    pf.close()
    g.close()


def test_recovery_composes(maps, gpu_ctx):
    """Recovery forced on (ratio 1e9) with adaptive mode: the tracker folds w_avg over active particles, the injected set is the model's
    over the next output particles, and the count includes the injected parents."""
    n = 8000
    out, pf, g = _run(maps, gpu_ctx, gm.CAL_MAP, n, 8, adaptive=_adaptive(200), recovery=True)
    cells, origin, mpc = _map(maps, gm.CAL_MAP)
    elig = gm.eligible_cells(cells)
    model = am.CountModel(n, am.Params(200, 0.01, 2.326, BXY, BTH))
    tr = rm.Tracker()
    S, sensed, active, injected = 0, False, n, 0
    for u, (st, parts, idx, _) in enumerate(out, start=1):
        t = tr.step(u, S, active, sensed, ratio=1e9, max_fraction=0.25)
        nxt = len(parts)
        assert nxt == model.next
        inj = rm.injected_mask(SEED, u, t, nxt)
        assert np.array_equal(idx == -1, inj), u
        x, y, th = rm.sample(SEED, elig, cells.shape[1], origin, mpc, np.flatnonzero(inj), u)
        for f, v in (("p_x", x), ("p_y", y), ("p_theta", th)):
            assert np.array_equal(_bits(parts[f][inj]), _bits(v)), (u, f)
        model.counted(parts["p_x"], parts["p_y"], parts["p_theta"])
        assert (st["bins"], st["next"]) == (model.bins, model.next), u
        injected += int(inj.sum())
        S, sensed, active = st["units_sum"], rm.folds_next(1000 if u == 1 else 0), nxt
    # (a quarter of every update scattered over the map occupies more bins than k_sat: recovery holds the count at the capacity)
    assert injected > 0 and out[-1][0]["next"] == n
    pf.close()
    g.close()
