"""bl.RBSlam on the inputs of tests/test_rb_slam_edges_cpu.py, which shows on the CPU that each of them reaches the path it is meant
for: k_rb_map's serial walk of scans above 512 rays, its column tiles, its several tiles per workgroup after a pose jump, rb_apply's
clamps and pass order in both code forms; k_rb_plan's exact due test at equality and one score beside it at 4096 particles near the
largest score, its searches where every target falls on a partial sum, its slot table and copy list with maps that name their particle;
k_rb_weigh's saturation, a scan without a kept ray, equal utimes; rays within one cell; walks with dmaj >= 32768 on a long thin grid
and from 8.5 million cells away.  Every case compares what
tests/test_gpu_rb_slam.py compares, after every update: flags, indices, likelihoods, scores, units, S, Q, best, all poses and all P maps,
byte for byte against tests/rb_slam_model.py."""
import numpy as np
import pytest

import botlab_amd as bl
import rb_slam_model as rbm
import test_rb_slam_edges_cpu as E
from botlab_amd import synth
from botlab_amd.host import LidarScan
from test_gpu_rb_slam import _compare, _pair, _run

pytestmark = pytest.mark.gpu


def _go(oracle, gpu_ctx, c):
    """The whole case on the device and in the model; returns (model, device object, [(moved, resampled)])."""
    mdl, rb = _pair(oracle, gpu_ctx, c.frame, c.P, c.num, c.den, c.odoms[0], spread=c.spread, cpm=c.cpm, max_laser=c.max_laser, hit=c.hit,
                    miss=c.miss)
    E.prepare(c, mdl, rb)
    flags = _run(mdl, rb, c.odoms, c.scans, c.noise_seed, rand_value=c.rand_value)
    return mdl, rb, flags


# ---- 1. long scans
@pytest.mark.parametrize("rays", [E.LONG_RAYS, E.LONGEST_RAYS])
def test_long_scans(oracle, maps, gpu_ctx, rays):
    c = E.long_case(maps, rays)
    mdl, rb, flags = _go(oracle, gpu_ctx, c)
    assert [f[0] for f in flags] == [False] + [True] * (len(flags) - 1)
    assert np.count_nonzero(mdl.maps[0]) > 1000
    rb.close()


def test_long_scan_through_a_pose_jump(oracle, maps, gpu_ctx):
    mdl, rb, flags = _go(oracle, gpu_ctx, E.long_jump_case(maps))
    assert all(f[0] for f in flags[1:])
    rb.close()


def test_a_scan_above_the_ray_limit_is_refused(maps, gpu_ctx):
    c = E.long_case(maps, E.LONG_RAYS)
    rb = bl.RBSlam(2, 200, 200, c.mpc, c.cpm, c.origin, c.max_laser, c.hit, c.miss, ctx=gpu_ctx)
    o = c.odoms[0]
    rb.initializeAtPose(bl.make_pose(o[0], o[1], o[2], utime=o[3]), seed=1)
    n = E.MAX_RAYS + 1
    scan = LidarScan(np.full(n, 1.0, np.float32), (2.0 * np.pi * np.arange(n) / n).astype(np.float32),
                     (o[3] - (n - 1 - np.arange(n)) * synth.RAY_DT_US).astype(np.int64), utime=o[3])
    with pytest.raises(bl.BotlabHipError):
        rb.update(bl.make_pose(o[0], o[1], o[2], utime=o[3]), scan, rand_value=1)
    rb.close()


# ---- 2. column tiles and row tiles; 3. more tiles than workgroups
@pytest.mark.parametrize("form", ["dwords", "bytes"])
def test_wide_window(oracle, maps, gpu_ctx, form):
    mdl, rb, flags = _go(oracle, gpu_ctx, E.wide_case(maps, form))
    assert np.count_nonzero(mdl.maps[0]) > 10000
    rb.close()


@pytest.mark.parametrize("form", ["dwords", "bytes"])
def test_pose_jump(oracle, maps, gpu_ctx, form):
    mdl, rb, flags = _go(oracle, gpu_ctx, E.jump_case(maps, form))
    assert all(f[0] for f in flags[1:])
    rb.close()


# ---- 4. rails
@pytest.mark.parametrize("variant", sorted(E.RAIL_VARIANTS))
def test_rails(oracle, maps, gpu_ctx, variant):
    mdl, rb, flags = _go(oracle, gpu_ctx, E.rail_case(maps, variant))
    assert np.count_nonzero(mdl.maps == 127) > 0 and np.count_nonzero(mdl.maps == -128) > 0
    rb.close()


# ---- 5. the exact due test
@pytest.mark.parametrize("which", ["tie", "up", "down"])
@pytest.mark.parametrize("P,t", E.DUE_CASES)
def test_due_edges(oracle, maps, gpu_ctx, P, t, which):
    """Update 0 does not move and reports S and Q of the uploaded scores; update 1 moves and resamples iff 5 S^2 <= 4 P Q."""
    c = E.due_case(maps, P, t, which)
    mdl, rb = _pair(oracle, gpu_ctx, c.frame, c.P, c.num, c.den, c.odoms[0], spread=c.spread, cpm=c.cpm, max_laser=c.max_laser, hit=c.hit,
                    miss=c.miss)
    E.prepare(c, mdl, rb)
    u = [1000 * int(v) for v in c.cum]
    S, Q = sum(u), sum(v * v for v in u)
    due = E.DUE_DEN * S * S <= E.DUE_NUM * P * Q
    assert due == (which != "down")
    rng = np.random.default_rng(c.noise_seed)
    for k in range(2):
        o = c.odoms[k]
        noise = mdl.draw_noise(o, rng)
        r_m = mdl.update(o, c.scans[k], 4242 + k, noise)
        r_g = rb.update(bl.make_pose(o[0], o[1], o[2], utime=o[3]), c.scans[k], rand_value=4242 + k, noise=noise)
        _compare(mdl, rb, r_m, r_g, k)
        if k == 0:
            assert not r_g["moved"] and (r_g["S"], r_g["Q"]) == (S, Q)
        else:
            assert r_g["moved"] and r_g["resampled"] == due
    idx = rb.debugLast()[0]
    assert np.array_equal(idx, rbm.am.resample_integer(np.array(u, np.uint64), 4242 + 1, P) if due else np.arange(P))
    rb.close()


def test_saturation(oracle, maps, gpu_ctx):
    c = E.saturation_case(maps)
    mdl, rb, flags = _go(oracle, gpu_ctx, c)
    assert flags == [(False, False), (True, False), (True, False)]
    cum = rb.particles()[1]
    assert np.count_nonzero(cum == rbm.SCORE_MAX) >= 3 and cum.max() == rbm.SCORE_MAX
    rb.close()


# ---- 6. search ties; maps that name their particle
@pytest.mark.parametrize("rand_value", E.TIE_RANDS)
@pytest.mark.parametrize("P", E.TIE_PS)
def test_search_ties(oracle, maps, gpu_ctx, P, rand_value):
    c = E.tie_case(maps, P, rand_value)
    mdl, rb, flags = _go(oracle, gpu_ctx, c)
    assert flags == [(False, False), (True, True)]
    idx = rb.debugLast()[0]
    assert np.array_equal(idx, rbm.am.resample_integer(rbm.units_of(c.cum), rand_value, P))
    for p in range(P):
        assert rbm.watermark_owner(rb.mapCells(p), E.SMALL_BLOCK) == idx[p], p
    rb.close()


def test_uneven_weights_with_named_maps(oracle, maps, gpu_ctx):
    c = E.uneven_case(maps)
    mdl, rb, flags = _go(oracle, gpu_ctx, c)
    res = [f[1] for f in flags if f[0]]
    assert any(res) and not all(res[1:])
    owners = np.array([rbm.watermark_owner(rb.mapCells(p), E.MAIN_BLOCK) for p in range(c.P)])
    assert np.all(owners >= 0) and np.count_nonzero(owners != np.arange(c.P)) >= 8       # children that carry another particle's map
    rb.close()


# ---- 7. small things
def test_scan_without_a_kept_ray(oracle, maps, gpu_ctx):
    c = E.blind_case(maps)
    mdl, rb, flags = _go(oracle, gpu_ctx, c)
    assert all(f[0] for f in flags[1:])
    rb.close()


def test_update_at_the_utime_of_the_one_before(oracle, maps, gpu_ctx):
    c = E.same_utime_case(maps)
    mdl, rb, flags = _go(oracle, gpu_ctx, c)
    assert all(f[0] for f in flags[1:])
    rb.close()


def test_coarse_grid(oracle, maps, gpu_ctx):
    c = E.coarse_case(maps)
    mdl, rb, flags = _go(oracle, gpu_ctx, c)
    assert np.count_nonzero(mdl.maps[0]) > 10
    rb.close()


# ---- 8. long and thin
def test_long_thin_grid(oracle, maps, gpu_ctx):
    """32 800 x 8 cells, two particles, eight rays with dmaj >= 32768: k_rb_map's segments start at k0 > 0 behind the point where the
    walk's first division takes 64 bits.  The particles follow the odometry (no noise), so the rays end inside the grid."""
    c = E.long_thin_case(maps)
    mdl, rb = _pair(oracle, gpu_ctx, c.frame, c.P, c.num, c.den, c.odoms[0], spread=c.spread, cpm=c.cpm, max_laser=c.max_laser, hit=c.hit,
                    miss=c.miss)
    parts = E.long_thin_particles(mdl)
    mdl.set_particles(parts)
    rb.setParticles(parts)
    rng = np.random.default_rng(c.noise_seed)
    for k, o in enumerate(c.odoms):
        noise = mdl.draw_noise(o, rng, stds=E.NO_NOISE)
        r_m = mdl.update(o, c.scans[k], 4242 + k, noise)
        r_g = rb.update(bl.make_pose(o[0], o[1], o[2], utime=o[3]), c.scans[k], rand_value=4242 + k, noise=noise)
        _compare(mdl, rb, r_m, r_g, k)
    assert np.count_nonzero(mdl.maps[0]) > 32768 and not np.array_equal(mdl.maps[0], mdl.maps[1])
    rb.close()


# ---- 9. a start far outside the grid
def test_far_start(oracle, maps, gpu_ctx):
    """Two particles 8.5 million cells from the grid: start cells between 2^23 and 2^24, and a walk whose first division takes in more
    than 2^32 where the rays reach the grid."""
    c = E.far_case(maps)
    mdl, rb = _pair(oracle, gpu_ctx, c.frame, c.P, c.num, c.den, c.odoms[0], spread=c.spread, cpm=c.cpm, max_laser=c.max_laser, hit=c.hit,
                    miss=c.miss)
    parts = E.far_particles(mdl)
    mdl.set_particles(parts)
    rb.setParticles(parts)
    rng = np.random.default_rng(c.noise_seed)
    for k, o in enumerate(c.odoms):
        noise = mdl.draw_noise(o, rng, stds=E.NO_NOISE)
        r_m = mdl.update(o, c.scans[k], 4242 + k, noise)
        r_g = rb.update(bl.make_pose(o[0], o[1], o[2], utime=o[3]), c.scans[k], rand_value=4242 + k, noise=noise)
        _compare(mdl, rb, r_m, r_g, k)
    assert np.count_nonzero(mdl.maps[0]) > 100 and not np.array_equal(mdl.maps[0], mdl.maps[1])
    rb.close()
