"""bl.RBSlam (bl_rbslam_*, botlab_amd/csrc/bl_rbslam.hip) against the model (tests/rb_slam_model.py), byte for byte: after EVERY update
moved, resampled, the resample indices, the likelihood half-units, cumulative scores, units, S, Q, the best index, all poses and ALL
P maps."""
import numpy as np
import pytest

import botlab_amd as bl
import helpers
import oracle_lib
import rb_slam_model as rbm
from test_rb_slam_model_cpu import CPM, HALF_SEEDED, HIT, MAX_LASER, MISS, RAGGED_ORIGIN, RAGGED_SHAPE, make_run

pytestmark = pytest.mark.gpu
POSE_FIELDS = ["utime", "x", "y", "theta", "p_utime", "p_x", "p_y", "p_theta"]


def _pair(oracle, gpu_ctx, m, P, num, den, start, shape=None, origin=None, spread=None, cpm=CPM, max_laser=MAX_LASER, hit=HIT, miss=MISS):
    """The model and the device object of one run, both holding the same particles (tests/test_gpu_rb_slam_edges.py shares it)."""
    shape = shape or m["cells"].shape
    origin = origin or m["origin"]
    mdl = rbm.started_model(oracle, P, shape, m["mpc"], cpm, origin, max_laser, hit, miss, num, den, start, spread)
    rb = bl.RBSlam(P, shape[1], shape[0], m["mpc"], cpm, origin, max_laser, hit, miss, ctx=gpu_ctx)
    rb.setResampling(num, den)
    rb.initializeAtPose(bl.make_pose(start[0], start[1], start[2], utime=1000), seed=1)
    rb.setParticles(mdl.parts)
    return mdl, rb


def _compare(mdl, rb, r_m, r_g, k, maps_of=None):
    assert r_g["moved"] == r_m["moved"] and r_g["resampled"] == r_m["resampled"], k
    parts, cum, units = rb.particles()
    for f in POSE_FIELDS:
        assert parts[f].tobytes() == mdl.parts[f].tobytes(), (k, f)
    assert np.array_equal(cum, mdl.cum) and np.array_equal(units, mdl.units), k
    if r_m["moved"]:
        idx, like = rb.debugLast()
        assert np.array_equal(idx, mdl.idx) and np.array_equal(like, mdl.like), k
        assert parts["weight"].tobytes() == mdl.parts["weight"].tobytes(), k
    assert (r_g["S"], r_g["Q"], r_g["best"]) == (r_m["S"], r_m["Q"], r_m["best"]), k
    gp = r_g["pose"]
    assert (np.float32(gp.x), np.float32(gp.y), np.float32(gp.theta), gp.utime) == \
           (np.float32(r_m["pose"][0]), np.float32(r_m["pose"][1]), np.float32(r_m["pose"][2]), r_m["pose"][3]), k
    for p in (range(mdl.P) if maps_of is None else maps_of):
        assert rb.mapCells(p).tobytes() == mdl.maps[p].tobytes(), (k, p)


def _run(mdl, rb, odoms, scans, seed, maps_every=1, maps_of=None, rand_value=None):
    rng = np.random.default_rng(seed)
    flags = []
    for k in range(len(odoms)):
        o = odoms[k]
        noise = mdl.draw_noise(o, rng)
        rv = 4242 + k if rand_value is None else rand_value
        r_m = mdl.update(o, scans[k], rv, noise)
        r_g = rb.update(bl.make_pose(o[0], o[1], o[2], utime=o[3]), scans[k], rand_value=rv, noise=noise)
        last = k == len(odoms) - 1
        _compare(mdl, rb, r_m, r_g, k, maps_of=maps_of if maps_of is not None else (None if last or k % maps_every == 0 else []))
        flags.append((r_m["moved"], r_m["resampled"]))
    return flags


@pytest.mark.parametrize("num,den", [(1, 1), (1, 2)])
def test_main_run_matches_the_model(oracle, maps, gpu_ctx, num, den):
    m, poses, odoms, scans = make_run(maps, 30)
    mdl, rb = _pair(oracle, gpu_ctx, m, 64, num, den, odoms[0], spread=9)
    if den == 2:
        mdl.maps[:HALF_SEEDED] = m["cells"]
        for p in range(HALF_SEEDED):
            rb.uploadMap(p, m["cells"])
    flags = _run(mdl, rb, odoms, scans, 11)
    res = [f[1] for f in flags if f[0]]
    if den == 1:
        assert all(res[1:]) and not res[0]
    else:
        assert any(res) and not all(res[1:])
    assert np.count_nonzero(mdl.maps[0]) > 1000
    rb.close()


def test_update_without_motion_in_the_middle(oracle, maps, gpu_ctx):
    m, poses, odoms, scans = make_run(maps, 8, pause_at=5)
    mdl, rb = _pair(oracle, gpu_ctx, m, 8, 1, 1, odoms[0], spread=2)
    flags = _run(mdl, rb, odoms, scans, 3)
    assert [f[0] for f in flags].count(False) == 2 and not flags[5][0]
    rb.close()


def test_ragged_grid_with_rays_leaving_it(oracle, maps, gpu_ctx):
    m, poses, odoms, scans = make_run(maps, 8)
    # 203 x 117 cells with the robot near their lower left corner: rays cross the left and the bottom edge and end outside the grid
    # (tests/test_rb_slam_model_cpu.py checks that of the inputs)
    mdl, rb = _pair(oracle, gpu_ctx, m, 8, 1, 1, odoms[0], shape=RAGGED_SHAPE, origin=RAGGED_ORIGIN, spread=4)
    _run(mdl, rb, odoms, scans, 5)
    assert np.count_nonzero(mdl.maps[0][:, 0]) > 0 and np.count_nonzero(mdl.maps[0][0, :]) > 0     # the update reaches the grid's edges
    rb.close()


def test_single_particle_against_the_existing_map_kernel(oracle, maps, gpu_ctx):
    m, poses, odoms, scans = make_run(maps, 10)
    mdl, rb = _pair(oracle, gpu_ctx, m, 1, 1, 1, odoms[0])
    g = bl.OccupancyGrid.from_cells(np.zeros(m["cells"].shape, np.int8), m["origin"], m["mpc"], cellsPerMeter=CPM, ctx=gpu_ctx)
    mapper = bl.Mapping(MAX_LASER, HIT, MISS, ctx=gpu_ctx)
    rng = np.random.default_rng(1)
    for k in range(len(odoms)):
        o = odoms[k]
        noise = mdl.draw_noise(o, rng)
        r_m = mdl.update(o, scans[k], 99 + k, noise)
        r_g = rb.update(bl.make_pose(o[0], o[1], o[2], utime=o[3]), scans[k], rand_value=99 + k, noise=noise)
        _compare(mdl, rb, r_m, r_g, k)
        mapper.updateMap(scans[k], r_g["pose"], g)
        assert rb.mapCells(0).tobytes() == g.cells().tobytes(), k
    rb.close(); mapper.close(); g.close()


def test_a_thousand_particles(oracle, maps, gpu_ctx):
    m, poses, odoms, scans = make_run(maps, 4)
    mdl, rb = _pair(oracle, gpu_ctx, m, 1000, 1, 1, odoms[0], spread=6)
    _run(mdl, rb, odoms, scans, 7)
    rb.close()


def test_large_grid(oracle, maps, gpu_ctx):
    m, poses, odoms, scans = make_run(maps, 5)
    origin = (np.float32(-25.0), np.float32(-25.0))
    mdl, rb = _pair(oracle, gpu_ctx, m, 16, 1, 1, odoms[0], shape=(1000, 1000), origin=origin, spread=8)
    _run(mdl, rb, odoms, scans, 9)
    assert np.count_nonzero(mdl.maps[0]) > 1000
    rb.close()


def test_upload_and_download_round_trips(oracle, maps, gpu_ctx):
    m = maps["obstacle_slam_10mx10m_5cm"]
    P = 5
    rb = bl.RBSlam(P, 200, 200, m["mpc"], CPM, m["origin"], MAX_LASER, HIT, MISS, ctx=gpu_ctx)
    rb.initializeAtPose(bl.make_pose(0.5, -0.25, 0.3, utime=77), seed=3)
    rng = np.random.default_rng(0)
    parts = np.zeros(P, bl.PARTICLE_DTYPE)
    for f in ["x", "y", "theta", "p_x", "p_y", "p_theta"]:
        parts[f] = rng.uniform(-1, 1, P).astype(np.float32)
    parts["utime"], parts["p_utime"] = 500, 400
    cum = np.array([0, 5, 1 << 33, 123456789, 7], np.int64)
    rb.setParticles(parts, cum)
    got, gcum, gunits = rb.particles()
    for f in POSE_FIELDS:
        assert got[f].tobytes() == parts[f].tobytes(), f
    assert np.array_equal(gcum, cum) and np.array_equal(gunits, rbm.units_of(cum))
    assert got["weight"].tobytes() == (gunits.astype(np.float64) / float(int(gunits.sum()))).tobytes()
    cells = [rng.integers(-128, 128, (200, 200)).astype(np.int8) for _ in range(P)]
    for p in (3, 0, 4, 1, 2):
        rb.uploadMap(p, cells[p])
    for p in range(P):
        assert rb.mapCells(p).tobytes() == cells[p].tobytes()
    assert rb.best_map().cells().tobytes() == cells[2].tobytes()          # the largest score
    # init draws as the particle filter's: same seed, same poses; the last particle is the pose itself
    rb.initializeAtPose(bl.make_pose(0.5, -0.25, 0.3, utime=77), seed=1234)
    pf = bl.ParticleFilter(P, ctx=gpu_ctx)
    pf.initializeFilterAtPose(bl.make_pose(0.5, -0.25, 0.3, utime=77), seed=1234)
    a, b = rb.particles()[0], pf.particles()
    for f in POSE_FIELDS:
        assert a[f].tobytes() == b[f].tobytes(), f
    assert not rb.mapCells(1).any()
    pf.close(); rb.close()


def test_best_map_feeds_the_motion_planner(oracle, maps, gpu_ctx):
    m, poses, odoms, scans = make_run(maps, 12)
    mdl, rb = _pair(oracle, gpu_ctx, m, 8, 1, 2, odoms[0], spread=12)
    _run(mdl, rb, odoms, scans, 13, maps_of=[0])
    planner = bl.MotionPlanner(ctx=gpu_ctx)
    planner.setMap(rb.best_map())
    exp = oracle.set_distances(mdl.maps[mdl.best], m["mpc"], CPM, m["origin"])
    assert planner.distances_.cells().view(np.uint32).tobytes() == exp.view(np.uint32).tobytes()
    rb.close()


def test_error_paths(gpu_ctx, maps):
    m = maps["obstacle_slam_10mx10m_5cm"]
    with pytest.raises(bl.BotlabHipError):                      # over the byte cap: 4096 maps of 2000 x 2000 cells
        bl.RBSlam(4096, 2000, 2000, 0.05, CPM, (0, 0), MAX_LASER, HIT, MISS, ctx=gpu_ctx)
    with pytest.raises(bl.BotlabHipError):
        bl.RBSlam(4097, 10, 10, 0.05, CPM, (0, 0), MAX_LASER, HIT, MISS, ctx=gpu_ctx)
    with pytest.raises(bl.BotlabHipError):
        bl.RBSlam(0, 10, 10, 0.05, CPM, (0, 0), MAX_LASER, HIT, MISS, ctx=gpu_ctx)
    rb = bl.RBSlam(4, 200, 200, m["mpc"], CPM, m["origin"], MAX_LASER, HIT, MISS, ctx=gpu_ctx)
    _, _, odoms, scans = make_run(maps, 1)
    with pytest.raises(bl.BotlabHipError):                      # update before init
        rb.update(bl.make_pose(0, 0, 0, utime=1), scans[0], rand_value=1)
    with pytest.raises(bl.BotlabHipError):
        rb.mapCells(0)
    rb.initializeAtPose(bl.make_pose(0, 0, 0, utime=1), seed=1)
    other = bl.OccupancyGrid.from_cells(np.zeros((100, 200), np.int8), m["origin"], m["mpc"], cellsPerMeter=CPM, ctx=gpu_ctx)
    with pytest.raises(bl.BotlabHipError):                      # shape mismatch
        rb.best_map(other)
    with pytest.raises(bl.BotlabHipError):
        rb.setResampling(0, 1)
    with pytest.raises(bl.BotlabHipError):
        rb.mapCells(4)
    other.close(); rb.close()


def test_philox_mode_is_repeatable_and_seeded(maps, gpu_ctx):
    """No bit-exact yardstick exists for the device's own noise: it runs, repeats for a seed, and differs between seeds."""
    m, poses, odoms, scans = make_run(maps, 10)

    def run(seed):
        rb = bl.RBSlam(32, 200, 200, m["mpc"], CPM, m["origin"], MAX_LASER, HIT, MISS, ctx=gpu_ctx)
        rb.setNoiseSeed(seed)
        rb.initializeAtPose(bl.make_pose(odoms[0][0], odoms[0][1], odoms[0][2], utime=1000), seed=5)
        for k in range(len(odoms)):
            o = odoms[k]
            r = rb.update(bl.make_pose(o[0], o[1], o[2], utime=o[3]), scans[k], rand_value=17 + k)
        out = (rb.particles()[0].tobytes(), b"".join(rb.mapCells(p).tobytes() for p in range(32)), r["best"])
        rb.close()
        return out

    a, b, c = run(1), run(1), run(2)
    assert a == b
    assert a[0] != c[0] and a[1] != c[1]
    assert np.frombuffer(a[1], np.int8).any()


def test_filter_and_rb_slam_share_the_devices_own_noise(gpu_ctx):
    """The yardstick the Philox path has: bl_pfmodel.h's initial draw and applyAction run in k_pf_init / k_mcl_main and in k_rb_init /
    k_rb_weigh.  One ParticleFilter and one RBSlam, P = 300 (two 256-thread blocks of the init kernels, 75 workgroups of k_rb_weigh),
    the same init pose and seed and the same noise seed: bit-identical (x, y, theta) of every particle after initialisation, and of
    every pose and parent pose after each of two moved steps -- the filter through updateFilterActionOnly, RB-SLAM through update on
    a 40 x 40 map with an 8-ray scan and a resampling threshold that no weight set reaches (1 / 65535 < 1 / P <= Q / S^2)."""
    P, W, H = 300, 40, 40
    start = bl.make_pose(0.3, -0.2, 3.1, utime=1000)
    pf = bl.ParticleFilter(P, ctx=gpu_ctx)
    rb = bl.RBSlam(P, W, H, 0.05, CPM, (-1.0, -1.0), MAX_LASER, HIT, MISS, ctx=gpu_ctx)
    rb.setResampling(1, 65535)
    pf.setNoiseSeed(0x123456789abcdef)
    rb.setNoiseSeed(0x123456789abcdef)
    pf.initializeFilterAtPose(start, seed=77)
    rb.initializeAtPose(start, seed=77)
    fields = ["x", "y", "theta", "p_x", "p_y", "p_theta"]

    def same(k):
        a, b = pf.particles(), rb.particles()[0]
        for f in fields:
            assert a[f].tobytes() == b[f].tobytes(), (k, f)
        return a

    a0 = same("init")
    assert len(np.unique(a0["x"])) > P // 2 and (a0["x"][-1], a0["y"][-1], a0["theta"][-1]) == (start.x, start.y, start.theta)
    thetas = np.linspace(0.0, 5.5, 8).astype(np.float32)
    prev = a0
    for k, o in enumerate([(0.3, -0.2, 3.1, 1000), (0.25, -0.19, -3.12, 101000), (0.2, -0.21, -3.0, 201000)]):
        scan = bl.LidarScan(np.full(8, 0.6, np.float32), thetas, np.linspace(o[3] - 90000, o[3], 8).astype(np.int64), utime=o[3])
        odom = bl.make_pose(o[0], o[1], o[2], utime=o[3])
        pf.updateFilterActionOnly(odom)
        r = rb.update(odom, scan, rand_value=99 + k)
        assert r["moved"] == (k > 0) and not r["resampled"], k
        cur = same(k)
        if k > 0:
            assert cur["p_x"].tobytes() == prev["x"].tobytes() and cur["p_theta"].tobytes() == prev["theta"].tobytes(), k
            assert np.count_nonzero(cur["x"] != prev["x"]) > P - 5, k
        prev = cur
    pf.close(); rb.close()
