"""bl_beam_reweigh_pf on a 64 x 48 map: the units it installs are the model's of the filter's own poses, poses and parents stay byte for
byte, and from then on the filter behaves as a twin that received the same units through bl_pf_set_particles: the same posterior pose
and the same resampling indices in the next update.

The issue's smallest count, one particle, does not exist: bl_pf_create refuses num_particles <= 1 (particle_filter.cpp:11), which the
first test states; the smallest filter there is, two particles, stands in for it."""
import ctypes as C
import math

import numpy as np
import pytest

import botlab_amd as bl
from botlab_amd import synth
import beam_cases as bc
import beam_model as bm
from test_gpu_beam import KEYS

pytestmark = pytest.mark.gpu
F32 = np.float32
POSE_FIELDS = ("utime", "x", "y", "theta", "p_utime", "p_x", "p_y", "p_theta")


class World:
    """The 64 x 48 room of the ray-count cases, a short drive through it and the scans seen on the way."""

    def __init__(self, ctx):
        self.case = c = bc.ray_count(0)
        self.params = bm.params(max_range=2.0, span=1 << 26)      # 1024 nats: a cloud after an update spreads over many units
        self.grid = bl.OccupancyGrid.from_cells(c["cells"], c["origin"], c["mpc"], cellsPerMeter=c["cpm"], ctx=ctx)
        truth = np.where(c["cells"] > 0, 127, -127).astype(np.int8)
        self.odo = [(0.8 + 0.05 * k, 1.0 + 0.02 * k, 0.1 * k) for k in range(5)]
        self.scans = [synth.raycast_scan(truth, c["origin"], c["mpc"], self.odo[max(k - 1, 0)], self.odo[k], 1_000_000 + 100_000 * k, max_range=3.0)
                      for k in range(5)]
        self.beam = bl.BeamModel(ctx=ctx, **{k: self.params[k] for k in KEYS})
        self.tables = self.beam.tables(c["cpm"])

    def cloud(self, n, seed=3):
        """n particles scattered round the drive's start, a few of them off the grid."""
        rng = np.random.default_rng(seed)
        p = np.zeros(n, bl.PARTICLE_DTYPE)
        p["x"] = (0.8 + rng.normal(0, 0.15, n)).astype(np.float32)
        p["y"] = (1.0 + rng.normal(0, 0.15, n)).astype(np.float32)
        p["theta"] = rng.normal(0, 0.2, n).astype(np.float32)
        if n >= 64:
            p["x"][5], p["y"][17] = -0.3, 9.0
        for f in ("x", "y", "theta"):
            p["p_" + f] = p[f]
        p["utime"] = p["p_utime"] = self.scans[0].utime
        p["weight"] = 1.0 / n
        return p

    def model_units(self, parts, scan):
        c = self.case
        poses = np.stack([parts["x"], parts["y"], parts["theta"]], axis=1)
        S = bm.scores(c["cells"], c["origin"], c["cpm"], scan.ranges, scan.thetas, poses, self.params, self.tables)
        return S, bm.units(S, self.params["span"], bl.BeamModel.unitTable())

    def update(self, pf, k, rand_value=12345):
        return pf.updateFilter(bl.make_pose(*self.odo[k], utime=self.scans[k].utime), self.scans[k], self.grid, rand_value=rand_value)

    def close(self):
        self.beam.close()
        self.grid.close()


@pytest.fixture(scope="module")
def world(gpu_ctx):
    w = World(gpu_ctx)
    yield w
    w.close()


def started(world, ctx, n, seed=3):
    pf = bl.ParticleFilter(n, ctx=ctx)
    pf.setParticles(world.cloud(n, seed))
    pf.setNoiseSeed(99)
    pf.debugEnable(True)
    world.update(pf, 0)                                                   # latches the odometry
    world.update(pf, 1)                                                   # a moved update: resampled, sensor-model weights
    return pf


def test_a_filter_of_one_particle_does_not_exist(gpu_ctx):
    h = C.c_void_p()
    assert gpu_ctx.lib.bl_pf_create(gpu_ctx.h, 1, 0, 1, C.byref(h)) == 2


@pytest.mark.parametrize("n", [2, 64, 1000])
def test_reweigh_equals_a_twin_with_uploaded_units(gpu_ctx, world, n):
    a, b = started(world, gpu_ctx, n), started(world, gpu_ctx, n)
    try:
        before = a.particles()
        assert before.tobytes() == b.particles().tobytes()
        scan = world.scans[1]
        pose_a = a.reweigh_beam(world.beam, world.grid, scan)
        after = a.particles()
        for f in POSE_FIELDS:
            assert after[f].tobytes() == before[f].tobytes(), f             # poses and parents byte for byte
        S, u = world.model_units(before, scan)
        got = world.beam.units(n)
        assert np.array_equal(got, u), (np.flatnonzero(got != u)[:5], got[:5], u[:5])
        print("n", n, "distinct units", len(set(u.tolist())), "at the floor", int((u == 1).sum()), "device ms", world.beam.lastDeviceMs())
        if n >= 64:
            assert len(set(u.tolist())) > 4                                  # (of the input: else the twin comparison says little)
        b.setParticles(b.particles(), u)
        pose_b = b.estimatePosteriorPose()
        est = a.poseEstimate()
        for p in (pose_a, est):
            assert (p.x, p.y, p.theta, p.utime) == (pose_b.x, pose_b.y, pose_b.theta, pose_b.utime)
        assert a.particles().tobytes() == b.particles().tobytes()            # the weights too: units / S
        assert a.debugUniformRuns() == 0                                     # an upload of unequal units, whatever the values
        for pf in (a, b):
            world.update(pf, 2, rand_value=846930886)
        ia, ib = a.debugLast()[0], b.debugLast()[0]
        assert np.array_equal(ia, ib)
        if len(set(u.tolist())) > 1:
            assert a.particles().tobytes() == b.particles().tobytes()
    finally:
        a.close()
        b.close()


def test_cloud_with_particles_off_the_grid(gpu_ctx, world):
    """Straight after an upload (no update moves them back): the off-grid particles get one unit and Smax ignores them."""
    n = 64
    pf = bl.ParticleFilter(n, ctx=gpu_ctx)
    try:
        cloud = world.cloud(n)
        pf.setParticles(cloud)
        pf.reweigh_beam(world.beam, world.grid, world.scans[0])
        S, u = world.model_units(cloud, world.scans[0])
        assert (S == bm.OFF_GRID).sum() == 2 and u[5] == 1 and u[17] == 1 and u.max() == 2 ** 20
        assert np.array_equal(world.beam.units(n), u)
        w = pf.particles()["weight"]
        assert np.array_equal(w, u.astype(np.float64) / float(u.astype(np.uint64).sum()))
    finally:
        pf.close()


def test_adaptive_count_below_capacity_scores_the_active_particles_only(gpu_ctx, world):
    cap = 1000
    pf = bl.ParticleFilter(cap, ctx=gpu_ctx)
    try:
        pf.initializeFilterAtPose(bl.make_pose(*world.odo[0], utime=world.scans[0].utime), seed=11)
        pf.setNoiseSeed(5)
        pf.setAdaptive(minParticles=100)
        for k in range(4):
            world.update(pf, k)
        active = pf.adaptiveState()["active"]
        assert 100 <= active < cap
        before = pf.particles()
        assert len(before) == active
        pf.reweigh_beam(world.beam, world.grid, world.scans[3])
        _, u = world.model_units(before, world.scans[3])
        assert np.array_equal(world.beam.units(active), u)
        with pytest.raises(bl.BotlabHipError, match="status 2"):
            world.beam.units(cap)
        after = pf.particles()
        assert len(after) == active
        for f in POSE_FIELDS:
            assert after[f].tobytes() == before[f].tobytes(), f
        assert np.array_equal(after["weight"], u.astype(np.float64) / float(u.astype(np.uint64).sum()))
        world.update(pf, 4)                                                  # and the filter goes on
        assert pf.adaptiveState()["active"] >= 100
    finally:
        pf.close()


def test_recovery_tracker_folds_the_sensor_update_behind_a_reweigh(gpu_ctx, world):
    """Recovery on and every update followed by a reweigh (what the driver does under setBeamModel): the tracker goes on folding the
    SENSOR update's weight total -- kept aside before the units are replaced, once per record -- exactly as its model does with the
    totals read before each reweigh; it primes, and with a huge ratio it injects."""
    import recovery_model as rm
    n = 1000
    pf = bl.ParticleFilter(n, ctx=gpu_ctx)
    try:
        pf.setParticles(world.cloud(n))                                      # pose utime != 0: the first moved update is not folded
        pf.setNoiseSeed(99)
        pf.setRecovery(world.grid, ratio=1e9, maxFraction=0.25, seed=77)
        world.update(pf, 0)                                                  # latches the odometry
        tr = rm.Tracker()
        S, sensed, utime = 0, False, world.scans[0].utime
        for u in range(1, 5):
            world.update(pf, u)
            st = pf.recoveryState()
            tr.step(u, S, n, sensed, ratio=1e9, max_fraction=0.25)
            assert (st["w_slow"], st["w_fast"], st["w_avg"], st["p_inject"], st["updates"], st["primed"]) == tr.as_tuple(), (u, st)
            S, sensed = pf.spread()["units_sum"], rm.folds_next(utime if u == 1 else 0)
            for _ in range(2):                                               # the second reweigh of a record must not take the beam total
                pf.reweigh_beam(world.beam, world.grid, world.scans[u])
            beam_total = int(world.beam.units(n).astype(np.uint64).sum())
            assert pf.spread()["units_sum"] == beam_total != S
            if u == 3:                                                       # an action-only update carries weights and the kept total over
                pf.updateFilterActionOnly(bl.make_pose(*world.odo[u], utime=world.scans[u].utime))
        st = pf.recoveryState()
        assert st["primed"] == 1 and st["w_avg"] > 0 and st["p_inject"] == 0.25 and st["injected_total"] > 0
        # with recovery off the units are an upload and nothing is kept: turning recovery on afterwards does not fold them
        pf.setRecovery(None)
        world.update(pf, 0)
        pf.reweigh_beam(world.beam, world.grid, world.scans[0])
        pf.setRecovery(world.grid, ratio=1e9, maxFraction=0.25, seed=77)
        world.update(pf, 1)
        st = pf.recoveryState()
        assert (st["primed"], st["updates"], st["w_avg"]) == (0, 1, 0.0)
    finally:
        pf.close()


def test_state_errors(gpu_ctx, world):
    fresh = bl.ParticleFilter(64, ctx=gpu_ctx)
    try:
        with pytest.raises(bl.BotlabHipError, match="status 4"):
            fresh.reweigh_beam(world.beam, world.grid, world.scans[0])       # not initialised
    finally:
        fresh.close()
    pf = started(world, gpu_ctx, 64)
    try:
        before = pf.particles()
        assert pf.updateBegin(bl.make_pose(*world.odo[2], utime=world.scans[2].utime), world.scans[2], world.grid, 12345)
        with pytest.raises(bl.BotlabHipError, match="status 4"):
            pf.reweigh_beam(world.beam, world.grid, world.scans[2])          # a pending update
        pf.updateEnd()
        far = bm.params(**dict(world.params, max_range=300.0))
        beam = bl.BeamModel(ctx=gpu_ctx, **{k: far[k] for k in KEYS})
        try:
            now = pf.particles()
            with pytest.raises(bl.BotlabHipError, match="status 2"):
                pf.reweigh_beam(beam, world.grid, world.scans[2])            # refused before anything is touched
            assert pf.particles().tobytes() == now.tobytes() and now.tobytes() != before.tobytes()
        finally:
            beam.close()
    finally:
        pf.close()
