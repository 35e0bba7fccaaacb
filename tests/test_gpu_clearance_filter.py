"""bl_clearance_reweigh_pf on the 64 x 48 map of tests/test_gpu_beam_filter.py: it leaves the bytes bl_beam_reweigh_pf leaves on a twin
filter -- the units, the pose, the particles, the next update's resampling indices -- and the units are the model's.  Recovery and the
state rules are bl_beam_reweigh_pf's, through the same install."""
import ctypes as C

import numpy as np
import pytest

import botlab_amd as bl
from botlab_amd import _capi
import beam_model as bm
import clearance_model as cm
from test_gpu_beam import KEYS
from test_gpu_beam_filter import POSE_FIELDS, World, started

pytestmark = pytest.mark.gpu


class LeapWorld(World):
    """The beam filter tests' world with a clearance grid built on its map."""

    def __init__(self, ctx, cap=64):
        World.__init__(self, ctx)
        self.cl = bl.ClearanceGrid(ctx, cap)
        self.cl.build(self.grid, self.params["occ_min"])
        assert np.array_equal(self.cl.read(), cm.grid(self.case["cells"], self.params["occ_min"], cap))

    def close(self):
        self.cl.close()
        World.close(self)


@pytest.fixture(scope="module")
def world(gpu_ctx):
    w = LeapWorld(gpu_ctx)
    yield w
    w.close()


@pytest.mark.parametrize("n", [2, 64, 1000])
def test_reweigh_leaves_the_bytes_the_cast_leaves_on_a_twin(gpu_ctx, world, n):
    a, b = started(world, gpu_ctx, n), started(world, gpu_ctx, n)
    try:
        before = a.particles()
        assert before.tobytes() == b.particles().tobytes()
        scan = world.scans[1]
        pose_a = a.reweigh_beam_leap(world.beam, world.cl, scan)
        ua = world.beam.units(n)
        assert world.beam.debugPath() == 1
        pose_b = b.reweigh_beam(world.beam, world.grid, scan)
        ub = world.beam.units(n)
        assert np.array_equal(ua, ub)
        S, u = world.model_units(before, scan)
        assert np.array_equal(ua, u), (np.flatnonzero(ua != u)[:5], ua[:5], u[:5])
        print("n", n, "distinct units", len(set(u.tolist())), "at the floor", int((u == 1).sum()), "device ms", world.beam.lastDeviceMs())
        if n >= 64:
            assert len(set(u.tolist())) > 4                                  # (of the input: else the twin comparison says little)
        after = a.particles()
        for f in POSE_FIELDS:
            assert after[f].tobytes() == before[f].tobytes(), f             # poses and parents byte for byte
        est = a.poseEstimate()
        for p in (pose_a, est):
            assert (p.x, p.y, p.theta, p.utime) == (pose_b.x, pose_b.y, pose_b.theta, pose_b.utime)
        assert after.tobytes() == b.particles().tobytes()                    # the weights too
        assert a.debugUniformRuns() == b.debugUniformRuns() == 0
        for pf in (a, b):
            world.update(pf, 2, rand_value=846930886)
        assert np.array_equal(a.debugLast()[0], b.debugLast()[0])
        assert a.particles().tobytes() == b.particles().tobytes()
    finally:
        a.close()
        b.close()


def test_cloud_with_particles_off_the_grid(gpu_ctx, world):
    n = 64
    pf = bl.ParticleFilter(n, ctx=gpu_ctx)
    try:
        cloud = world.cloud(n)
        pf.setParticles(cloud)
        pf.reweigh_beam_leap(world.beam, world.cl, world.scans[0])
        S, u = world.model_units(cloud, world.scans[0])
        assert (S == bm.OFF_GRID).sum() == 2 and u[5] == 1 and u[17] == 1 and u.max() == 2 ** 20
        assert np.array_equal(world.beam.units(n), u)
        w = pf.particles()["weight"]
        assert np.array_equal(w, u.astype(np.float64) / float(u.astype(np.uint64).sum()))
    finally:
        pf.close()


def test_recovery_tracker_folds_the_sensor_update_behind_a_reweigh(gpu_ctx, world):
    """Recovery on and every update followed by a reweigh by leaps: the tracker goes on folding the SENSOR update's weight total,
    exactly as its model does with the totals read before each reweigh -- bl_beam_reweigh_pf's behaviour, through the same install."""
    import recovery_model as rcv
    n = 1000
    pf = bl.ParticleFilter(n, ctx=gpu_ctx)
    try:
        pf.setParticles(world.cloud(n))
        pf.setNoiseSeed(99)
        pf.setRecovery(world.grid, ratio=1e9, maxFraction=0.25, seed=77)
        world.update(pf, 0)
        tr = rcv.Tracker()
        S, sensed, utime = 0, False, world.scans[0].utime
        for u in range(1, 5):
            world.update(pf, u)
            st = pf.recoveryState()
            tr.step(u, S, n, sensed, ratio=1e9, max_fraction=0.25)
            assert (st["w_slow"], st["w_fast"], st["w_avg"], st["p_inject"], st["updates"], st["primed"]) == tr.as_tuple(), (u, st)
            S, sensed = pf.spread()["units_sum"], rcv.folds_next(utime if u == 1 else 0)
            for _ in range(2):                                               # the second reweigh of a record must not take the beam total
                pf.reweigh_beam_leap(world.beam, world.cl, world.scans[u])
            beam_total = int(world.beam.units(n).astype(np.uint64).sum())
            assert pf.spread()["units_sum"] == beam_total != S
        st = pf.recoveryState()
        assert st["primed"] == 1 and st["w_avg"] > 0 and st["p_inject"] == 0.25 and st["injected_total"] > 0
    finally:
        pf.close()


def test_state_errors_and_sharded_filters(gpu_ctx, world):
    fresh = bl.ParticleFilter(64, ctx=gpu_ctx)
    try:
        with pytest.raises(bl.BotlabHipError, match="status 4"):
            fresh.reweigh_beam_leap(world.beam, world.cl, world.scans[0])   # not initialised
    finally:
        fresh.close()
    pf = started(world, gpu_ctx, 64)
    try:
        before = pf.particles()
        assert pf.updateBegin(bl.make_pose(*world.odo[2], utime=world.scans[2].utime), world.scans[2], world.grid, 12345)
        with pytest.raises(bl.BotlabHipError, match="status 4"):
            pf.reweigh_beam_leap(world.beam, world.cl, world.scans[2])      # a pending update
        pf.updateEnd()
        now = pf.particles()
        unbuilt = bl.ClearanceGrid(gpu_ctx, 64)
        other = bm.params(**dict(world.params, occ_min=2))
        beam = bl.BeamModel(ctx=gpu_ctx, **{k: other[k] for k in KEYS})
        h = C.c_void_p()
        assert gpu_ctx.lib.bl_beam_create(gpu_ctx.h, C.byref(h)) == 0         # a beam model without parameters
        try:
            with pytest.raises(bl.BotlabHipError, match="status 4"):
                pf.reweigh_beam_leap(world.beam, unbuilt, world.scans[2])    # refused before anything is touched
            with pytest.raises(bl.BotlabHipError, match="status 4"):
                pf.reweigh_beam_leap(beam, world.cl, world.scans[2])         # another occ_min than the grid's
            ls, out = world.scans[2].as_c(), bl.Pose()
            assert gpu_ctx.lib.bl_clearance_reweigh_pf(h, pf.h, world.cl.h, C.byref(ls), C.byref(out)) == 4
            assert gpu_ctx.lib.bl_clearance_reweigh_pf(world.beam.h, None, world.cl.h, C.byref(ls), C.byref(out)) == 2
            assert pf.particles().tobytes() == now.tobytes() and now.tobytes() != before.tobytes()
        finally:
            gpu_ctx.lib.bl_beam_destroy(h)
            beam.close()
            unbuilt.close()
    finally:
        pf.close()
    # a composed shard: two ranks of one set on this device, each with the other's records mapped; refused as bl_beam_reweigh_pf
    # refuses it
    ranks = [bl.ParticleFilter(2048, ctx=gpu_ctx, shard=(r * 1024, (r + 1) * 1024)) for r in range(2)]
    try:
        ptrs = []
        for r, k in enumerate(ranks):
            k.initializeFilterAtPose(bl.make_pose(*world.odo[0], utime=world.scans[0].utime), seed=5)
            _capi.check(gpu_ctx.lib.bl_pf_shard_setup(k.h, r, 2, 1024))
            p3 = [C.c_void_p() for _ in range(3)]
            _capi.check(gpu_ctx.lib.bl_pf_shard_local_ptrs(k.h, *[C.byref(q) for q in p3]))
            ptrs.append([q.value for q in p3])
        for k in ranks:
            for r in range(2):
                _capi.check(gpu_ctx.lib.bl_pf_shard_set_peer(k.h, r, *ptrs[r]))
            _capi.check(gpu_ctx.lib.bl_pf_shard_commit(k.h))
            for reweigh, source in ((k.reweigh_beam_leap, world.cl), (k.reweigh_beam, world.grid)):
                with pytest.raises(bl.BotlabHipError, match="status 4"):
                    reweigh(world.beam, source, world.scans[0])
                assert b"shard" in gpu_ctx.lib.bl_last_error()
    finally:
        for k in ranks:
            k.close()
