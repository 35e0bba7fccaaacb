"""bl_rangetable_reweigh_pf on the 64 x 48 map of tests/test_gpu_beam_filter.py: the units it installs are the table model's of the
filter's own poses, poses and parents stay byte for byte, and from then on the filter behaves as a twin that received the same units
through bl_pf_set_particles: the same posterior pose and the same resampling indices in the next update.  Recovery and the state rules
are bl_beam_reweigh_pf's."""
import numpy as np
import pytest

import botlab_amd as bl
import beam_model as bm
import range_table_model as rm
from test_gpu_beam import KEYS
from test_gpu_beam_filter import POSE_FIELDS, World, started

pytestmark = pytest.mark.gpu


class TableWorld(World):
    """The beam filter tests' world with a range table of 256 headings built on its map, and the model's table beside it."""

    def __init__(self, ctx):
        World.__init__(self, ctx)
        self.rt = bl.RangeTable(ctx, 256)
        self.rt.build(self.beam, self.grid)
        self.table = rm.build(self.case["cells"], self.rt.directions().astype(np.int64), self.params["occ_min"])
        self.table.setflags(write=False)
        assert np.array_equal(self.rt.read(), self.table)

    def model_units(self, parts, scan):
        c = self.case
        poses = np.stack([parts["x"], parts["y"], parts["theta"]], axis=1)
        S = rm.scores(self.table, c["origin"], c["cpm"], scan.ranges, scan.thetas, poses, self.params, self.tables)
        return S, bm.units(S, self.params["span"], bl.BeamModel.unitTable())

    def close(self):
        self.rt.close()
        World.close(self)


@pytest.fixture(scope="module")
def world(gpu_ctx):
    w = TableWorld(gpu_ctx)
    yield w
    w.close()


@pytest.mark.parametrize("n", [2, 64, 1000])
def test_reweigh_equals_a_twin_with_uploaded_units(gpu_ctx, world, n):
    a, b = started(world, gpu_ctx, n), started(world, gpu_ctx, n)
    try:
        before = a.particles()
        assert before.tobytes() == b.particles().tobytes()
        scan = world.scans[1]
        pose_a = a.reweigh_beam_table(world.beam, world.rt, scan)
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
    n = 64
    pf = bl.ParticleFilter(n, ctx=gpu_ctx)
    try:
        cloud = world.cloud(n)
        pf.setParticles(cloud)
        pf.reweigh_beam_table(world.beam, world.rt, world.scans[0])
        S, u = world.model_units(cloud, world.scans[0])
        assert (S == bm.OFF_GRID).sum() == 2 and u[5] == 1 and u[17] == 1 and u.max() == 2 ** 20
        assert np.array_equal(world.beam.units(n), u)
        w = pf.particles()["weight"]
        assert np.array_equal(w, u.astype(np.float64) / float(u.astype(np.uint64).sum()))
    finally:
        pf.close()


def test_recovery_tracker_folds_the_sensor_update_behind_a_reweigh(gpu_ctx, world):
    """Recovery on and every update followed by a reweigh by table: the tracker goes on folding the SENSOR update's weight total,
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
                pf.reweigh_beam_table(world.beam, world.rt, world.scans[u])
            beam_total = int(world.beam.units(n).astype(np.uint64).sum())
            assert pf.spread()["units_sum"] == beam_total != S
        st = pf.recoveryState()
        assert st["primed"] == 1 and st["w_avg"] > 0 and st["p_inject"] == 0.25 and st["injected_total"] > 0
    finally:
        pf.close()


def test_state_errors(gpu_ctx, world):
    fresh = bl.ParticleFilter(64, ctx=gpu_ctx)
    try:
        with pytest.raises(bl.BotlabHipError, match="status 4"):
            fresh.reweigh_beam_table(world.beam, world.rt, world.scans[0])   # not initialised
    finally:
        fresh.close()
    pf = started(world, gpu_ctx, 64)
    try:
        before = pf.particles()
        assert pf.updateBegin(bl.make_pose(*world.odo[2], utime=world.scans[2].utime), world.scans[2], world.grid, 12345)
        with pytest.raises(bl.BotlabHipError, match="status 4"):
            pf.reweigh_beam_table(world.beam, world.rt, world.scans[2])      # a pending update
        pf.updateEnd()
        now = pf.particles()
        unbuilt = bl.RangeTable(gpu_ctx, 256)
        other = bm.params(**dict(world.params, occ_min=2))
        beam = bl.BeamModel(ctx=gpu_ctx, **{k: other[k] for k in KEYS})
        try:
            with pytest.raises(bl.BotlabHipError, match="status 4"):
                pf.reweigh_beam_table(world.beam, unbuilt, world.scans[2])   # refused before anything is touched
            with pytest.raises(bl.BotlabHipError, match="status 4"):
                pf.reweigh_beam_table(beam, world.rt, world.scans[2])        # another occ_min than the table's
            assert pf.particles().tobytes() == now.tobytes() and now.tobytes() != before.tobytes()
        finally:
            beam.close()
            unbuilt.close()
    finally:
        pf.close()
