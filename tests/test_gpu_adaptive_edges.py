"""Adaptive particle count on hand-built inputs (tests/adaptive_cases.py; each case's condition is proved on the model alone in
tests/test_adaptive_cases_cpu.py).

A. k_kld_count on parents chosen here: upload a cloud with equal units, latch the odometry (no move: the record stays), one moved
   update drawn with MID -- its exported parents are the cloud, pose for pose and bit for bit (asserted), and bins, k_sat and next are
   the model's on them.  Every comparison is exact.
B. Resampling updates at commanded (active, next) pairs: the in-kernel draw, the full-range draw of debugResample and the model's
   rule give the same indices, the exported parents are the previous record's poses at those indices bit for bit, and in strict
   parity mode the whole update equals the CPU reference run on the prior the indices name.
C. An all-floor record while active != capacity: its weight is the reference's serial sum over `active` floor weights, and the
   draws from it at other counts follow the reference's rule on those weights."""
import numpy as np
import pytest

import adaptive_cases as ac
import adaptive_model as am
import global_init_model as gm
import helpers
import oracle_lib
import recovery_model as rm
import botlab_amd as bl
from botlab_amd import synth
from botlab_amd.host import PARTICLE_DTYPE

pytestmark = pytest.mark.gpu
REL = 1e-5                                   # particle poses after an update, as in test_gpu_adaptive.py / test_gpu_parity.py
RAND_VALUES = [0, 1, 12345, am.RAND_MAX // 2, am.RAND_MAX - 1, am.RAND_MAX, 1804289383, 846930886]


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


class Rig:
    """A map, two scans and the two odometry poses they end at; a filter driven over it goes back and forth between the two."""

    def __init__(self, gpu_ctx, cells, origin, mpc, scans, odo):
        self.ctx, self.cells, self.origin, self.mpc, self.scans, self.odo = gpu_ctx, cells, origin, mpc, scans, odo
        self.cpm = helpers.CPM_DEFAULT
        self.g = bl.OccupancyGrid.from_cells(cells, origin, mpc, cellsPerMeter=self.cpm, ctx=gpu_ctx)
        self.at = 0

    def start(self, particles, units=None):
        """A filter holding `particles`, debug on, the odometry latched at odo[0] by an update that does not move."""
        pf = bl.ParticleFilter(len(particles), ctx=self.ctx)
        pf.setParticles(particles, units)
        pf.debugEnable(True)
        before = pf.particles()
        self.at = 0
        assert not pf.updateBegin(bl.make_pose(*self.odo[0], utime=self.scans[0].utime), self.scans[0], self.g, 777)
        pf.updateEnd(want_pose=False)
        assert pf.particles().tobytes() == before.tobytes()          # the uploaded record stands
        return pf

    def move(self):
        """(previous odometry, odometry, scan) of the next moved update."""
        prev = self.odo[self.at]
        self.at ^= 1
        return prev, self.odo[self.at], self.scans[self.at]


@pytest.fixture(scope="module")
def free_rig(gpu_ctx):
    scans, odo = ac.travel_scans()
    rig = Rig(gpu_ctx, ac.free_map(), ac.FREE_ORIGIN, ac.FREE_MPC, scans, odo)
    yield rig
    rig.g.close()


@pytest.fixture(scope="module")
def track_rig(maps, gpu_ctx):
    m = maps[gm.CAL_MAP]
    truth = np.where(m["cells"] > 0, 127, -127).astype(np.int8)
    poses = synth.square_trajectory(ac.TRACK_START, 3, step_len=0.02, turn=0.05, side=0.8)
    scans = [synth.raycast_scan(truth, m["origin"], 0.05, poses[k - 1], poses[k], 1_000_000 + k * 100_000) for k in (1, 2)]
    rig = Rig(gpu_ctx, m["cells"], m["origin"], m["mpc"], scans, [tuple(poses[1]), tuple(poses[2])])
    yield rig
    rig.g.close()


def _set_adaptive(pf, p):
    pf.setAdaptive(minParticles=p.min_particles, epsilon=p.epsilon, z=p.z, binXY=p.bin_xy, binTheta=p.bin_theta)


# ---------------------------------------------------------------- A: the count on hand-built parents
@pytest.mark.parametrize("case", ac.count_cases(), ids=lambda c: c.name)
def test_count_on_hand_built_parents(free_rig, case):
    p = case.params
    model = am.CountModel(case.cap, p)
    pf = free_rig.start(ac.as_particles(case, free_rig.scans[0].times[0], PARTICLE_DTYPE), np.full(case.cap, 7, np.uint32))
    try:
        _set_adaptive(pf, p)
        st = pf.adaptiveState()
        assert (st["active"], st["next"], st["bins"], st["counts"], st["k_sat"]) == (case.cap, case.cap, 0, 0, model.ksat), st
        _, od, scan = free_rig.move()
        assert pf.updateBegin(bl.make_pose(*od, utime=scan.utime), scan, free_rig.g, ac.MID)
        pf.updateEnd(want_pose=False)
        idx, _ = pf.debugLast()
        assert np.array_equal(idx, np.arange(case.cap))                              # the draw kept every pose where it was
        parts = pf.particles()
        assert len(parts) == case.cap
        for f, v in (("p_x", case.x), ("p_y", case.y), ("p_theta", case.th)):
            assert np.array_equal(_bits(parts[f]), _bits(v)), (case.name, f)         # ... so the parents counted are the case, bit for bit
        # the case's condition on the exported parents themselves: the distinct bins its builder states, by math.floor
        assert len(ac.explicit_bins(parts["p_x"], parts["p_y"], parts["p_theta"], p.bin_xy, p.bin_theta)) == case.k
        model.counted(parts["p_x"], parts["p_y"], parts["p_theta"])
        st = pf.adaptiveState()
        print(case.name, st, (model.active, model.bins, model.ksat, model.next))
        assert (st["active"], st["bins"], st["k_sat"], st["next"], st["counts"]) == (model.active, model.bins, model.ksat, model.next, 1), (case.name, st)
        assert st["bins"] == min(case.k, model.ksat)
    finally:
        pf.close()


# ---------------------------------------------------------------- B: updates at commanded counts
def _expected_draw(pf, post, units, strict, rv, nxt):
    """The model's indices of the next draw of nxt particles from the record post (units: its weight units, None for an upload of
    equal units): the reference's rule in strict mode or on equal weights (an upload, the all-floor set), else the integer rule."""
    equal = units is None or bool(np.all(units == 2))
    if not strict:
        assert (pf.debugUniformRuns() > 0) == equal
    if strict or equal:
        return am.resample_reference(post["weight"], rv, nxt)
    return am.resample_integer(units, rv, nxt)


def _checked_update(rig, pf, cap, strict, rv, units, oracle=None):
    """One resampling update at the (active, next) the filter stands at, checked; returns ((active, next), units of the new record)."""
    st = pf.adaptiveState()
    active, nxt = st["active"], st["next"]
    post = pf.particles()
    assert len(post) == active
    want = _expected_draw(pf, post, units, strict, rv, nxt)
    before = pf.debugResample(rv)
    assert np.array_equal(before, want), (active, nxt, rv)                           # the full-range search
    prev, od, scan = rig.move()
    pose_od = bl.make_pose(*od, utime=scan.utime)
    if oracle is None:
        assert pf.updateBegin(pose_od, scan, rig.g, rv)
        pf.updateEnd(want_pose=False)
    else:
        # the whole update against the reference filter on the prior of nxt particles (as test_next_differs_from_active)
        prior = post[want].copy()
        prior["weight"] = 1.0 / nxt
        opf = oracle_lib.OraclePF(oracle, nxt)
        opf.set_particles(prior)
        args = (rig.cells, rig.mpc, rig.cpm, rig.origin)
        assert not opf.update(oracle.pose(*prev, utime=scan.utime - 1), scan, *args, 1)["moved"]
        res = opf.update(oracle.pose(*od, utime=scan.utime), scan, *args, ac.MID)
        assert res["moved"] and np.array_equal(res["idx"], np.arange(nxt))
        assert res["noise"].size == 3 * nxt
        pose = pf.updateFilter(pose_od, scan, rig.g, rand_value=rv, noise=res["noise"])
    parts = pf.particles()
    st2 = pf.adaptiveState()
    assert len(parts) == nxt == st2["active"], (active, nxt, st2)
    idx, like = pf.debugLast()
    assert np.array_equal(idx, want), (active, nxt, rv)                              # the search inside the update kernel
    for f in ("x", "y", "theta"):
        assert np.array_equal(_bits(parts["p_" + f]), _bits(post[f][want])), (active, nxt, f)      # the right records were copied
    if oracle is not None:
        exp = opf.particles()
        assert np.array_equal(like.astype(np.float64) * 0.5, res["raw"]), (active, nxt)
        for f in ("x", "y", "theta"):
            assert np.allclose(parts[f], exp[f], rtol=REL, atol=1e-7), (active, nxt, f)
        assert np.allclose(parts["weight"], exp["weight"], rtol=REL, atol=0), (active, nxt)
        est = oracle_lib.OPose()
        oracle.lib.orc_estimate_pose(np.ascontiguousarray(parts).ctypes.data, nxt, est)
        assert _bits([pose.x, pose.y, pose.theta]).tobytes() == _bits([est.x, est.y, est.theta]).tobytes(), (active, nxt)
    return (active, nxt), rm.units_of(like.astype(np.float64) * 0.5), st2, parts


def _run_chain(rig, cap, targets, strict, required, oracle=None, parity_pairs=()):
    pf = rig.start(ac.track_cloud(cap, PARTICLE_DTYPE, rig.scans[0].times[0]))
    try:
        pf.setStrictResampling(strict)
        units, seen, n_up = None, [], 0

        def step(model, commanded):
            nonlocal units, n_up
            st = pf.adaptiveState()
            use_oracle = oracle if (st["active"], st["next"]) in parity_pairs else None
            pair, units, st2, parts = _checked_update(rig, pf, cap, strict, RAND_VALUES[n_up % len(RAND_VALUES)], units, use_oracle)
            n_up += 1
            seen.append(pair)
            assert not np.all(units == units[0])                                     # a real scan on a real map: unequal weights, so the next draw is the integer rule's
            if model is None:                                                        # adaptive mode off: the capacity, no count
                assert (st2["active"], st2["next"], st2["k_sat"]) == (cap, cap, 0), st2
            else:
                model.counted(parts["p_x"], parts["p_y"], parts["p_theta"])
                assert (st2["active"], st2["bins"], st2["k_sat"], st2["next"]) == (model.active, model.bins, model.ksat, model.next), st2
                assert st2["bins"] == 1 and st2["next"] == commanded, st2            # the cloud is in one bin: the command holds

        pf.setAdaptive(minParticles=cap, **ac.ONE_BIN)
        step(am.CountModel(cap, am.Params(cap, ac.ONE_BIN["epsilon"], ac.Z, ac.ONE_BIN["binXY"], ac.ONE_BIN["binTheta"])), cap)
        for t in targets:
            if t is None:
                pf.setAdaptive(None)
                step(None, cap)
            else:
                pf.setAdaptive(minParticles=t, **ac.ONE_BIN)
                model = am.CountModel(cap, am.Params(t, ac.ONE_BIN["epsilon"], ac.Z, ac.ONE_BIN["binXY"], ac.ONE_BIN["binTheta"]))
                step(model, t)                                                       # settles: active -> active, its count commands t
                step(model, t)
        assert seen == ac.chain_pairs(cap, targets), seen
        assert set(required) <= set(seen)
    finally:
        pf.close()


@pytest.mark.parametrize("strict", [False, True], ids=["default", "strict"])
@pytest.mark.parametrize("name", list(ac.CHAINS))
def test_updates_at_commanded_counts(track_rig, name, strict):
    cap, targets = ac.CHAINS[name]
    _run_chain(track_rig, cap, targets, strict, ac.REQUIRED_PAIRS[name])


@pytest.mark.parametrize("name", list(ac.PARITY_CHAINS))
def test_whole_update_equals_the_reference_at_commanded_counts(oracle, track_rig, name):
    """Strict parity mode: 3 * next noise floats from the reference, likelihood halves exact, the estimate's bits those of the
    reference's estimatePosteriorPose on the exported particles, poses and weights within REL."""
    cap, targets = ac.PARITY_CHAINS[name]
    _run_chain(track_rig, cap, targets, True, ac.PARITY_PAIRS[name], oracle=oracle, parity_pairs=ac.PARITY_PAIRS[name])


# ---------------------------------------------------------------- C: an all-floor record at active != capacity
@pytest.mark.parametrize("strict", [False, True], ids=["default", "strict"])
def test_all_floor_record_below_the_capacity(oracle, free_rig, strict):
    cap, n, nxt = ac.FLOOR_CAP, ac.FLOOR_ACTIVE, ac.FLOOR_NEXT
    opf = oracle_lib.OraclePF(oracle, n)                                             # the reference's computeNormalizedPosterior of n floor weights
    opf.set_particles(ac.track_cloud(n, PARTICLE_DTYPE, 1000))
    assert np.all(ac.floor_update(oracle, opf)["raw"] <= 0.001)
    w_ref = opf.particles()["weight"]
    assert w_ref[0] == ac.serial_floor_weight(n)
    pf = free_rig.start(ac.track_cloud(cap, PARTICLE_DTYPE, free_rig.scans[0].times[0]))
    try:
        pf.setStrictResampling(strict)
        units, seen = None, []

        def step(k):
            nonlocal units
            pair, units, st2, parts = _checked_update(free_rig, pf, cap, strict, RAND_VALUES[k % len(RAND_VALUES)], units)
            seen.append(pair)
            assert np.all(units == 2)                                                # every likelihood at the floor
            assert pf.debugUniformRuns() > 0
            return parts

        pf.setAdaptive(minParticles=n, **ac.ONE_BIN)
        step(0)                                                                      # cap -> cap: its count commands n
        for k in (1, 2):                                                             # cap -> n, n -> n: all-floor records of n != cap particles
            parts = step(k)
            assert len(parts) == n
            assert parts["weight"].tobytes() == w_ref.tobytes()
        pf.setAdaptive(minParticles=nxt, **ac.ONE_BIN)
        step(3)                                                                      # n -> n again: commands nxt
        parts = step(4)                                                              # n -> nxt, drawn from the all-floor record
        assert np.array_equal(parts["weight"], np.full(nxt, ac.serial_floor_weight(nxt)))
        pf.setAdaptive(None)
        parts = step(5)                                                              # nxt -> cap
        assert np.array_equal(parts["weight"], np.full(cap, ac.serial_floor_weight(cap)))
        assert seen == [(cap, cap), (cap, n), (n, n), (n, n), (n, nxt), (nxt, cap)], seen
    finally:
        pf.close()
