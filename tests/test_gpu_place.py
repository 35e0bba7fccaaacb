"""Loop closure by place recognition on the device (bl_loopclose_find_places, botlab_amd.LoopCloser.find_places)
against its model and against the per-candidate calls it batches.

On every named case (tests/place_cases.py) the device equals the model with nothing left out: the descriptors and their counts, the
record of every query, the candidates, first / count, every submap's bytes and origin, every result and moments record as bytes, the
flags, the edges bit for bit.  It also equals ScanHistory.rebuild + ScanMatcher.match_prior at the place centre per candidate (on the
long case: a stated sample).  find and find_places on one handle, in either order, equal fresh handles; a handle exactly full is
accepted and one candidate more is refused with the earlier results kept; so is every other refusal.  End to end on the drift case,
where the pair search finds nothing, find_places + close_loops lowers the largest position error against truth."""
import ctypes as C
import math

import numpy as np
import pytest

import botlab_amd as bl
from botlab_amd import _capi

import loop_closure_cases as lcc
import place_cases as pc
import place_model as pm
from test_gpu_loop_closure_batch import _assert_equals_model, _history, _like, _refused, _snapshot

pytestmark = pytest.mark.gpu

NAMES = list(pc.cases())


class _Run:
    """a case's history on the device and one find_places on a fresh handle"""

    def __init__(self, ctx, case, slots=128):
        self.case = case
        self.history, self.like = _history(ctx, case), _like(ctx, case.mpc, case.cpm)
        self.lc = bl.LoopCloser(slots, ctx=ctx)
        self.edges = self.lc.find_places(self.history, self.like, **case.params)
        self.ms = self.lc.lastDeviceMs(split=True) if len(self.history) >= 2 else None
        self.cands = self.lc.candidates()
        self.submaps = [self.lc.submap(m) for m in range(len(self.cands))]
        self.places = self.lc.places()
        self.words, self.bits = self.lc.descriptors()

    def close(self):
        self.lc.close(); self.like.close(); self.history.close()


@pytest.fixture(scope="module")
def runs(gpu_ctx):
    made = {}

    def get(name):
        if name not in made:
            made[name] = _Run(gpu_ctx, pc.long_case() if name == "long_log" else pc.cases()[name], 1024 if name == "long_log" else 128)
        return made[name]
    yield get
    for r in made.values():
        r.close()


def _assert_equals_place_model(r, model):
    words, bits, places, cands = model
    assert r.words.shape == words.shape and np.array_equal(r.bits, bits), (r.bits.tolist(), bits.tolist())
    assert np.array_equal(r.words, words), np.argwhere(r.words != words)[:8].tolist()
    for got, want in zip(r.places, places):
        assert got.tobytes() == want.tobytes(), (got, want)
    assert r.places.tobytes() == places.tobytes()
    _assert_equals_model(r.cands, r.submaps, r.edges, cands)


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_model(runs, name):
    r = runs(name)
    model = pc.model(name)
    assert r.case.reaches(model)
    print(name, "queries", len(model[2]), "candidates", len(model[3]), "kept", len(r.edges), "device ms", r.ms)
    _assert_equals_place_model(r, model)


def _assert_equals_the_calls(r, ctx, sample):
    p = r.case.params
    poses = r.history.poses()
    by_q = {int(pl["q"]): pl for pl in r.places}
    matcher = bl.ScanMatcher(ctx=ctx)
    try:
        for m in sample:
            c = r.cands[m]
            cells, origin = r.submaps[m]
            S = p["submap_cells"]
            sub = bl.OccupancyGrid(ctx=ctx, _raw=(S, S, r.like.mpc, r.like.cpm, origin[0], origin[1]))
            try:
                r.history.rebuild(sub, p["maxLaserDistance"], p["hitOdds"], p["missOdds"], first=int(c["first"]), count=int(c["count"]))
                assert np.array_equal(sub.cells(), cells), m
                if c["flags"] & bl.LC_TOO_MANY_RAYS:
                    continue
                q, j = int(c["q"]), int(c["j"])
                assert by_q[q]["partner"] == j
                rr, tt, ss = r.history.scan(q)
                scan = bl.LidarScan(rr, tt, ss, utime=int(poses["utime"][q]))
                x, y, th = pm.centre((poses["x"][j], poses["y"][j], poses["theta"][j]), int(by_q[q]["shift"]))
                centre = bl.make_pose(float(x), float(y), float(th), utime=int(poses["utime"][q]))
                assert np.float32(centre.theta) == th
                res, mom = matcher.match_prior(scan, centre, sub, prior=p["prior"], half_life=p["half_life"], nx=p["nx"], ny=p["ny"],
                                               ntheta=p["ntheta"], dtheta=p["dtheta"], max_range=p["max_range"], min_score=p["min_score"])
                assert bytes(res) == c["result"].tobytes(), (m, res, c["result"])
                assert bytes(mom) == c["moments"].tobytes(), (m, mom, c["moments"])
            finally:
                sub.close()
    finally:
        matcher.close()


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_the_per_candidate_calls(runs, gpu_ctx, name):
    r = runs(name)
    _assert_equals_the_calls(r, gpu_ctx, range(len(r.cands)))


def test_long_log_equals_model(runs):
    r = runs("long_log")
    model = pc.model("long_log")
    assert r.case.reaches(model)
    assert len(r.history) == pc.LONG_N > 1024 and len(r.places) == pc.LONG_N
    print("long_log queries", len(r.places), "candidates", len(model[3]), "kept", len(r.edges), "device ms", r.ms)
    assert len(r.cands) == len(model[3]) >= 257
    _assert_equals_place_model(r, model)


def test_long_log_equals_the_per_candidate_calls(runs, gpu_ctx):
    """m = 0, 255, 256, M - 1, the last candidate of a query index <= 1023, the first of one >= 1024, and the first 8 kept ones"""
    r = runs("long_log")
    cands = pc.model("long_log")[3]
    below = max(m for m, c in enumerate(cands) if c["q"] <= 1023)
    above = min(m for m, c in enumerate(cands) if c["q"] >= 1024)
    assert above == below + 1
    kept = [m for m, c in enumerate(cands) if c["flags"] == 0][:pc.LONG_SAMPLE_KEPT]
    sample = sorted({0, 255, 256, len(cands) - 1, below, above, *kept})
    assert 14 >= len(sample) >= 6
    _assert_equals_the_calls(r, gpu_ctx, sample)


def _place_snapshot(lc):
    w, b = lc.descriptors()
    return lc.places().tobytes(), w.tobytes(), b.tobytes()


def test_find_and_find_places_on_one_handle_equal_fresh_handles(runs, gpu_ctx):
    place = runs("stride_3")
    pose_case = lcc.cases()["two_lap"]
    history, like = _history(gpu_ctx, pose_case), _like(gpu_ctx, pose_case.mpc, pose_case.cpm)
    fresh, lc, other = bl.LoopCloser(128, ctx=gpu_ctx), bl.LoopCloser(128, ctx=gpu_ctx), bl.LoopCloser(128, ctx=gpu_ctx)
    try:
        want_edges = fresh.find(history, like, **pose_case.params)
        want = _snapshot(fresh)
        assert len(fresh.candidates()) > len(place.cands) >= 1
        # find_places, then find: the pose path is what it was, and the place results stay
        assert lc.find_places(place.history, place.like, **place.case.params).tobytes() == place.edges.tobytes()
        assert _snapshot(lc) == _snapshot(place.lc)
        placed = _place_snapshot(lc)
        assert placed == _place_snapshot(place.lc)
        assert lc.find(history, like, **pose_case.params).tobytes() == want_edges.tobytes() and _snapshot(lc) == want
        assert _place_snapshot(lc) == placed
        # find, then find_places
        assert other.find(history, like, **pose_case.params).tobytes() == want_edges.tobytes()
        assert other.find_places(place.history, place.like, **place.case.params).tobytes() == place.edges.tobytes()
        assert _snapshot(other) == _snapshot(place.lc) and _place_snapshot(other) == placed
    finally:
        other.close(); lc.close(); fresh.close(); like.close(); history.close()


def test_handle_exactly_full_and_one_short(runs, gpu_ctx):
    r = runs("stride_3")
    M = len(r.cands)
    assert M >= 3
    full, short = bl.LoopCloser(M, ctx=gpu_ctx), bl.LoopCloser(M - 1, ctx=gpu_ctx)
    try:
        edges = full.find_places(r.history, r.like, **r.case.params)                 # M == max_candidates: accepted
        assert len(full.candidates()) == M and edges.tobytes() == r.edges.tobytes() and _snapshot(full) == _snapshot(r.lc)
        one = short.find_places(r.history, r.like, **dict(r.case.params, stride=23))
        assert len(short.candidates()) == 1
        before = _snapshot(short)
        _refused(lambda: short.find_places(r.history, r.like, **r.case.params))     # M == max_candidates + 1: refused
        assert _snapshot(short) == before and short.edges().tobytes() == one.tobytes()
        # the refused call did launch: the diagnostics are its own
        assert _place_snapshot(short) == _place_snapshot(r.lc)
    finally:
        short.close(); full.close()


def test_refusals_leave_the_last_results(runs, gpu_ctx):
    r = runs("stride_3")
    lib = gpu_ctx.lib
    lc = bl.LoopCloser(128, ctx=gpu_ctx)
    other = bl.Context(0)
    other_history = bl.ScanHistory(4, 16, ctx=other)
    try:
        n = C.c_int(-5)
        assert lib.bl_loopclose_places(lc.h, C.byref(n), None) == 4 and lib.bl_loopclose_descriptors(lc.h, C.byref(n), None, None) == 4
        with pytest.raises(bl.BotlabHipError, match="status 4"):
            lc.places()
        ok = dict(r.case.params)
        lc.find_places(r.history, r.like, **ok)
        before, placed = _snapshot(lc), _place_snapshot(lc)
        assert len(lc.candidates()) >= 2
        for bad in (dict(bins_per_meter=0.0), dict(bins_per_meter=-2.0), dict(bins_per_meter=1000.5), dict(bins_per_meter=float("nan")),
                    dict(place_max_range=0.15), dict(place_max_range=1000.5), dict(place_max_range=float("nan")), dict(dilate=2), dict(dilate=-1),
                    dict(min_key=-1), dict(min_key=65537), dict(min_bits=-1), dict(min_bits=2049),
                    dict(stride=0), dict(min_gap=-1), dict(w=32), dict(w=-1), dict(submap_cells=15), dict(submap_cells=513), dict(hitOdds=-1),
                    dict(missOdds=128), dict(nx=65), dict(ny=-1), dict(ntheta=181), dict(dtheta=0.0), dict(half_life=0),
                    dict(half_life=(1 << 20) + 1), dict(prior=(1, 2, 1, 0)), dict(prior=(-1, 0, 0, 0)), dict(prior=(0, 0, 0, 32768))):
            _refused(lambda: lc.find_places(r.history, r.like, **dict(ok, **bad)))
            assert _snapshot(lc) == before and _place_snapshot(lc) == placed, bad
        for fine in (dict(bins_per_meter=1000.0), dict(place_max_range=1000.0), dict(min_key=65536), dict(min_bits=2048)):
            lc.find_places(r.history, r.like, **dict(ok, **fine))
        lc.find_places(r.history, r.like, **ok)
        assert _snapshot(lc) == before and _place_snapshot(lc) == placed
        # keep_volume, null pointers, a log of another ctx: through the C ABI.  The radius is not read: NaN is accepted.
        p = r.case.params
        prm = _capi.LoopCloseParams(p["stride"], p["min_gap"], float("nan"), p["w"], p["submap_cells"], 5.0, 3, 1,
                                    _capi.ScanMatchParams(p["nx"], p["ny"], p["ntheta"], float(np.float32(p["dtheta"])), 8.0, 0, 1),
                                    _capi.ScanMatchPrior(0, 0, 0, 0, 64, 1))
        pl = _capi.PlaceParams(4.0, 8.0, 1, 16384, 8)
        args = [lc.h, r.history.h, r.like.h, C.byref(prm), C.byref(pl), C.byref(n)]
        assert lib.bl_loopclose_find_places(*args) == 2 and n.value == -5           # keep_volume
        prm.match.keep_volume = 0
        for k in range(6):
            assert lib.bl_loopclose_find_places(*[None if i == k else a for i, a in enumerate(args)]) == 2
        assert lib.bl_loopclose_find_places(lc.h, other_history.h, r.like.h, C.byref(prm), C.byref(pl), C.byref(n)) == 2
        assert lib.bl_loopclose_places(lc.h, None, None) == 2 and lib.bl_loopclose_descriptors(lc.h, None, None, None) == 2
        assert n.value == -5 and _snapshot(lc) == before and _place_snapshot(lc) == placed
        assert lib.bl_loopclose_find_places(*args) == 0 and n.value == len(lc.candidates())
        assert _snapshot(lc) == before and _place_snapshot(lc) == placed
    finally:
        other_history.close(); other.close(); lc.close()


def test_short_logs_have_no_candidates(gpu_ctx):
    case = pc.cases()["stride_3"]
    like = _like(gpu_ctx)
    history = bl.ScanHistory(4, case.max_rays, ctx=gpu_ctx)
    lc = bl.LoopCloser(4, ctx=gpu_ctx)
    try:
        assert len(lc.find_places(history, like, **dict(case.params, min_gap=0))) == 0 and len(lc.candidates()) == 0
        history.append(case.scans[0], bl.make_pose(0.0, 0.0, 0.0, utime=1))
        assert len(lc.find_places(history, like, **dict(case.params, min_gap=0))) == 0 and len(lc.candidates()) == 0
        with pytest.raises(bl.BotlabHipError, match="status 4"):
            lc.places()                                                            # nothing was launched
    finally:
        lc.close(); history.close(); like.close()


# The chain's information, one value for every odometry edge as close_loops takes it, has to be honest about the drift: 0.72 m that
# built up over the 46 edges from entry 14 to entry 60, 0.0157 m an edge and all one way, so it adds up linearly where the gate's
# model, a random walk, adds up by the root.  The per-edge sigma under which the 0.72 m over a lap of 60 edges lie just at the gate
# (chi2 = 11.345) is 0.72 / sqrt(60 * 11.345) = 0.028 m; 0.05 m is taken, about twice that (chi2 = 3.5).  With the 5 mm of the
# pose-mode tests every true edge would be thrown out (chi2 = 346).  The heading did not drift: its sigma is the pose-mode tests'.
DRIFT_CHAIN_INFO = np.array([1 / 0.05 ** 2, 0.0, 1 / 0.05 ** 2, 0.0, 0.0, 1 / 0.003 ** 2])


def test_drift_end_to_end(runs, gpu_ctx):
    r = runs("drift")
    case = r.case
    graph = bl.PoseGraph(len(case.scans), 64, 65, ctx=gpu_ctx)
    lc = bl.LoopCloser(64, ctx=gpu_ctx)
    try:
        pose_params = {k: v for k, v in case.params.items() if k not in pm.PLACE_DEFAULTS}
        assert len(lc.find(r.history, r.like, radius=pc.DRIFT_RADIUS, **pose_params)) == 0 and len(lc.candidates()) == 0
        assert len(r.edges) >= 1
        recorded = r.history.poses()
        truth = case.truth

        def worst(p):
            return float(np.hypot(p["x"] - truth[:, 0], p["y"] - truth[:, 1]).max())
        before = worst(recorded)
        try:
            kept = bl.close_loops(r.history, graph, r.edges, DRIFT_CHAIN_INFO)[0]
            after = worst(r.history.poses())
        finally:
            r.history.set_poses(0, recorded)
        print("drift: edges", len(r.edges), "kept by close_loops", len(kept), "largest position error before", before, "after", after)
        assert abs(before - math.hypot(*pc.DRIFT_XY)) < 1e-5 and len(kept) >= 1
        assert after < before
    finally:
        lc.close(); graph.close()
