"""The loop-closure front end on the device (bl_loopclose_*, botlab_amd.LoopCloser) against its model and against the
per-candidate calls it batches.

On every named case (tests/loop_closure_cases.py) the device equals the model with nothing left out: the pair list, first / count, every
submap's bytes and origin, every result and moments record as bytes, the flags, the edges bit for bit.  On every case it also equals the
existing calls on the same handles: ScanHistory.rebuild into a grid of the submap's frame plus ScanMatcher.match_prior.  On the two-lap
case LoopCloser.find and find_loop_closures give the same (i, j) list, z and info within the bound the CPU test measured, and
close_loops keeps the same edges of either.  Every refusal leaves the previous results readable and unchanged."""
import ctypes as C
import math

import numpy as np
import pytest

import botlab_amd as bl
from botlab_amd import _capi

import loop_closure_cases as lcc
import loop_closure_model as lcm

pytestmark = pytest.mark.gpu

CHAIN_INFO = np.array([1 / 0.005 ** 2, 0.0, 1 / 0.005 ** 2, 0.0, 0.0, 1 / 0.003 ** 2])
NAMES = list(lcc.cases())


def _history(ctx, case):
    h = bl.ScanHistory(case.capacity, case.max_rays, ctx=ctx)
    for s, p in zip(case.scans, case.poses):
        h.append(s, bl.make_pose(p[0], p[1], p[2], utime=p[3]))
    return h


def _like(ctx, mpc=lcc.MPC, cpm=lcc.CPM):
    g = bl.OccupancyGrid(ctx=ctx, _raw=(lcc.SIZE, lcc.SIZE, np.float32(mpc), np.float32(cpm), np.float32(lcc.ORIGIN[0]), np.float32(lcc.ORIGIN[1])))
    assert g.mpc == np.float32(mpc) and g.cpm == np.float32(cpm)
    return g


class _Run:
    """a case's history on the device and one find on a fresh handle"""

    def __init__(self, ctx, name):
        self.case = lcc.cases()[name]
        self.history, self.like = _history(ctx, self.case), _like(ctx, self.case.mpc, self.case.cpm)
        self.lc = bl.LoopCloser(128, ctx=ctx)
        self.edges = self.lc.find(self.history, self.like, **self.case.params)
        self.cands = self.lc.candidates()
        self.submaps = [self.lc.submap(m) for m in range(len(self.cands))]

    def close(self):
        self.lc.close(); self.like.close(); self.history.close()


@pytest.fixture(scope="module")
def runs(gpu_ctx):
    made = {}

    def get(name):
        if name not in made:
            made[name] = _Run(gpu_ctx, name)
        return made[name]
    yield get
    for r in made.values():
        r.close()


def _assert_equals_model(cands, submaps, edges, model):
    want = lcm.records(model)
    assert [(int(c["q"]), int(c["j"])) for c in cands] == [(c["q"], c["j"]) for c in model]
    assert cands["first"].tolist() == want["first"].tolist() and cands["count"].tolist() == want["count"].tolist()
    for m, (c, (cells, origin)) in enumerate(zip(model, submaps)):
        assert origin.tobytes() == np.array(c["origin"], np.float32).tobytes(), m
        assert np.array_equal(cells, c["cells"]), (m, int(np.count_nonzero(cells != c["cells"])))
    assert cands["flags"].tolist() == want["flags"].tolist()
    for m in range(len(model)):
        assert cands["result"][m].tobytes() == want["result"][m].tobytes(), (m, cands["result"][m], want["result"][m])
        assert cands["moments"][m].tobytes() == want["moments"][m].tobytes(), (m, cands["moments"][m], want["moments"][m])
        assert cands["edge"][m].tobytes() == want["edge"][m].tobytes(), (m, cands["edge"][m], want["edge"][m])
    assert cands.tobytes() == want.tobytes()
    assert edges.tobytes() == lcm.edges(model).tobytes()
    assert edges["j"].tolist() == sorted(edges["j"].tolist())


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_model(runs, name):
    r = runs(name)
    model = lcc.model(name)
    assert r.case.reaches(model)
    print(name, "candidates", len(model), "kept", len(r.edges), "device ms", r.lc.lastDeviceMs(split=True) if len(r.history) >= 2 else None)
    _assert_equals_model(r.cands, r.submaps, r.edges, model)


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_the_per_candidate_calls(runs, gpu_ctx, name):
    r = runs(name)
    p = r.case.params
    poses = r.history.poses()
    matcher = bl.ScanMatcher(ctx=gpu_ctx)
    try:
        for m, c in enumerate(r.cands):
            cells, origin = r.submaps[m]
            S = p["submap_cells"]
            sub = bl.OccupancyGrid(ctx=gpu_ctx, _raw=(S, S, r.like.mpc, r.like.cpm, origin[0], origin[1]))
            try:
                r.history.rebuild(sub, p["maxLaserDistance"], p["hitOdds"], p["missOdds"], first=int(c["first"]), count=int(c["count"]))
                assert np.array_equal(sub.cells(), cells), m
                if c["flags"] & bl.LC_TOO_MANY_RAYS:
                    continue
                q = int(c["q"])
                rr, tt, ss = r.history.scan(q)
                scan = bl.LidarScan(rr, tt, ss, utime=int(poses["utime"][q]))
                centre = bl.make_pose(poses["x"][q], poses["y"][q], poses["theta"][q], utime=int(poses["utime"][q]))
                res, mom = matcher.match_prior(scan, centre, sub, prior=p["prior"], half_life=p["half_life"], nx=p["nx"], ny=p["ny"],
                                               ntheta=p["ntheta"], dtheta=p["dtheta"], max_range=p["max_range"], min_score=p["min_score"])
                assert bytes(res) == c["result"].tobytes(), (m, res, c["result"])
                assert bytes(mom) == c["moments"].tobytes(), (m, mom, c["moments"])
            finally:
                sub.close()
    finally:
        matcher.close()


def test_second_find_equals_a_fresh_handle(runs, gpu_ctx):
    big, small = (runs(n) for n in lcc.SECOND_FIND)
    assert len(big.cands) > len(small.cands) >= 1
    lc = bl.LoopCloser(128, ctx=gpu_ctx)
    try:
        lc.find(big.history, big.like, **big.case.params)
        edges = lc.find(small.history, small.like, **small.case.params)
        cands = lc.candidates()
        assert cands.tobytes() == small.cands.tobytes() and edges.tobytes() == small.edges.tobytes()
        for m in range(len(cands)):
            cells, origin = lc.submap(m)
            assert np.array_equal(cells, small.submaps[m][0]) and origin.tobytes() == small.submaps[m][1].tobytes()
        _assert_equals_model(cands, [lc.submap(m) for m in range(len(cands))], edges, lcc.model(lcc.SECOND_FIND[1]))
    finally:
        lc.close()


def test_two_lap_against_the_python_path(gpu_ctx):
    case = lcc.cases()["two_lap"]
    history, like = _history(gpu_ctx, case), _like(gpu_ctx)
    matcher, lc = bl.ScanMatcher(ctx=gpu_ctx), bl.LoopCloser(64, ctx=gpu_ctx)
    graph = bl.PoseGraph(len(case.scans), 64, 65, ctx=gpu_ctx)
    try:
        p = dict(case.params)
        dev = lc.find(history, like, **p)
        prior = p.pop("prior")
        assert prior == (0, 0, 0, 0)
        py = bl.find_loop_closures(history, matcher, like, **p)
        assert len(py) >= 3
        assert list(zip(py["i"].tolist(), py["j"].tolist())) == list(zip(dev["i"].tolist(), dev["j"].tolist()))
        worst_info = max(float(np.abs(a["info"] - b["info"]).max() / np.abs(a["info"]).max()) for a, b in zip(py, dev))
        worst_z = float(np.abs(py["z"] - dev["z"]).max())
        print("python path against the device: info", worst_info, "z", worst_z)
        assert worst_info <= lcc.INFO_REL_BOUND and worst_z <= lcc.Z_ABS_BOUND
        recorded = history.poses()
        kept_py = bl.close_loops(history, graph, py, CHAIN_INFO)[0]
        history.set_poses(0, recorded)
        kept_dev = bl.close_loops(history, graph, dev, CHAIN_INFO)[0]
        print("close_loops keeps", len(kept_py), "of", len(py))
        assert list(zip(kept_py["i"].tolist(), kept_py["j"].tolist())) == list(zip(kept_dev["i"].tolist(), kept_dev["j"].tolist()))
        assert len(kept_dev) >= 1
    finally:
        graph.close(); lc.close(); matcher.close(); like.close(); history.close()


def _snapshot(lc):
    c = lc.candidates()
    return c.tobytes(), lc.edges().tobytes(), [(a.tobytes(), b.tobytes()) for a, b in (lc.submap(m) for m in range(len(c)))]


def _refused(fn):
    with pytest.raises(bl.BotlabHipError, match="status 2"):
        fn()


def test_refusals_leave_the_last_results(runs, gpu_ctx):
    r = runs("two_lap")
    lib = gpu_ctx.lib
    h = C.c_void_p()
    assert lib.bl_loopclose_create(gpu_ctx.h, 0, C.byref(h)) == 2 and lib.bl_loopclose_create(gpu_ctx.h, 1025, C.byref(h)) == 2
    assert lib.bl_loopclose_create(None, 4, C.byref(h)) == 2 and lib.bl_loopclose_create(gpu_ctx.h, 4, None) == 2
    lc = bl.LoopCloser(128, ctx=gpu_ctx)
    other = bl.Context(0)
    other_history = bl.ScanHistory(4, 16, ctx=other)
    many = runs("wave_plus_one")
    try:
        ok = dict(r.case.params, stride=4)
        lc.find(r.history, r.like, **ok)
        before = _snapshot(lc)
        assert len(lc.candidates()) >= 2
        for bad in (dict(stride=0), dict(min_gap=-1), dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")), dict(w=32), dict(w=-1),
                    dict(submap_cells=15), dict(submap_cells=513), dict(hitOdds=-1), dict(missOdds=128), dict(nx=65), dict(ny=-1),
                    dict(ntheta=181), dict(dtheta=0.0), dict(half_life=0), dict(half_life=(1 << 20) + 1), dict(prior=(1, 2, 1, 0)),
                    dict(prior=(-1, 0, 0, 0)), dict(prior=(0, 0, 0, 32768))):
            _refused(lambda: lc.find(r.history, r.like, **dict(ok, **bad)))
            assert _snapshot(lc) == before, bad
        # keep_volume, null pointers, a log of another ctx: through the C ABI
        prm = _capi.LoopCloseParams(4, 6, 0.25, 3, 130, 5.0, 3, 1, _capi.ScanMatchParams(3, 3, 3, float(np.float32(math.radians(0.5))), 8.0, 0, 1),
                                    _capi.ScanMatchPrior(0, 0, 0, 0, 64, 1))
        n = C.c_int(-5)
        assert lib.bl_loopclose_find(lc.h, r.history.h, r.like.h, C.byref(prm), C.byref(n)) == 2 and n.value == -5
        prm.match.keep_volume = 0
        assert lib.bl_loopclose_find(None, r.history.h, r.like.h, C.byref(prm), C.byref(n)) == 2
        assert lib.bl_loopclose_find(lc.h, None, r.like.h, C.byref(prm), C.byref(n)) == 2
        assert lib.bl_loopclose_find(lc.h, r.history.h, None, C.byref(prm), C.byref(n)) == 2
        assert lib.bl_loopclose_find(lc.h, r.history.h, r.like.h, None, C.byref(n)) == 2
        assert lib.bl_loopclose_find(lc.h, r.history.h, r.like.h, C.byref(prm), None) == 2
        assert lib.bl_loopclose_find(lc.h, other_history.h, r.like.h, C.byref(prm), C.byref(n)) == 2
        assert lib.bl_loopclose_submap(lc.h, -1, None, None) == 2 and lib.bl_loopclose_submap(lc.h, len(lc.candidates()), None, None) == 2
        assert n.value == -5 and _snapshot(lc) == before
        # more than 1 GiB of submaps and volumes: 69 slots of 512 x 512 cells and 361 x 129 x 129 objectives
        _refused(lambda: lc.find(many.history, many.like, **dict(many.case.params, submap_cells=512, nx=64, ny=64, ntheta=180)))
        assert _snapshot(lc) == before
        # the same parameters are accepted: the last call's results replace the earlier ones
        assert lib.bl_loopclose_find(lc.h, r.history.h, r.like.h, C.byref(prm), C.byref(n)) == 0 and n.value == len(lc.candidates())
        assert _snapshot(lc) == before
    finally:
        other_history.close(); other.close(); lc.close()


def test_more_partners_than_the_handle_holds(runs, gpu_ctx):
    r = runs("two_lap")
    lc = bl.LoopCloser(2, ctx=gpu_ctx)
    try:
        edges = lc.find(r.history, r.like, **dict(r.case.params, stride=31, submap_cells=64))
        assert len(lc.candidates()) == 1
        before = _snapshot(lc)
        assert len(r.cands) > 2
        _refused(lambda: lc.find(r.history, r.like, **r.case.params))              # larger submaps too: the buffer grows, the old bytes stay
        assert _snapshot(lc) == before and lc.edges().tobytes() == edges.tobytes()
        again = lc.find(r.history, r.like, **dict(r.case.params, stride=31, submap_cells=64))
        assert again.tobytes() == edges.tobytes() and _snapshot(lc) == before
    finally:
        lc.close()


def test_short_logs_have_no_candidates(gpu_ctx):
    like = _like(gpu_ctx)
    case = lcc.cases()["two_lap"]
    history = bl.ScanHistory(4, case.max_rays, ctx=gpu_ctx)
    lc = bl.LoopCloser(4, ctx=gpu_ctx)
    try:
        assert len(lc.find(history, like, **dict(case.params, min_gap=0))) == 0 and len(lc.candidates()) == 0
        history.append(case.scans[0], bl.make_pose(0.0, 0.0, 0.0, utime=1))
        assert len(lc.find(history, like, **dict(case.params, min_gap=0))) == 0 and len(lc.candidates()) == 0
        with pytest.raises(bl.BotlabHipError, match="status 4"):
            lc.lastDeviceMs()
    finally:
        lc.close(); history.close(); like.close()
