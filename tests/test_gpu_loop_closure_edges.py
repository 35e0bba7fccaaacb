"""The loop-closure front end on the device at the limits tests/test_gpu_loop_closure_batch.py does not reach
(loop_closure_cases.edge_cases): more than 1024 queries and more than 256 candidates on a handle of 1024 slots; equal
minima of d2 within one lane and across lanes with the lower lane holding the higher j; a handle exactly full and one candidate short;
a second, smaller find on the 1024-slot handle.  Every comparison with the model is byte for byte, as there."""
import numpy as np
import pytest

import botlab_amd as bl

import loop_closure_cases as lcc
from test_gpu_loop_closure_batch import _assert_equals_model, _history, _like, _refused, _snapshot

pytestmark = pytest.mark.gpu


class _Find:
    """a case's history on the device and one find on a handle of `slots` candidates"""

    def __init__(self, ctx, case, slots):
        self.case = case
        self.history, self.like = _history(ctx, case), _like(ctx, case.mpc, case.cpm)
        self.lc = bl.LoopCloser(slots, ctx=ctx)
        self.edges = self.lc.find(self.history, self.like, **case.params)
        self.ms = self.lc.lastDeviceMs(split=True)
        self.cands = self.lc.candidates()
        self.submaps = [self.lc.submap(m) for m in range(len(self.cands))]

    def close(self):
        self.lc.close(); self.like.close(); self.history.close()


@pytest.fixture(scope="module")
def long_run(gpu_ctx):
    r = _Find(gpu_ctx, lcc.edge_cases()["long_log"], 1024)
    yield r
    r.close()


def test_long_log_equals_model(long_run):
    r = long_run
    model = lcc.model("long_log")
    assert r.case.reaches(model)
    assert len(r.history) == lcc.LONG_N > 1024                                    # slots = min(queries, 1024) = 1024, most of them idle
    print("long_log queries", len(r.history), "candidates", len(model), "kept", len(r.edges), "device ms", r.ms)
    assert len(r.cands) == len(model) >= 257
    _assert_equals_model(r.cands, r.submaps, r.edges, model)


def _long_sample(model, stride):
    """m = 0, 255, 256, M - 1, the last candidate of a query index <= 1023, the first of one >= 1024, and the first 16 kept ones"""
    M = len(model)
    below = max(m for m, c in enumerate(model) if c["q"] // stride <= 1023)
    above = min(m for m, c in enumerate(model) if c["q"] // stride >= 1024)
    assert above == below + 1
    kept = [m for m, c in enumerate(model) if c["flags"] == 0][:lcc.LONG_SAMPLE_KEPT]
    return sorted({0, 255, 256, M - 1, below, above, *kept})


def test_long_log_equals_the_per_candidate_calls(long_run, gpu_ctx):
    r = long_run
    p = r.case.params
    sample = _long_sample(lcc.model("long_log"), p["stride"])
    assert 22 >= len(sample) >= 6
    poses = r.history.poses()
    matcher = bl.ScanMatcher(ctx=gpu_ctx)
    try:
        for m in sample:
            c = r.cands[m]
            cells, origin = r.submaps[m]
            S = p["submap_cells"]
            sub = bl.OccupancyGrid(ctx=gpu_ctx, _raw=(S, S, r.like.mpc, r.like.cpm, origin[0], origin[1]))
            try:
                r.history.rebuild(sub, p["maxLaserDistance"], p["hitOdds"], p["missOdds"], first=int(c["first"]), count=int(c["count"]))
                assert np.array_equal(sub.cells(), cells), m
                assert not c["flags"] & bl.LC_TOO_MANY_RAYS
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


def test_second_find_on_the_long_handle_equals_a_fresh_one(long_run, gpu_ctx):
    """after test_long_log_*: 366 candidates, then one, on the same handle of 1024 slots"""
    big, small_name = long_run, lcc.SECOND_FIND_LONG[1]
    assert lcc.SECOND_FIND_LONG[0] == "long_log"
    small = _Find(gpu_ctx, lcc.cases()[small_name], 128)
    try:
        assert len(big.cands) > len(small.cands) >= 1
        edges = big.lc.find(small.history, small.like, **small.case.params)
        cands = big.lc.candidates()
        submaps = [big.lc.submap(m) for m in range(len(cands))]
        assert cands.tobytes() == small.cands.tobytes() and edges.tobytes() == small.edges.tobytes()
        for (cells, origin), (want_cells, want_origin) in zip(submaps, small.submaps):
            assert np.array_equal(cells, want_cells) and origin.tobytes() == want_origin.tobytes()
        _assert_equals_model(cands, submaps, edges, lcc.model(small_name))
        # and the long find again on the handle the small one has used
        edges = big.lc.find(big.history, big.like, **big.case.params)
        assert big.lc.candidates().tobytes() == big.cands.tobytes() and edges.tobytes() == big.edges.tobytes()
    finally:
        small.close()


@pytest.mark.parametrize("name", ["tie_same_lane", "tie_lane_order", "tie_three"])
def test_ties_take_the_lowest_index(gpu_ctx, name):
    case = lcc.edge_cases()[name]
    model = lcc.model(name)
    assert case.reaches(model)
    r = _Find(gpu_ctx, case, 4)
    try:
        print(name, "partner", int(r.cands["j"][0]) if len(r.cands) else None, "device ms", r.ms)
        _assert_equals_model(r.cands, r.submaps, r.edges, model)
    finally:
        r.close()


def test_handle_exactly_full_and_one_short(gpu_ctx):
    case = lcc.cases()["two_lap"]
    model = lcc.model("two_lap")
    M = len(model)
    assert case.reaches(model) and M >= 3
    history, like = _history(gpu_ctx, case), _like(gpu_ctx, case.mpc, case.cpm)
    full, short = bl.LoopCloser(M, ctx=gpu_ctx), bl.LoopCloser(M - 1, ctx=gpu_ctx)
    try:
        edges = full.find(history, like, **case.params)                           # M == max_candidates: accepted
        cands = full.candidates()
        assert len(cands) == M
        _assert_equals_model(cands, [full.submap(m) for m in range(M)], edges, model)
        one = short.find(history, like, **dict(case.params, stride=31))
        assert len(short.candidates()) == 1 == len(lcc.model("single"))
        before = _snapshot(short)
        _refused(lambda: short.find(history, like, **case.params))                # M == max_candidates + 1: refused
        assert _snapshot(short) == before and short.edges().tobytes() == one.tobytes()
    finally:
        short.close(); full.close(); like.close(); history.close()
