"""bl.RBSlam with scan-matched proposals (bl_rbslam_set_scan_matching, botlab_amd/csrc/bl_rbslam_match.h) against the model
(tests/rb_slam_match_model.py), bit for bit and byte for byte: after EVERY update what tests/test_gpu_rb_slam.py compares -- moved,
resampled, the resample indices, the likelihood half-units, cumulative scores, units, S, Q, the best index, all poses and ALL P maps --
and debugMatch()'s seven arrays.  The inputs and the model's side of every run are tests/test_rb_slam_match_model_cpu.py's (CASES,
record), which also shows that each input reaches the condition it is there for."""
import math

import numpy as np
import pytest

import botlab_amd as bl
import rb_slam_match_model as rmm
from test_gpu_rb_slam import POSE_FIELDS
from test_rb_slam_match_model_cpu import CASES, DTH, HIT, MAX_LASER, MISS, _case, record

pytestmark = pytest.mark.gpu


def _device(gpu_ctx, c, mdl_parts):
    H, W = c["shape"]
    rb = bl.RBSlam(c["P"], W, H, c["mpc"], c["cpm"], c["origin"], MAX_LASER, HIT, MISS, ctx=gpu_ctx)
    rb.setResampling(c["num"], c["den"])
    o = c["odoms"][0]
    rb.initializeAtPose(bl.make_pose(o[0], o[1], o[2], utime=1000), seed=1)
    rb.setParticles(mdl_parts)
    if c["init_maps"] is not None:
        for p in range(c["P"]):
            rb.uploadMap(p, c["init_maps"][p])
    return rb


def _compare(rb, s, r_g, k, maps_of=None):
    r_m = s["r"]
    assert r_g["moved"] == r_m["moved"] and r_g["resampled"] == r_m["resampled"], k
    parts, cum, units = rb.particles()
    for f in POSE_FIELDS:
        assert parts[f].tobytes() == s["parts"][f].tobytes(), (k, f)
    assert np.array_equal(cum, s["cum"]) and np.array_equal(units, s["units"]), k
    if r_m["moved"]:
        idx, like = rb.debugLast()
        assert np.array_equal(idx, s["idx"]) and np.array_equal(like, s["like"]), k
        assert parts["weight"].tobytes() == s["parts"]["weight"].tobytes(), k
    if s["matched"]:
        got = rb.debugMatch()
        for f in rmm.MATCH_FIELDS:
            assert np.array_equal(got[f], s["match"][f]), (k, f)
    assert (r_g["S"], r_g["Q"], r_g["best"]) == (r_m["S"], r_m["Q"], r_m["best"]), k
    gp = r_g["pose"]
    assert (np.float32(gp.x), np.float32(gp.y), np.float32(gp.theta), gp.utime) == \
           (np.float32(r_m["pose"][0]), np.float32(r_m["pose"][1]), np.float32(r_m["pose"][2]), r_m["pose"][3]), k
    for p in (range(len(s["maps"])) if maps_of is None else maps_of):
        assert rb.mapCells(p).tobytes() == s["maps"][p].tobytes(), (k, p)


def _replay(gpu_ctx, c, snaps, force=None, maps_of=None):
    """The device over the case's inputs, compared with the snapshots after every update.  force: the setScanMatching keywords for
    every update in place of the case's own."""
    rb = _device(gpu_ctx, c, snaps[0]["before"])
    current, paths = "unset", []
    for k, o in enumerate(c["odoms"]):
        kw = c["match"][k] if force is None else force
        if kw is not current:
            rb.setScanMatching(**kw) if kw is not None else rb.setScanMatching(None)
            current = kw
        s = snaps[k]
        r_g = rb.update(bl.make_pose(o[0], o[1], o[2], utime=o[3]), c["scans"][k], rand_value=s["rand_value"], noise=s["noise"])
        last = k == len(snaps) - 1
        _compare(rb, s, r_g, k, maps_of=None if (maps_of is None or last) else maps_of)
        if s["matched"]:
            paths.append(rb.debugMatchPath())
    rb.close()
    return paths


@pytest.mark.parametrize("name", [n for n in CASES if n != "zero_window"])
def test_run_matches_the_model(oracle, maps, gpu_ctx, name):
    c, snaps = record(oracle, maps, name)
    paths = _replay(gpu_ctx, c, snaps, maps_of=[0, c["P"] - 1] if name == "p1000" else None)
    expect = [rmm.window_path(c["scans"][k], c["match"][k]["max_range"], c["cpm"], c["shape"][1], c["shape"][0], c["match"][k]["nx"], c["match"][k]["ny"])
              for k, s in enumerate(snaps) if s["matched"]]
    assert paths == expect
    if name == "main":
        assert paths and set(paths) == {0}
    if name == "direct":
        assert paths and set(paths) == {1}


def test_zero_window_equals_matching_off(oracle, maps, gpu_ctx):
    """The device with a 0, 0, 0 window against the model WITHOUT matching (rb_slam_model.RBSlamModel), and against the model with it."""
    c, plain = record(oracle, maps, "zero_window", plain=True)
    for s in plain:
        assert not s["matched"]
    zero = dict(nx=0, ny=0, ntheta=0, dtheta=DTH, max_range=8.0, min_score=0)
    _replay(gpu_ctx, c, plain, force=zero)
    _replay(gpu_ctx, *record(oracle, maps, "zero_window"))


def test_error_paths(oracle, maps, gpu_ctx):
    c, snaps = record(oracle, maps, "p1")
    rb = _device(gpu_ctx, c, snaps[0]["before"])
    with pytest.raises(bl.BotlabHipError):                      # nothing matched so far
        rb.debugMatch()
    assert rb.debugMatchPath() == -1
    good = dict(nx=2, ny=2, ntheta=3, dtheta=DTH, max_range=8.0, min_score=0)
    rb.setScanMatching(**good)
    for bad in [dict(nx=9), dict(ny=9), dict(ntheta=17), dict(nx=-1), dict(ny=-1), dict(ntheta=-1), dict(dtheta=0.0), dict(dtheta=float("nan"))]:
        with pytest.raises(bl.BotlabHipError):
            rb.setScanMatching(**dict(good, **bad))
    rb.setScanMatching(**dict(good, nx=8, ny=8, ntheta=16))     # the limits themselves are fine
    rb.setScanMatching(**good)
    with pytest.raises(bl.BotlabHipError):                      # still nothing matched
        rb.debugMatch()
    # 4097 valid rays: refused with the state unchanged -- the ActionModel has not latched the odometry -- so that the run that follows
    # equals the model's, which never saw the call
    n = 4097
    far = c["odoms"][-1]
    big = bl.LidarScan(np.full(n, 1.0, np.float32), np.linspace(0, 6.28, n).astype(np.float32), np.arange(n, dtype=np.int64), utime=far[3])
    with pytest.raises(bl.BotlabHipError):
        rb.update(bl.make_pose(far[0] + 1.0, far[1], far[2], utime=far[3]), big, rand_value=1)
    for k, o in enumerate(c["odoms"]):
        s = snaps[k]
        if k == 2:
            with pytest.raises(bl.BotlabHipError):
                rb.update(bl.make_pose(far[0] + 1.0, far[1], far[2], utime=far[3]), big, rand_value=1)
        r_g = rb.update(bl.make_pose(o[0], o[1], o[2], utime=o[3]), c["scans"][k], rand_value=s["rand_value"], noise=s["noise"])
        _compare(rb, s, r_g, k)
    # 4096 valid rays are taken
    ok = bl.LidarScan(big.ranges[:4096], big.thetas[:4096], big.times[:4096], utime=far[3] + 1000)
    rb.update(bl.make_pose(far[0] + 0.02, far[1], far[2], utime=far[3] + 1000), ok, rand_value=1)
    assert np.all(rb.debugMatch()["ties"] >= 1)
    rb.close()
