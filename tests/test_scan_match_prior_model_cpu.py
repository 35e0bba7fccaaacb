"""The model of the scan match with a prior (tests/scan_match_prior_model.py) against the definition spelled out in Python
integers, the cases of tests/scan_match_prior_cases.py against the conditions they are named for, and the host-side pieces
that need no device: the weight table, the two double helpers of include/botlab_hip.h, prior_from_sigmas."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

import botlab_amd as bl
import helpers
import scan_match_model as sm
import scan_match_prior_cases as pc
import scan_match_prior_model as smp
from botlab_amd import _capi, synth

CPM = helpers.CPM_DEFAULT
DTH = np.float32(math.radians(0.5))


def truth_of(cells):
    return np.where(cells > 0, 127, -127).astype(np.int8)


def test_weight_table_is_exact():
    """n = BL_SM_EXP2[i] iff n^64 2^i <= 2^1280 < (n + 1)^64 2^i, in Python integers; the header's literals, the model's table."""
    table = smp.header_table()
    assert len(table) == 64 and table == smp.EXP2
    for i, n in enumerate(table):
        assert n ** 64 * 2 ** i <= 2 ** 1280 < (n + 1) ** 64 * 2 ** i, i
    assert table[0] == 1 << 20 and table[63] > 1 << 19


def test_weights_follow_the_definition():
    for hl in (1, 2, 3, 777, 1000, (1 << 20) - 1, 1 << 20):
        for d in (0, 1, hl - 1, hl, hl + 1, 20 * hl + hl - 1, 21 * hl - 1, 21 * hl, (1 << 23) + (1 << 19) - 1):
            if d < 0 or d >= (1 << 23) + (1 << 19):
                continue
            e, f = divmod(d, hl)
            want = 0 if e >= 21 else smp.EXP2[(64 * f) // hl] >> e
            assert smp.weight(d, hl) == want
            assert int(smp.weights(np.array([-d], np.int32), 0, hl)[0]) == want
    assert smp.weight(0, 5) == 1 << 20 and smp.weight(5, 5) == 1 << 19 and smp.weight(105, 5) == 0 and smp.weight(104, 5) == smp.EXP2[51] >> 20


@pytest.mark.parametrize("name", helpers.SLAM_MAPS)
def test_zero_prior_is_the_plain_match(maps, name):
    m = maps[name]
    truth = truth_of(m["cells"])
    pose = (-0.75, 0.2, 0.4)
    scan = synth.raycast_scan(truth, m["origin"], 0.05, pose, pose, 123456)
    for centre, (nx, ny, nt), min_score in [((pose[0] + 0.12, pose[1] - 0.08, pose[2] + 0.03), (4, 4, 12), 0),
                                            ((pose[0] - 0.3, pose[1] + 0.2, pose[2] - 0.1), (10, 3, 20), 10 ** 6),
                                            ((40.0, -37.0, 2.0), (6, 6, 2), 0)]:
        a = sm.match(truth, m["origin"], m["mpc"], CPM, scan.ranges, scan.thetas, centre, nx, ny, nt, DTH, 8.0, min_score=min_score, utime=5)
        b = smp.match(truth, m["origin"], m["mpc"], CPM, scan.ranges, scan.thetas, centre, nx, ny, nt, DTH, 8.0, min_score=min_score,
                      utime=5, half_life=100)
        for k in a:
            if k == "volume":
                assert np.array_equal(a[k], b[k])
            else:
                assert a[k] == b[k] and type(a[k]) is type(b[k]), k
        assert b["best_obj"] == a["score"] and b["pen_best"] == 0


def test_moments_equal_a_brute_force_loop():
    """Every candidate in a plain triple loop, Python integers throughout; the covariance in Fractions."""
    case = pc.get("window_4_4_12")._replace(name="brute", window=(3, 2, 2), prop=None)
    for prior, hl in [((300, -200, 400, 50), 40), ((0, 0, 0, 0), 1), ((32767, 32767, 32767, 32767), 1 << 20)]:
        ref = pc.model(case, prior=prior, half_life=hl)
        nx, ny, nt = case.window
        score = ref["score_volume"]
        objs = {}
        for dk in range(-nt, nt + 1):
            for dj in range(-ny, ny + 1):
                for di in range(-nx, nx + 1):
                    q = prior[0] * di * di + 2 * prior[1] * di * dj + prior[2] * dj * dj + prior[3] * dk * dk
                    assert q >= 0
                    objs[(di, dj, dk)] = int(score[dk + nt, dj + ny, di + nx]) - (q >> 8)
        best = max(objs.values())
        order = min((di * di + dj * dj, abs(dk), dk, dj, di) for (di, dj, dk), o in objs.items() if o == best)
        assert (ref["di"], ref["dj"], ref["dk"]) == (order[4], order[3], order[2]) and ref["best_obj"] == best
        assert ref["ties"] == sum(1 for o in objs.values() if o == best)
        sums = [0] * 10
        for (di, dj, dk), o in objs.items():
            w = smp.weight(best - o, hl)
            for n, v in enumerate((1, di, dj, dk, di * di, di * dj, dj * dj, di * dk, dj * dk, dk * dk)):
                sums[n] += w * v
        assert tuple(sums) == ref["sums"]
        assert np.array_equal(ref["volume"], np.array([[[objs[(di, dj, dk)] for di in range(-nx, nx + 1)] for dj in range(-ny, ny + 1)]
                                                        for dk in range(-nt, nt + 1)], dtype=np.int32))
        # the fractions from the same dictionary
        for axis, step in enumerate(((1, 0, 0), (0, 1, 0), (0, 0, 1))):
            b = (ref["di"], ref["dj"], ref["dk"])
            lo, hi = tuple(x - s for x, s in zip(b, step)), tuple(x + s for x, s in zip(b, step))
            if lo in objs and hi in objs:
                den, num = 2 * (2 * best - objs[lo] - objs[hi]), objs[hi] - objs[lo]
                want = (num, den) if den else (0, 1)
            else:
                want = (0, 1)
            assert ref["fractions"][axis] == want


@pytest.mark.parametrize("name", sorted(pc.BUILDERS))
def test_every_case_reaches_what_it_is_named_for(name):
    """The builders' own assertions (from the model alone), and |num / den| <= 1/2 with den >= 1 on every case."""
    ref = pc.evaluate(pc.get(name))
    assert ref["raw_best"][3] == int(ref["score_volume"].max())


def test_corridor_prior_and_covariance():
    """Two parallel walls: without a prior the score is flat along the corridor (ties > 1); with a_xx > 0 the winner is unique and
    no further from the centre than any of the tying candidates; the covariance along the corridor exceeds that across it."""
    free, prior = pc.get("corridor_free"), pc.get("corridor_prior")
    rf, rp = pc.evaluate(free), pc.evaluate(prior)
    assert rf["ties"] > 1 and rp["ties"] == 1
    for case, ref in ((free, rf), (prior, rp)):
        _, cov = smp.covariance(ref["sums"], float(case.mpc), float(case.dtheta))
        print("%s: cov_xx = %.6f m^2, cov_yy = %.6f m^2, ratio %.2f" % (case.name, cov[0], cov[2], cov[0] / cov[2]))
        assert cov[0] > cov[2] > 0
    assert smp.covariance(rp["sums"], 0.05, 1.0)[1][0] < smp.covariance(rf["sums"], 0.05, 1.0)[1][0]      # the prior narrows it


def test_prior_moves_the_winner():
    ref = pc.evaluate(pc.get("prior_moves_winner"))
    assert (ref["di"], ref["dj"], ref["dk"]) != ref["raw_best"][:3] and ref["score"] < ref["raw_best"][3]


def test_fractions_on_edges_and_empty_axes():
    for name in sorted(pc.BUILDERS):
        case, ref = pc.get(name), pc.evaluate(pc.get(name))
        for axis in range(3):
            num, den = ref["fractions"][axis]
            assert den >= 1 and 2 * abs(num) <= den
            pos = (ref["di"], ref["dj"], ref["dk"])[axis]
            if case.window[axis] == 0 or abs(pos) == case.window[axis]:
                assert (num, den) == (0, 1), (name, axis)
    assert pc.evaluate(pc.get("nx_zero"))["fractions"][0] == (0, 1)
    edges = {(a, s) for a in range(3) for s in (-1, 1)}
    for a, s in edges:
        ref = pc.evaluate(pc.get("face_%s_%s" % ("xyt"[a], "plus" if s > 0 else "minus")))
        assert ref["fractions"][a] == (0, 1)


def test_prior_from_sigmas_rounding_and_clamping():
    mpc, dth = 0.0625, 0.015625                                        # powers of two: every product below is exact in double
    # sigma = 2 cells, 4 cells, 8 steps, one unit per nat: 128 / 4 = 32, 128 / 16 = 8, 128 / 64 = 2
    assert bl.prior_from_sigmas(2 * mpc, 4 * mpc, 0.0, 8 * dth, 1.0, mpc, dth) == (32, 0, 8, 2)
    # rounding to nearest, halves up: 128 * 3 / 256 = 1.5 -> 2;  128 * 1 / 256 = 0.5 -> 1;  128 * 0.99 / 256 -> 0
    assert bl.prior_from_sigmas(16 * mpc, 16 * mpc, 0.0, 16 * dth, 3.0, mpc, dth) == (2, 0, 2, 2)
    assert bl.prior_from_sigmas(16 * mpc, 16 * mpc, 0.0, 16 * dth, 1.0, mpc, dth) == (1, 0, 1, 1)
    assert bl.prior_from_sigmas(16 * mpc, 16 * mpc, 0.0, 16 * dth, 0.99, mpc, dth) == (0, 0, 0, 0)
    # correlation: q = 3/4; 128 / (3/4 * 4) = 42.67 -> 43; -0.5 * 128 / (3/4 * 4) = -21.33 -> -21
    assert bl.prior_from_sigmas(2 * mpc, 2 * mpc, 0.5, 8 * dth, 1.0, mpc, dth) == (43, -21, 43, 2)
    assert bl.prior_from_sigmas(2 * mpc, 2 * mpc, -0.5, 8 * dth, 1.0, mpc, dth) == (43, 21, 43, 2)
    # clamping: a tight sigma saturates at 32767; the cross term is then lowered to keep the form non-negative
    assert bl.prior_from_sigmas(mpc / 64, mpc / 64, 0.0, dth / 64, 1.0, mpc, dth) == (32767, 0, 32767, 32767)
    got = bl.prior_from_sigmas(mpc / 64, 2 * mpc, 0.75, dth, 1.0, mpc, dth)
    assert got[0] == 32767 and got[1] < 0 and got[1] * got[1] <= got[0] * got[2] < (abs(got[1]) + 1) ** 2 and smp.check_prior(*got)
    assert bl.prior_from_sigmas(float("inf"), 2 * mpc, 0.0, float("inf"), 1.0, mpc, dth) == (0, 0, 32, 0)
    for args in [(2 * mpc, 4 * mpc, 0.0, 8 * dth, 1.0), (3 * mpc, 5 * mpc, 0.25, 7 * dth, 2.0), (mpc, mpc, -0.875, dth, 100.0)]:
        got = bl.prior_from_sigmas(*args, mpc, dth)
        assert got == smp.prior_from_sigmas(*args, mpc, dth) and smp.check_prior(*got), (args, got)
    for bad in [(0.0, 1.0, 0.0, 1.0, 1.0), (1.0, -1.0, 0.0, 1.0, 1.0), (1.0, 1.0, 1.0, 1.0, 1.0), (1.0, 1.0, 0.0, 0.0, 1.0),
                (1.0, 1.0, float("nan"), 1.0, 1.0), (1.0, 1.0, 0.0, 1.0, -1.0)]:
        with pytest.raises(ValueError):
            bl.prior_from_sigmas(*bad, mpc, dth)


def test_refusals():
    """What bl_scanmatch_match_prior refuses, as the model states it (the library's own refusals are compared with this on the
    device, tests/test_gpu_scan_match_prior.py); and the one refusal that needs no device."""
    ok = dict(half_life=10, want_moments=True, moments_given=True)
    assert smp.check_prior(0, 0, 0, 0) and smp.check_prior(32767, 32767, 32767, 32767, **ok) and smp.check_prior(4, -2, 1, 0, **ok)
    assert not smp.check_prior(4, 3, 2, 0)                            # 9 > 8: not positive semi-definite
    assert not smp.check_prior(0, 1, 5, 0) and not smp.check_prior(0, -1, 0, 0)
    for bad in [(32768, 0, 0, 0), (0, 0, 32768, 0), (0, 0, 0, 32768), (-1, 0, 0, 0), (0, 0, -1, 0), (0, 0, 0, -1),
                (32767, 32768, 32767, 0), (32767, -32768, 32767, 0)]:
        assert not smp.check_prior(*bad), bad
    assert not smp.check_prior(1, 0, 1, 1, half_life=0, want_moments=True)
    assert not smp.check_prior(1, 0, 1, 1, half_life=(1 << 20) + 1, want_moments=True)
    assert not smp.check_prior(1, 0, 1, 1, half_life=None, want_moments=True)
    assert not smp.check_prior(1, 0, 1, 1, half_life=5, want_moments=True, moments_given=False)      # NULL moments pointer
    assert smp.check_prior(1, 0, 1, 1, half_life=0, want_moments=False, moments_given=False)          # half_life is not read
    lib = _capi.load()
    assert lib.bl_scanmatch_match_prior(None, None, None, None, None, None, None, None) == 2


def test_covariance_helper_against_the_exact_value():
    """bl_scanmatch_covariance (the header's function, as the library exports it) against Fractions.  The tolerance is derived, not
    tuned: an entry is a difference of two quotients times a scale -- s_ab / s0, (s_a / s0)(s_b / s0), each a handful of
    roundings of relative size 2^-53 (the int64 -> double conversions, two or three divisions, a product, the difference, the
    scale's product and the final product) -- so 8 * 2^-53 * (|E[ab]| + |E[a] E[b]|) * scale absolute covers them with margin.
    The mean is one quotient and one product: 4 * 2^-53 relative."""
    eps = 2.0 ** -53
    for name in ("window_4_4_12", "half_life_1", "half_life_1048576", "corridor_free", "flat_free", "window_1_1_180", "prior_moves_winner"):
        case, ref = pc.get(name), pc.evaluate(pc.get(name))
        mpc, dth = float(case.mpc), float(case.dtheta)
        mom = _capi.ScanMatchMoments(*ref["sums"])
        mean, cov = mom.covariance(mpc, dth)
        assert (tuple(mean), tuple(cov)) == smp.covariance(ref["sums"], mpc, dth)                     # the model's restatement, bit for bit
        emean, ecov = smp.covariance_exact(ref["sums"], mpc, dth)
        for got, exact in zip(mean, emean):
            assert abs(Fraction(got) - exact) <= Fraction(4 * eps) * abs(exact), (name, got, float(exact))
        for got, exact, (eab, eaeb, scale) in zip(cov, ecov, smp.covariance_terms(ref["sums"], mpc, dth)):
            tol = 8 * eps * (eab + eaeb) * scale
            assert abs(Fraction(got) - exact) <= Fraction(tol), (name, got, float(exact), tol)
        assert ecov[0] >= 0 and ecov[2] >= 0 and ecov[5] >= 0
    assert _capi.ScanMatchMoments().covariance(0.05, 0.01) == ((0.0,) * 3, (0.0,) * 6)               # a record never filled


def test_refined_pose_helper():
    for name in ("window_4_4_12", "width_203", "face_x_plus", "prior_moves_winner"):
        case, ref = pc.get(name), pc.evaluate(pc.get(name))
        res = _capi.ScanMatchResult()
        res.pose = bl.make_pose(float(ref["x"]), float(ref["y"]), float(ref["theta"]), utime=9)
        res.di, res.dj, res.dk, res.accepted = ref["di"], ref["dj"], ref["dk"], 1
        mom = _capi.ScanMatchMoments(*ref["sums"])
        for a in range(3):
            mom.sub_num[a], mom.sub_den[a] = ref["fractions"][a]
        centre = bl.make_pose(*(float(v) for v in case.centre))
        out = mom.refined_pose(res, centre, float(case.mpc), float(case.dtheta))
        want = smp.refined_pose(ref, case.centre, float(case.mpc), float(case.dtheta))
        assert np.array([out.x, out.y, out.theta], np.float32).tobytes() == np.array(want, np.float32).tobytes() and out.utime == 9
        # within half a cell / half a step of the whole-cell pose
        assert abs(float(out.x) - float(ref["x"])) <= 0.5 * float(case.mpc) + 1e-6
        assert abs(float(out.y) - float(ref["y"])) <= 0.5 * float(case.mpc) + 1e-6
        res.accepted = 0
        out = mom.refined_pose(res, centre, float(case.mpc), float(case.dtheta))
        assert (out.x, out.y, out.theta) == (res.pose.x, res.pose.y, res.pose.theta)
