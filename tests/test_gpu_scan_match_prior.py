"""bl_scanmatch_match_prior (botlab_amd/csrc/bl_scanmatch.hip) against the model (tests/scan_match_prior_model.py): the result
struct, the ten sums, best_obj, pen_best, the sub-cell fractions and the whole objective volume, byte for byte.  Everything
compared is an integer, so the allowed number of mismatches is 0.  The inputs are tests/scan_match_prior_cases.py's, each of
which asserts from the model alone that it reaches the condition it is named for."""
import ctypes as C

import numpy as np
import pytest

import botlab_amd as bl
import scan_match_model as sm
import scan_match_prior_cases as pc
import scan_match_prior_model as smp
from botlab_amd import _capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def matcher(gpu_ctx):
    m = bl.ScanMatcher(ctx=gpu_ctx)
    yield m
    m.close()


def grid_of(case, ctx):
    return bl.OccupancyGrid.from_cells(case.cells, case.origin, case.mpc, cellsPerMeter=case.cpm, ctx=ctx)


def scan_of(case):
    n = len(case.ranges)
    return bl.LidarScan(case.ranges, case.thetas, np.arange(n, dtype=np.int64), utime=pc.UTIME)


def window_kw(case):
    nx, ny, nt = case.window
    return dict(nx=nx, ny=ny, ntheta=nt, dtheta=case.dtheta, max_range=case.max_range, min_score=case.min_score)


def result_tuple(res):
    return (res.di, res.dj, res.dk, res.score, res.score_centre, res.ties, res.rays_used, res.accepted, res.pose.utime,
            np.array([res.pose.x, res.pose.y, res.pose.theta], np.float32).tobytes())


def model_tuple(ref):
    return (ref["di"], ref["dj"], ref["dk"], ref["score"], ref["score_centre"], ref["ties"], ref["rays_used"], ref["accepted"], ref["utime"],
            np.array([ref["x"], ref["y"], ref["theta"]], np.float32).tobytes())


def compare(matcher, grid, case, ref):
    """One match with the moments: every field, every sum, every objective against the model.  Then the same match without the
    moments (no volume kept): the same result struct.  Returns (result, moments)."""
    c = bl.make_pose(*(float(v) for v in case.centre), utime=7)
    res, mom = matcher.match_prior(scan_of(case), c, grid, prior=case.prior, half_life=case.half_life, **window_kw(case))
    vol = matcher.volume()
    mismatches = int((vol != ref["volume"]).sum())
    assert vol.shape == ref["volume"].shape and mismatches == 0, "%d of %d objectives differ" % (mismatches, vol.size)
    assert result_tuple(res) == model_tuple(ref), (res, {k: v for k, v in ref.items() if "volume" not in k})
    assert mom.sums() == ref["sums"], (mom.sums(), ref["sums"])
    assert (mom.best_obj, mom.pen_best) == (ref["best_obj"], ref["pen_best"])
    assert mom.fractions() == ref["fractions"], (mom.fractions(), ref["fractions"])
    assert res.score == mom.best_obj + mom.pen_best
    res2, none = matcher.match_prior(scan_of(case), c, grid, prior=case.prior, **window_kw(case))
    assert none is None and bytes(res2) == bytes(res)
    with pytest.raises(bl.BotlabHipError):
        matcher.volume()
    return res, mom


@pytest.mark.parametrize("name", sorted(pc.BUILDERS))
def test_case(gpu_ctx, matcher, name):
    case = pc.get(name)
    ref = pc.evaluate(case)
    g = grid_of(case, gpu_ctx)
    compare(matcher, g, case, ref)
    assert matcher.debugPath() == (1 if name == "direct_path" else 0)
    g.close()


def test_zero_prior_without_moments_is_the_plain_match(gpu_ctx, matcher):
    """All four coefficients 0, want_moments 0: the result struct of bl_scanmatch_match, byte for byte -- on both scoring paths, a
    grid of odd width, a rejected match and an empty map."""
    for name, min_score in [("window_4_4_12", 0), ("window_4_4_12", 10 ** 6), ("window_64_64_2", 0), ("width_203", 0), ("direct_path", 0),
                            ("corridor_free", 0), ("flat_empty", 1), ("face_t_minus", 0)]:
        case = pc.get(name)
        g = grid_of(case, gpu_ctx)
        c = bl.make_pose(*(float(v) for v in case.centre), utime=7)
        kw = dict(window_kw(case), min_score=min_score)
        plain = matcher.match(scan_of(case), c, g, **kw)
        path = matcher.debugPath()
        prior, none = matcher.match_prior(scan_of(case), c, g, **kw)
        assert none is None and bytes(prior) == bytes(plain), (name, prior, plain)
        assert matcher.debugPath() == path
        # and with the volume kept: the objective volume of a zero prior is the score volume
        matcher.match(scan_of(case), c, g, keep_volume=True, **kw)
        a = matcher.volume()
        kept, mom = matcher.match_prior(scan_of(case), c, g, half_life=50, **kw)
        assert bytes(kept) == bytes(plain) and np.array_equal(matcher.volume(), a) and mom.pen_best == 0 and mom.best_obj == plain.score
        g.close()


def test_call_order_and_the_kept_volume(gpu_ctx):
    """A plain match after a match with a prior and the reverse, windows of different sizes on one matcher: the buffers are shared,
    and bl_scanmatch_volume follows the last call."""
    big, small = pc.get("window_4_4_12"), pc.get("prior_moves_winner")
    rb, rs = pc.evaluate(big), pc.evaluate(small)
    gb, gs = grid_of(big, gpu_ctx), grid_of(small, gpu_ctx)
    m = bl.ScanMatcher(ctx=gpu_ctx)
    cb = bl.make_pose(*(float(v) for v in big.centre), utime=7)
    cs = bl.make_pose(*(float(v) for v in small.centre), utime=7)
    plain_ref = sm.match(small.cells, small.origin, small.mpc, small.cpm, small.ranges, small.thetas, small.centre, *small.window,
                         small.dtheta, small.max_range, utime=pc.UTIME)
    for _ in range(2):
        compare(m, gb, big, rb)                                                  # prior, moments (ends with a match that keeps nothing)
        res = m.match(scan_of(small), cs, gs, keep_volume=True, **window_kw(small))            # plain after prior: the SCORE volume
        assert np.array_equal(m.volume(), plain_ref["volume"]) and (res.di, res.dj, res.dk, res.score) == (3, 0, 0, 100)
        res, mom = m.match_prior(scan_of(small), cs, gs, prior=small.prior, half_life=small.half_life, **window_kw(small))
        assert np.array_equal(m.volume(), rs["volume"]) and mom.sums() == rs["sums"] and result_tuple(res) == model_tuple(rs)
        res = m.match(scan_of(big), cb, gb, **window_kw(big))                                  # plain, nothing kept
        with pytest.raises(bl.BotlabHipError):
            m.volume()
        res, _ = m.match_prior(scan_of(big), cb, gb, prior=big.prior, keep_volume=True, **window_kw(big))   # kept without moments
        assert np.array_equal(m.volume(), rb["volume"]) and result_tuple(res) == model_tuple(rb)
    m.close(); gb.close(); gs.close()


def test_refusals_change_nothing(gpu_ctx):
    """Every refusal the model states (smp.check_prior) is BL_ERR_ARG, and a kept volume outlives it."""
    case = pc.get("window_4_4_12")
    ref = pc.evaluate(case)
    g = grid_of(case, gpu_ctx)
    m = bl.ScanMatcher(ctx=gpu_ctx)
    c = bl.make_pose(*(float(v) for v in case.centre), utime=7)
    scan = scan_of(case)
    kw = window_kw(case)
    m.match_prior(scan, c, g, prior=case.prior, half_life=case.half_life, **kw)

    def status(fn):
        with pytest.raises(bl.BotlabHipError) as e:
            fn()
        return int(str(e.value).split("status ")[1].split(")")[0])

    bad_priors = [(4, 3, 2, 0), (0, 1, 5, 0), (32768, 0, 0, 0), (0, 0, 32768, 0), (0, 0, 0, 32768), (-1, 0, 0, 0), (0, 0, -1, 0),
                  (0, 0, 0, -1), (32767, 32768, 32767, 0), (32767, -32768, 32767, 0)]
    for p in bad_priors:
        assert not smp.check_prior(*p)
        assert status(lambda: m.match_prior(scan, c, g, prior=p, **kw)) == 2, p
        assert status(lambda: m.match_prior(scan, c, g, prior=p, half_life=5, **kw)) == 2, p
    for hl in (0, -1, (1 << 20) + 1):
        assert status(lambda: m.match_prior(scan, c, g, prior=case.prior, half_life=hl, **kw)) == 2, hl
    assert status(lambda: m.match_prior(scan, c, g, prior=case.prior, half_life=5, **dict(kw, nx=65))) == 2
    assert status(lambda: m.match_prior(scan, c, g, prior=case.prior, half_life=5, **dict(kw, dtheta=0.0))) == 2
    # want_moments with a NULL moments pointer, and a NULL prior, straight at the C ABI
    lib = gpu_ctx.lib
    ls, p, r = scan.as_c(), _capi.ScanMatchParams(4, 4, 12, float(case.dtheta), case.max_range, 0, 0), _capi.ScanMatchResult()
    pr = _capi.ScanMatchPrior(*case.prior, 5, 1)
    assert lib.bl_scanmatch_match_prior(m.h, g.h, C.byref(ls), C.byref(c), C.byref(p), C.byref(pr), C.byref(r), None) == 2
    assert lib.bl_scanmatch_match_prior(m.h, g.h, C.byref(ls), C.byref(c), C.byref(p), None, C.byref(r), None) == 2
    assert lib.bl_scanmatch_match_prior(m.h, g.h, C.byref(ls), C.byref(c), C.byref(p), C.byref(pr), None, None) == 2
    # half_life is not read without want_moments, and the moments pointer may be NULL
    pr0 = _capi.ScanMatchPrior(*case.prior, 0, 0)
    vol = m.volume()                                                             # still the first call's: nothing above changed it
    assert np.array_equal(vol, ref["volume"])
    out = np.zeros(vol.size, np.int32)
    assert lib.bl_scanmatch_volume(m.h, out.ctypes.data_as(C.c_void_p)) == 0 and np.array_equal(out.reshape(vol.shape), vol)
    assert lib.bl_scanmatch_match_prior(m.h, g.h, C.byref(ls), C.byref(c), C.byref(p), C.byref(pr0), C.byref(r), None) == 0
    assert (r.di, r.dj, r.dk, r.score) == (ref["di"], ref["dj"], ref["dk"], ref["score"])
    assert lib.bl_scanmatch_volume(m.h, out.ctypes.data_as(C.c_void_p)) == 4       # an accepted call that kept nothing
    m.close(); g.close()
