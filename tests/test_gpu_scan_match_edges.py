"""bl_scanmatch_match and bl_scanmatch_match_wide (botlab_amd/csrc/bl_scanmatch.hip) on the hand-built inputs of
tests/scan_match_cases.py: ties at a positive score decided by every level of the order and counted across slices, waves, workgroups,
kept blocks and headings; winners at the limits of the key fields; ray counts at the wave edges and the largest score; headings
across +-pi and rays the 2^30 guard takes out; other resolutions and origins; the largest LDS requests.  Each case proves on the
CPU that it reaches what it is named for (scan_match_cases.evaluate) before the device is asked.  One matcher serves every case, so
its buffers grow and are reused across very different sizes.  The definition is exact: 0 mismatching scores, every field of the
result equal, the pose as float32 bytes, and no case left out."""
import numpy as np
import pytest

import botlab_amd as bl
import scan_match_cases as smc
import scan_match_model as sm
import scan_match_prior_model as smp
import scan_match_wide_model as smw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def matcher(gpu_ctx):
    m = bl.ScanMatcher(ctx=gpu_ctx)
    yield m
    m.close()


def as_dict(res):
    return dict(x=np.float32(res.pose.x), y=np.float32(res.pose.y), theta=np.float32(res.pose.theta), utime=res.pose.utime, di=res.di,
                dj=res.dj, dk=res.dk, score=res.score, score_centre=res.score_centre, ties=res.ties, rays_used=res.rays_used,
                accepted=res.accepted)


def assert_same(res, ref, what):
    got = as_dict(res)
    assert smw.same_result(got, ref), (what, {f: (got[f], ref[f]) for f in smw.RESULT_FIELDS if str(got[f]) != str(ref[f])})


def seed_candidates(case, ev, h):
    """Exact scores k_smw_seed computes when every bound is the same positive number: block (0, 0) of every heading, clipped to
    the window, and the centre."""
    nx, ny, nt = case.window
    B = 1 << h
    return (2 * nt + 1) * min(B, 2 * nx + 1) * min(B, 2 * ny + 1) + 1


@pytest.mark.parametrize("name", list(smc.BUILDERS))
def test_case_on_the_device(gpu_ctx, matcher, name):
    case = smc.get(name)
    ev = smc.evaluate(case)
    ref = ev["ref"]
    nx, ny, nt = case.window
    grid = bl.OccupancyGrid.from_cells(case.cells, case.origin, case.mpc, cellsPerMeter=case.cpm, ctx=gpu_ctx)
    scan = bl.LidarScan(case.ranges, case.thetas, np.zeros(len(case.ranges), np.int64), utime=smc.UTIME)
    c = bl.make_pose(*[float(v) for v in case.centre], utime=7)
    assert np.array([c.x, c.y, c.theta], np.float32).tobytes() == np.array(case.centre, np.float32).tobytes()
    window = dict(nx=nx, ny=ny, ntheta=nt, dtheta=case.dtheta, max_range=case.max_range, min_score=case.min_score)

    narrow = None
    if smc.is_narrow(case):
        res = matcher.match(scan, c, grid, keep_volume=True, **window)
        vol = matcher.volume()
        mismatches = int((vol != ev["volume"]).sum())
        print(name, "narrow:", as_dict(res), "mismatching scores", mismatches, "path", matcher.debugPath())
        assert vol.shape == ev["volume"].shape and mismatches == 0, "%d of %d scores differ" % (mismatches, vol.size)
        assert_same(res, ref, (name, "narrow"))
        if "narrow_path" in case.expect:
            assert matcher.debugPath() == case.expect["narrow_path"]
        narrow = bytes(res)
        assert bytes(matcher.match(scan, c, grid, **window)) == narrow            # the same match without the volume

    auto = smc.auto_block_log2(case.window)
    candidates = (2 * nt + 1) * (2 * ny + 1) * (2 * nx + 1)
    for block_log2 in case.hs:
        res = matcher.match_wide(scan, c, grid, block_log2=block_log2, **window)
        st = matcher.wide_stats()
        h = block_log2 or auto
        print(name, "block_log2", block_log2, as_dict(res), st)
        assert_same(res, ref, (name, block_log2))
        if narrow is not None:
            assert bytes(res) == narrow, (name, block_log2)
        nbx, nby = smw.block_counts(nx, ny, h)
        assert (st.block_log2, st.candidates, st.blocks) == (h, candidates, (2 * nt + 1) * nbx * nby)
        if "wide_path" in case.expect:
            assert st.path == case.expect["wide_path"]
        if h in ev["pruned"]:
            pr = ev["pruned"][h]
            assert st.blocks == pr["blocks"] and st.blocks_kept == pr["kept"] and st.blocks_kept >= pr["kept_min"], (name, h, st, pr)
            if case.expect.get("all_kept"):
                assert st.blocks_kept == st.blocks == pr["kept_min"]
                assert st.candidates_scored == st.candidates + seed_candidates(case, ev, h)      # the statistic counts the seeds too
    if "auto_h" in case.expect:
        assert 0 in case.hs and auto == case.expect["auto_h"]
    if case.exhaustive:
        res = matcher.match_wide(scan, c, grid, exhaustive=True, **window)
        st = matcher.wide_stats()
        print(name, "exhaustive", as_dict(res), st)
        assert_same(res, ref, (name, "exhaustive"))
        if narrow is not None:
            assert bytes(res) == narrow, (name, "exhaustive")
        assert st.candidates_scored == st.candidates == candidates and st.blocks_kept == st.blocks
        if "wide_path" in case.expect:
            assert st.path == case.expect["wide_path"]
    grid.close()


def test_one_handle_across_the_three_matches(gpu_ctx):
    """The plain, the prior and the wide match share a handle's header and ray buffers.  One handle, on a 20 x 19 grid (rows copied
    as dwords) and again on a 21 x 19 one (as bytes): 1 valid ray plain; 300 wide (the buffers grow); 65 with a prior and the
    moments; 0 plain; 64 wide exhaustive; 300 plain with the volume kept.  Every result, the kept volume and the moments equal the
    model's, and every result is the one a fresh handle gives.  Each scan also has a ray at the 0.15 limit and one at max_range."""
    rng = np.random.default_rng(20260227)
    max_range, prior, half_life, dtheta = 0.55, (300, -40, 200, 90), 37, np.float32(np.radians(1.0))
    centre = (0.52, 0.47, 0.3)
    c = bl.make_pose(*centre, utime=7)

    def scan_of(n):
        r = np.concatenate([rng.uniform(0.16, 0.54, n), [0.15, max_range]]).astype(np.float32)
        t = rng.uniform(-np.pi, np.pi, n + 2).astype(np.float32)
        order = rng.permutation(n + 2)
        return r[order], t[order]

    # call, valid rays, window, what the call is given beyond the window
    calls = [("plain", 1, (3, 3, 2), {}), ("wide", 300, (3, 2, 2), {}), ("prior", 65, (2, 3, 2), dict(prior=prior, half_life=half_life)),
             ("plain", 0, (3, 3, 1), {}), ("wide", 64, (3, 3, 2), dict(exhaustive=True)), ("plain", 300, (3, 3, 2), dict(keep_volume=True))]

    def run(m, grid, kind, scan, window, extra):
        kw = dict(nx=window[0], ny=window[1], ntheta=window[2], dtheta=dtheta, max_range=max_range, min_score=1, **extra)
        if kind == "plain":
            return m.match(scan, c, grid, **kw), None
        if kind == "wide":
            return m.match_wide(scan, c, grid, **kw), None
        return m.match_prior(scan, c, grid, **kw)

    one = bl.ScanMatcher(ctx=gpu_ctx)
    for width in (20, 21):
        cells = rng.integers(-128, 128, (19, width)).astype(np.int8)
        grid = bl.OccupancyGrid.from_cells(cells, (0.0, 0.0), smc.MPC, cellsPerMeter=smc.CPM, ctx=gpu_ctx)
        for kind, n, window, extra in calls:
            ranges, thetas = scan_of(n)
            scan = bl.LidarScan(ranges, thetas, np.zeros(len(ranges), np.int64), utime=smc.UTIME)
            model = (ranges, thetas, centre, *window, dtheta, max_range)
            if kind == "prior":
                ref = smp.match(cells, (0.0, 0.0), smc.MPC, smc.CPM, *model, prior=prior, half_life=half_life, min_score=1, utime=smc.UTIME)
            else:
                ref = sm.match(cells, (0.0, 0.0), smc.MPC, smc.CPM, *model, min_score=1, utime=smc.UTIME)
            assert ref["rays_used"] == n
            res, mom = run(one, grid, kind, scan, window, extra)
            assert_same(res, ref, (width, kind, n))
            if kind == "prior":
                assert (mom.sums(), mom.best_obj, mom.pen_best, mom.fractions()) == (ref["sums"], ref["best_obj"], ref["pen_best"], ref["fractions"])
            if kind == "prior" or extra.get("keep_volume"):
                assert np.array_equal(one.volume(), ref["volume"]), (width, kind, n)
            fresh = bl.ScanMatcher(ctx=gpu_ctx)
            again, mom2 = run(fresh, grid, kind, scan, window, extra)
            assert bytes(again) == bytes(res), (width, kind, n)
            if kind == "prior":
                assert (mom2.sums(), mom2.best_obj, mom2.pen_best, mom2.fractions()) == (mom.sums(), mom.best_obj, mom.pen_best, mom.fractions())
            fresh.close()
        grid.close()
    one.close()


def test_over_budget_block_sizes_are_refused(gpu_ctx, matcher):
    """d_over_budget with the block sizes its budget excludes, and its exhaustive form: argument errors, not launches."""
    case = smc.get("d_over_budget")
    nx, ny, nt = case.window
    grid = bl.OccupancyGrid.from_cells(case.cells, case.origin, case.mpc, cellsPerMeter=case.cpm, ctx=gpu_ctx)
    scan = bl.LidarScan(case.ranges, case.thetas, np.zeros(len(case.ranges), np.int64), utime=smc.UTIME)
    c = bl.make_pose(*[float(v) for v in case.centre], utime=7)
    window = dict(nx=nx, ny=ny, ntheta=nt, dtheta=case.dtheta, max_range=case.max_range)
    for bad in (dict(block_log2=1), dict(block_log2=2), dict(block_log2=3), dict(exhaustive=True)):
        with pytest.raises(bl.BotlabHipError, match="status 2"):
            matcher.match_wide(scan, c, grid, **dict(window, **bad))
    grid.close()
