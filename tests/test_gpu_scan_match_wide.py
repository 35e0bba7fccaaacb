"""bl_scanmatch_match_wide (botlab_amd/csrc/bl_scanmatch.hip) against the wide model (tests/scan_match_wide_model.py) and against
bl_scanmatch_match: every field of the result bit for bit, and the statistics that show the pruning happened."""
import ctypes as C
import math

import numpy as np
import pytest

import botlab_amd as bl
import helpers
import scan_match_model as sm
import scan_match_wide_model as smw
from botlab_amd import _capi, synth

pytestmark = pytest.mark.gpu
CPM = helpers.CPM_DEFAULT
DTH = np.float32(math.radians(0.5))
DEG1, DEG2 = np.float32(math.radians(1.0)), np.float32(math.radians(2.0))


def truth_of(cells):
    return np.where(cells > 0, 127, -127).astype(np.int8)


def as_dict(res):
    return dict(x=np.float32(res.pose.x), y=np.float32(res.pose.y), theta=np.float32(res.pose.theta), utime=res.pose.utime, di=res.di,
                dj=res.dj, dk=res.dk, score=res.score, score_centre=res.score_centre, ties=res.ties, rays_used=res.rays_used,
                accepted=res.accepted)


def assert_same(res, ref, what=""):
    got = as_dict(res)
    assert smw.same_result(got, ref), (what, {f: (got[f], ref[f]) for f in smw.RESULT_FIELDS if str(got[f]) != str(ref[f])})


def wide(matcher, grid, scan, centre, nx, ny, nt, dtheta, max_range=8.0, min_score=0, block_log2=0, exhaustive=False):
    c = bl.make_pose(*centre, utime=7)
    res = matcher.match_wide(scan, c, grid, nx=nx, ny=ny, ntheta=nt, dtheta=dtheta, max_range=max_range, min_score=min_score,
                             block_log2=block_log2, exhaustive=exhaustive)
    return res, matcher.wide_stats(), (c.x, c.y, c.theta)


@pytest.fixture(scope="module")
def matcher(gpu_ctx):
    m = bl.ScanMatcher(ctx=gpu_ctx)
    yield m
    m.close()


@pytest.mark.parametrize("name", helpers.SLAM_MAPS)
def test_whole_map_windows(gpu_ctx, matcher, maps, name):
    """The whole 10 m map and the whole circle, no prior: centre = the map's middle, heading 0."""
    m = maps[name]
    truth = truth_of(m["cells"])
    g = bl.OccupancyGrid.from_cells(truth, m["origin"], m["mpc"], cellsPerMeter=CPM, ctx=gpu_ctx)
    mid = (float(m["origin"][0]) + 5.0, float(m["origin"][1]) + 5.0)
    pose = (mid[0] - 0.75, mid[1] + 0.2, math.radians(6.0))
    scan = synth.raycast_scan(truth, m["origin"], 0.05, pose, pose, 1000)
    centre = (mid[0], mid[1], 0.0)
    ref = None
    for block_log2 in (0, 4):
        res, st, c = wide(matcher, g, scan, centre, 100, 100, 90, DEG2, block_log2=block_log2)
        if ref is None:
            ref = smw.match_exhaustive(truth, m["origin"], m["mpc"], CPM, scan.ranges, scan.thetas, c, 100, 100, 90, DEG2, 8.0,
                                       utime=scan.utime)
        assert_same(res, ref, (name, block_log2))
        pr = smw.match_pruned(truth, m["origin"], m["mpc"], CPM, scan.ranges, scan.thetas, c, 100, 100, 90, DEG2, 8.0, st.block_log2,
                              utime=scan.utime)
        assert smw.same_result(pr, ref)
        print(name, st, "model: must score", pr["kept_min"], "blocks; the model's own threshold keeps", pr["kept"])
        assert st.block_log2 == (block_log2 or 3) and st.candidates == 201 * 201 * 181 == pr["candidates"] and st.blocks == pr["blocks"]
        assert st.path == 0                                       # a 200 x 200 map fits in LDS
        assert st.blocks_kept >= pr["kept_min"]                   # a correct pruner cannot keep fewer
        assert st.blocks_kept == pr["kept"]                       # the model takes its threshold from the same seeds
        assert st.candidates_scored * 10 <= st.candidates
    assert ref["ties"] == 1 and ref["accepted"] == 1
    if name != "convex_10mx10m_5cm_offcenter":
        assert (ref["di"], ref["dj"], ref["dk"]) == (-15, 4, 3)
    # the map as a SLAM run leaves it (mixed log-odds), the whole circle in steps of a degree
    g2 = bl.OccupancyGrid.from_cells(m["cells"], m["origin"], m["mpc"], cellsPerMeter=CPM, ctx=gpu_ctx)
    res, st, c = wide(matcher, g2, scan, centre, 100, 100, 180, DEG1, max_range=9.0)
    ref2 = smw.match_pruned(m["cells"], m["origin"], m["mpc"], CPM, scan.ranges, scan.thetas, c, 100, 100, 180, DEG1, 9.0, 3,
                            utime=scan.utime)
    assert_same(res, ref2, name)
    assert st.blocks_kept >= ref2["kept_min"] and st.candidates_scored * 10 <= st.candidates
    g.close(); g2.close()


SMALL_CASES = [((0.0, 0.0, 0.0), (4, 4, 12)), ((-0.3, 0.2, -0.1), (10, 3, 20)), ((0.1, 0.1, 0.0), (7, 9, 0)), ((0.0, 0.0, 0.0), (0, 0, 5)),
               ((0.5, -0.4, 0.2), (20, 20, 30)), ((1.0, -0.7, 0.5), (64, 64, 180))]


@pytest.mark.parametrize("name", ["obstacle_slam_10mx10m_5cm", "drive_square_10mx10m_5cm"])
def test_windows_within_the_old_limits(gpu_ctx, matcher, maps, name):
    """match_wide == the model == bl_scanmatch_match."""
    m = maps[name]
    g = bl.OccupancyGrid.from_cells(m["cells"], m["origin"], m["mpc"], cellsPerMeter=CPM, ctx=gpu_ctx)
    pose = (-0.75, 0.2, 0.4)
    scan = synth.raycast_scan(truth_of(m["cells"]), m["origin"], 0.05, pose, pose, 123456)
    for off, (nx, ny, nt) in SMALL_CASES:
        centre = (pose[0] + off[0], pose[1] + off[1], pose[2] + off[2])
        res, st, c = wide(matcher, g, scan, centre, nx, ny, nt, DTH)
        old = matcher.match(scan, bl.make_pose(*centre, utime=7), g, nx=nx, ny=ny, ntheta=nt, dtheta=DTH, max_range=8.0)
        assert bytes(res) == bytes(old), (off, res, old)
        ref = sm.match(m["cells"], m["origin"], m["mpc"], CPM, scan.ranges, scan.thetas, c, nx, ny, nt, DTH, 8.0, utime=scan.utime)
        assert_same(res, ref, off)
        ex, _, _ = wide(matcher, g, scan, centre, nx, ny, nt, DTH, exhaustive=True)
        assert bytes(ex) == bytes(res)
    g.close()


def test_exhaustive_equals_pruned_on_a_tiled_world(gpu_ctx, matcher, maps):
    """2000 x 2000 cells, +-1000 x +-1000 x +-20 steps of a degree: 1.6e8 candidates, beyond numpy's exhaustive volume.  The
    device's exhaustive form, its pruned form and the pruned model (tied to the exhaustive model on the CPU) agree."""
    world = synth.tile_world(maps["obstacle_slam_10mx10m_5cm"]["cells"], 2000)
    origin, mpc = (-50.0, -50.0), np.float32(0.05)
    g = bl.OccupancyGrid.from_cells(world, origin, mpc, cellsPerMeter=CPM, ctx=gpu_ctx)
    pose = (3.3, -7.1, 0.9)
    scan = synth.raycast_scan(world, origin, 0.05, pose, pose, 11)
    centre = (0.0, 0.0, 0.8)
    pruned, st, c = wide(matcher, g, scan, centre, 1000, 1000, 20, DEG1)
    assert st.path == 1 and st.block_log2 == 3 and st.candidates == 2001 * 2001 * 41
    full, st_full, _ = wide(matcher, g, scan, centre, 1000, 1000, 20, DEG1, exhaustive=True)
    assert bytes(full) == bytes(pruned), (full, pruned)
    assert st_full.candidates_scored == st_full.candidates and st_full.blocks_kept == st_full.blocks
    ref = smw.match_pruned(world, origin, mpc, CPM, scan.ranges, scan.thetas, c, 1000, 1000, 20, DEG1, 8.0, 3, utime=scan.utime)
    assert_same(pruned, ref)
    print(st, "model: must score", ref["kept_min"], "keeps", ref["kept"], "ties", ref["ties"])
    assert st.blocks_kept >= ref["kept_min"] and st.blocks_kept == ref["kept"] and st.candidates_scored * 10 <= st.candidates
    g.close()


@pytest.mark.parametrize("w,h", [(199, 200), (187, 150), (202, 93), (65, 70), (1, 1), (3, 257)])
def test_grid_widths_and_block_sizes(gpu_ctx, matcher, maps, w, h):
    m = maps["convex_10mx10m_5cm"]
    full = truth_of(m["cells"])
    cells = np.ascontiguousarray(full[:h, :w]) if h <= 200 else np.ascontiguousarray(np.tile(full, (2, 1))[:h, :w])
    g = bl.OccupancyGrid.from_cells(cells, m["origin"], m["mpc"], cellsPerMeter=CPM, ctx=gpu_ctx)
    pose = (-3.0, -2.6, -0.7)
    scan = synth.raycast_scan(cells, m["origin"], 0.05, pose, pose, 5)
    for centre, (nx, ny, nt) in [((pose[0] + 0.1, pose[1] - 0.05, pose[2] + 0.02), (9, 6, 7)), ((-4.9, -4.9, 0.3), (30, 17, 3)),
                                 ((0.0, 0.0, 0.0), (110, 140, 2))]:
        ref = None
        for block_log2 in (0, 1, 2, 3, 4, 5, 6):
            res, st, c = wide(matcher, g, scan, centre, nx, ny, nt, DTH, max_range=9.0, block_log2=block_log2)
            if ref is None:
                ref = smw.match_exhaustive(cells, m["origin"], m["mpc"], CPM, scan.ranges, scan.thetas, c, nx, ny, nt, DTH, 9.0,
                                           utime=scan.utime)
            assert_same(res, ref, (centre, block_log2))
            assert st.block_log2 == (block_log2 or 3)
            B = 1 << st.block_log2
            assert st.blocks == (2 * nt + 1) * ((2 * nx + B) // B) * ((2 * ny + B) // B)
    g.close()


def test_all_free_min_score_and_bad_rays(gpu_ctx, matcher, maps):
    m = maps["drive_square_10mx10m_5cm"]
    truth = truth_of(m["cells"])
    g = bl.OccupancyGrid.from_cells(truth, m["origin"], m["mpc"], cellsPerMeter=CPM, ctx=gpu_ctx)
    pose = (-0.75, 0.2, 0.0)
    scan = synth.raycast_scan(truth, m["origin"], 0.05, pose, pose, 1)
    centre = (pose[0] + 0.4, pose[1] - 0.3, pose[2] + 0.05)
    args = (truth, m["origin"], m["mpc"], CPM)
    res, st, c = wide(matcher, g, scan, centre, 30, 30, 12, DTH)
    ref = smw.match_exhaustive(*args, scan.ranges, scan.thetas, c, 30, 30, 12, DTH, 8.0, utime=scan.utime)
    assert_same(res, ref)
    assert res.accepted == 1 and res.score > 0
    for min_score, accepted in [(res.score + 1, 0), (res.score, 1)]:
        rej, _, _ = wide(matcher, g, scan, centre, 30, 30, 12, DTH, min_score=min_score)
        assert_same(rej, smw.match_exhaustive(*args, scan.ranges, scan.thetas, c, 30, 30, 12, DTH, 8.0, min_score=min_score, utime=scan.utime))
        assert rej.accepted == accepted
    # invalid and max-range rays
    r = scan.ranges.copy()
    r[::7] = 0.1; r[3::11] = 0.15; r[5::13] = 0.0; r[1::17] = -1.0; r[2::19] = 8.0; r[4::23] = np.inf; r[6::29] = np.nan
    r[8::31] = np.float32(0.15000001)
    bad = bl.LidarScan(r, scan.thetas, scan.times, utime=77)
    res, _, c = wide(matcher, g, bad, centre, 30, 30, 12, DTH)
    assert_same(res, smw.match_exhaustive(*args, bad.ranges, bad.thetas, c, 30, 30, 12, DTH, 8.0, utime=77))
    assert 0 < res.rays_used < 290
    # max-range returns counted as hits, the window pushing endpoints off every edge
    res, _, c = wide(matcher, g, scan, (0.3, -0.2, 1.0), 90, 90, 2, DTH, max_range=9.0)
    assert_same(res, smw.match_exhaustive(*args, scan.ranges, scan.thetas, c, 90, 90, 2, DTH, 9.0, utime=scan.utime))
    # no valid ray at all, an empty scan, a centre far from the grid: every score is 0, nothing is scored
    none = bl.LidarScan(np.full(290, 9.0, np.float32), scan.thetas, scan.times, utime=78)
    empty = bl.LidarScan(np.zeros(0, np.float32), np.zeros(0, np.float32), np.zeros(0, np.int64), utime=79)
    for s, ctr in [(none, pose), (empty, pose), (scan, (40.0, -37.0, 2.0))]:
        for exhaustive in (False, True):
            res, st, c = wide(matcher, g, s, ctr, 12, 13, 4, DTH, exhaustive=exhaustive)
            assert (res.score, res.ties, res.di, res.dj, res.dk, res.accepted) == (0, 25 * 27 * 9, 0, 0, 0, 1)
            assert (res.pose.x, res.pose.y, res.pose.theta, res.pose.utime) == (c[0], c[1], c[2], s.utime)
            assert st.candidates_scored == (25 * 27 * 9 if exhaustive else 0)
    g.close()


def test_all_free_map_and_saturating_ties(gpu_ctx, matcher, maps):
    m = maps["obstacle_slam_10mx10m_5cm"]
    free = np.full((200, 200), -127, np.int8)
    e = bl.OccupancyGrid.from_cells(free, m["origin"], m["mpc"], cellsPerMeter=CPM, ctx=gpu_ctx)
    pose = (-0.75, 0.2, 0.0)
    scan = synth.raycast_scan(truth_of(m["cells"]), m["origin"], 0.05, pose, pose, 1)
    # small enough to count
    for exhaustive in (False, True):
        res, st, c = wide(matcher, e, scan, pose, 100, 100, 45, DEG2, min_score=1, exhaustive=exhaustive)
        assert (res.score, res.score_centre, res.accepted, res.di, res.dj, res.dk, res.ties) == (0, 0, 0, 0, 0, 0, 201 * 201 * 91)
        assert (res.pose.x, res.pose.y, res.pose.theta) == c
    assert smw.saturate(201 * 201 * 91) == 201 * 201 * 91
    # 2001 * 2001 * 1441 = 5.8e9 candidates tie at 0: the count saturates
    n = 2001 * 2001 * 1441
    res, st, c = wide(matcher, e, scan, pose, 1000, 1000, 720, np.float32(math.radians(0.25)))
    assert n > 2 ** 31 - 1 and res.ties == smw.saturate(n) == 2 ** 31 - 1 and (res.score, res.di, res.dj, res.dk) == (0, 0, 0, 0)
    assert st.candidates == n and st.candidates_scored == 0 and st.blocks_kept == 0
    assert st.block_log2 == 4 and st.blocks == 1441 * 126 * 126          # 8 x 8 blocks would be 9.1e7 bounds: over the budget of 2^26
    e.close()


def test_argument_errors_leave_the_statistics(gpu_ctx, maps):
    m = maps["obstacle_slam_10mx10m_5cm"]
    truth = truth_of(m["cells"])
    g = bl.OccupancyGrid.from_cells(truth, m["origin"], m["mpc"], cellsPerMeter=CPM, ctx=gpu_ctx)
    pose = (-0.75, 0.2, 0.0)
    scan = synth.raycast_scan(truth, m["origin"], 0.05, pose, pose, 1)
    c = bl.make_pose(*pose)
    sm_ = bl.ScanMatcher(ctx=gpu_ctx)

    def status(fn):
        with pytest.raises(bl.BotlabHipError) as e:
            fn()
        return int(str(e.value).split("status ")[1].split(")")[0])

    assert status(sm_.wide_stats) == 4                              # no wide match yet
    ok = dict(nx=20, ny=10, ntheta=12, dtheta=DTH, max_range=8.0)
    first = sm_.match_wide(scan, c, g, **ok)
    before = bytes(sm_.wide_stats())
    for bad in [dict(nx=4097), dict(nx=-1), dict(ny=4097), dict(ny=-1), dict(ntheta=721), dict(ntheta=-1), dict(dtheta=0.0),
                dict(dtheta=-0.01), dict(dtheta=float("nan")), dict(block_log2=7), dict(block_log2=-1),
                dict(nx=4096, ny=4096, ntheta=720, block_log2=3),                    # 3.8e8 bounds: over the budget
                dict(nx=4096, ny=4096, ntheta=20, exhaustive=True)]:                 # 2.7e9 candidates: over the exhaustive limit
        assert status(lambda: sm_.match_wide(scan, c, g, **dict(ok, **bad))) == 2, bad
        assert bytes(sm_.wide_stats()) == before
    many = bl.LidarScan(np.full(4097, 1.0, np.float32), np.zeros(4097, np.float32), np.zeros(4097, np.int64))
    assert status(lambda: sm_.match_wide(many, c, g, **ok)) == 2
    many.ranges[0] = 0.0                                          # 4096 valid rays are allowed
    assert sm_.match_wide(many, c, g, **ok).rays_used == 4096
    lib = gpu_ctx.lib
    ls, p, r = scan.as_c(), _capi.ScanMatchWideParams(20, 10, 12, float(DTH), 8.0, 0, 0, 0), _capi.ScanMatchResult()
    assert lib.bl_scanmatch_match_wide(sm_.h, g.h, C.byref(ls), C.byref(c), C.byref(p), C.byref(r)) == 0
    assert bytes(r) == bytes(first)
    before = bytes(sm_.wide_stats())
    assert lib.bl_scanmatch_match_wide(None, g.h, C.byref(ls), C.byref(c), C.byref(p), C.byref(r)) == 2
    assert lib.bl_scanmatch_match_wide(sm_.h, None, C.byref(ls), C.byref(c), C.byref(p), C.byref(r)) == 2
    assert lib.bl_scanmatch_match_wide(sm_.h, g.h, None, C.byref(c), C.byref(p), C.byref(r)) == 2
    assert lib.bl_scanmatch_match_wide(sm_.h, g.h, C.byref(ls), None, C.byref(p), C.byref(r)) == 2
    assert lib.bl_scanmatch_match_wide(sm_.h, g.h, C.byref(ls), C.byref(c), None, C.byref(r)) == 2
    assert lib.bl_scanmatch_match_wide(sm_.h, g.h, C.byref(ls), C.byref(c), C.byref(p), None) == 2
    nul = _capi.Lidar(0, 5, None, None, None, None)
    assert lib.bl_scanmatch_match_wide(sm_.h, g.h, C.byref(nul), C.byref(c), C.byref(p), C.byref(r)) == 2
    assert lib.bl_scanmatch_wide_stats(None, None) == 2 and lib.bl_scanmatch_wide_stats(sm_.h, None) == 2
    assert bytes(r) == bytes(first) and bytes(sm_.wide_stats()) == before
    # the narrow entry point and its kept volume are not disturbed by wide matches
    sm_.match(scan, c, g, nx=2, ny=2, ntheta=1, dtheta=DTH, max_range=8.0, keep_volume=True)
    sm_.match_wide(scan, c, g, **ok)
    assert sm_.volume().shape == (3, 5, 5)
    sm_.close(); g.close()
