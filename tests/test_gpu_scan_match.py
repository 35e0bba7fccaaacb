"""bl_scanmatch_* (botlab_amd/csrc/bl_scanmatch.hip) against the model (tests/scan_match_model.py): the result struct and the whole
score volume, bit for bit.  The definition is exact, so the allowed number of mismatches is 0 and no case is left out."""
import math

import numpy as np
import pytest

import botlab_amd as bl
import helpers
import scan_match_model as sm
from botlab_amd import synth

pytestmark = pytest.mark.gpu
CPM = helpers.CPM_DEFAULT
DTH = np.float32(math.radians(0.5))


def truth_of(cells):
    return np.where(cells > 0, 127, -127).astype(np.int8)


def compare(matcher, grid, cells, origin, mpc, cpm, scan, centre, nx, ny, ntheta, dtheta=DTH, max_range=8.0, min_score=0):
    """One match on the device with the volume kept, every field and every score against the model.  Returns (result, model)."""
    c = bl.make_pose(*centre, utime=7)
    res = matcher.match(scan, c, grid, nx=nx, ny=ny, ntheta=ntheta, dtheta=dtheta, max_range=max_range, min_score=min_score,
                        keep_volume=True)
    vol = matcher.volume()
    ref = sm.match(cells, origin, mpc, cpm, scan.ranges, scan.thetas, (c.x, c.y, c.theta), nx, ny, ntheta, dtheta, max_range,
                   min_score=min_score, utime=scan.utime)
    mismatches = int((vol != ref["volume"]).sum())
    assert vol.shape == ref["volume"].shape and mismatches == 0, "%d of %d scores differ" % (mismatches, vol.size)
    got = (res.di, res.dj, res.dk, res.score, res.score_centre, res.ties, res.rays_used, res.accepted, res.pose.utime)
    exp = (ref["di"], ref["dj"], ref["dk"], ref["score"], ref["score_centre"], ref["ties"], ref["rays_used"], ref["accepted"], ref["utime"])
    assert got == exp, (got, exp)
    gp = np.array([res.pose.x, res.pose.y, res.pose.theta], dtype=np.float32)
    ep = np.array([ref["x"], ref["y"], ref["theta"]], dtype=np.float32)
    assert gp.tobytes() == ep.tobytes(), (gp, ep)
    # the same match without the volume gives the same result
    res2 = matcher.match(scan, c, grid, nx=nx, ny=ny, ntheta=ntheta, dtheta=dtheta, max_range=max_range, min_score=min_score)
    assert bytes(res2) == bytes(res)
    return res, ref


@pytest.fixture(scope="module")
def matcher(gpu_ctx):
    m = bl.ScanMatcher(ctx=gpu_ctx)
    yield m
    m.close()


SLAM_CASES = [
    # centre offset from the scan's pose (m, m, rad), window
    ((0.0, 0.0, 0.0), (4, 4, 12)),
    ((0.12, -0.08, 0.03), (4, 4, 12)),
    ((-0.3, 0.2, -0.1), (10, 3, 20)),             # nx != ny
    ((0.1, 0.1, 0.0), (7, 9, 0)),                 # ntheta = 0
    ((0.0, 0.0, 0.0), (0, 0, 5)),                 # headings only
    ((0.5, -0.4, 0.2), (20, 20, 30)),
]


@pytest.mark.parametrize("name", helpers.SLAM_MAPS)
def test_reference_maps(gpu_ctx, matcher, maps, name):
    m = maps[name]
    truth = truth_of(m["cells"])
    g = bl.OccupancyGrid.from_cells(truth, m["origin"], m["mpc"], cellsPerMeter=CPM, ctx=gpu_ctx)
    pose = (-0.75, 0.2, 0.4)
    scan = synth.raycast_scan(truth, m["origin"], 0.05, pose, pose, 123456)
    for off, (nx, ny, nt) in SLAM_CASES:
        centre = (pose[0] + off[0], pose[1] + off[1], pose[2] + off[2])
        res, _ = compare(matcher, g, truth, m["origin"], m["mpc"], CPM, scan, centre, nx, ny, nt)
        assert matcher.debugPath() == 0                      # a 10 m map always fits in LDS
    # the map as a SLAM run leaves it (mixed log-odds, not just +-127): the reference cells themselves
    g2 = bl.OccupancyGrid.from_cells(m["cells"], m["origin"], m["mpc"], cellsPerMeter=CPM, ctx=gpu_ctx)
    compare(matcher, g2, m["cells"], m["origin"], m["mpc"], CPM, scan, (pose[0] + 0.05, pose[1], pose[2] - 0.02), 5, 6, 8)
    # a window that pushes endpoints off every edge: max-range returns (8 m on a 10 m map) count as hits here, +-64 cells
    compare(matcher, g, truth, m["origin"], m["mpc"], CPM, scan, (0.3, -0.2, 1.0), 64, 64, 2, max_range=9.0)
    # centres outside the grid: just outside (part of the scan lands on it) and far outside (nothing does)
    compare(matcher, g, truth, m["origin"], m["mpc"], CPM, scan, (-5.6, 0.1, 0.0), 12, 5, 3, max_range=9.0)
    res, _ = compare(matcher, g, truth, m["origin"], m["mpc"], CPM, scan, (40.0, -37.0, 2.0), 6, 6, 2)
    assert (res.di, res.dj, res.dk, res.score) == (0, 0, 0, 0)
    g.close(); g2.close()


def test_window_limits(gpu_ctx, matcher, maps):
    m = maps["obstacle_slam_10mx10m_5cm"]
    truth = truth_of(m["cells"])
    g = bl.OccupancyGrid.from_cells(truth, m["origin"], m["mpc"], cellsPerMeter=CPM, ctx=gpu_ctx)
    pose = (-0.75, 0.2, 0.4)
    scan = synth.raycast_scan(truth, m["origin"], 0.05, pose, pose, 99)
    compare(matcher, g, truth, m["origin"], m["mpc"], CPM, scan, (pose[0] + 1.0, pose[1] - 0.7, pose[2] + 0.5), 64, 64, 180)
    g.close()


@pytest.mark.parametrize("w,h", [(199, 200), (187, 150), (202, 93), (208, 131), (65, 70), (1, 1), (3, 257)])
def test_grid_widths(gpu_ctx, matcher, maps, w, h):
    m = maps["convex_10mx10m_5cm"]
    full = truth_of(m["cells"])
    cells = np.ascontiguousarray(full[:h, :w]) if h <= 200 else np.ascontiguousarray(np.tile(full, (2, 1))[:h, :w])
    g = bl.OccupancyGrid.from_cells(cells, m["origin"], m["mpc"], cellsPerMeter=CPM, ctx=gpu_ctx)
    pose = (-3.0, -2.6, -0.7)
    scan = synth.raycast_scan(cells, m["origin"], 0.05, pose, pose, 5)
    compare(matcher, g, cells, m["origin"], m["mpc"], CPM, scan, (pose[0] + 0.1, pose[1] - 0.05, pose[2] + 0.02), 9, 6, 7, max_range=9.0)
    compare(matcher, g, cells, m["origin"], m["mpc"], CPM, scan, (-4.9, -4.9, 0.3), 30, 17, 3, max_range=9.0)
    g.close()


def test_large_grid_both_paths(gpu_ctx, matcher, maps):
    world = synth.tile_world(maps["obstacle_slam_10mx10m_5cm"]["cells"], 2000)
    origin, mpc = (-50.0, -50.0), np.float32(0.05)
    g = bl.OccupancyGrid.from_cells(world, origin, mpc, cellsPerMeter=CPM, ctx=gpu_ctx)
    pose = (3.3, -7.1, 0.9)
    near = synth.raycast_scan(world, origin, 0.05, pose, pose, 11)                       # 8 m lidar: the window is a few hundred cells
    compare(matcher, g, world, origin, mpc, CPM, near, (pose[0] + 0.1, pose[1] + 0.1, pose[2] - 0.03), 6, 4, 10)
    assert matcher.debugPath() == 0
    # a long-range scan: endpoints spread over more cells than LDS holds, the grid is read directly
    rays = 290
    thetas = (2.0 * np.pi * np.arange(rays) / rays).astype(np.float32)
    rng = np.random.default_rng(5)
    far = bl.LidarScan(rng.uniform(0.2, 45.0, rays).astype(np.float32), thetas, np.arange(rays, dtype=np.int64), utime=12)
    compare(matcher, g, world, origin, mpc, CPM, far, (pose[0], pose[1], pose[2]), 6, 4, 10, max_range=50.0)
    assert matcher.debugPath() == 1
    compare(matcher, g, world, origin, mpc, CPM, far, (-49.0, 48.0, -2.0), 64, 33, 4, max_range=50.0)       # off two edges, direct
    assert matcher.debugPath() == 1
    # and back: the staged path after the direct one
    compare(matcher, g, world, origin, mpc, CPM, near, (pose[0], pose[1], pose[2]), 3, 3, 3)
    assert matcher.debugPath() == 0
    g.close()


def test_invalid_and_max_range_rays(gpu_ctx, matcher, maps):
    m = maps["drive_square_10mx10m_5cm"]
    truth = truth_of(m["cells"])
    g = bl.OccupancyGrid.from_cells(truth, m["origin"], m["mpc"], cellsPerMeter=CPM, ctx=gpu_ctx)
    pose = (-0.75, 0.2, 0.0)
    scan = synth.raycast_scan(truth, m["origin"], 0.05, pose, pose, 1)
    r = scan.ranges.copy()
    r[::7] = 0.1; r[3::11] = 0.15; r[5::13] = 0.0; r[1::17] = -1.0; r[2::19] = 8.0; r[4::23] = np.inf; r[6::29] = np.nan
    r[8::31] = np.float32(0.15000001)
    bad = bl.LidarScan(r, scan.thetas, scan.times, utime=77)
    res, ref = compare(matcher, g, truth, m["origin"], m["mpc"], CPM, bad, (pose[0] + 0.05, pose[1], pose[2]), 4, 4, 6, max_range=8.0)
    assert 0 < res.rays_used < 290
    # no valid ray at all
    none = bl.LidarScan(np.full(290, 9.0, np.float32), scan.thetas, scan.times, utime=78)
    res, _ = compare(matcher, g, truth, m["origin"], m["mpc"], CPM, none, pose, 2, 3, 4)
    assert (res.rays_used, res.score, res.ties, res.di, res.dj, res.dk) == (0, 0, 5 * 7 * 9, 0, 0, 0)
    empty = bl.LidarScan(np.zeros(0, np.float32), np.zeros(0, np.float32), np.zeros(0, np.int64), utime=79)
    compare(matcher, g, truth, m["origin"], m["mpc"], CPM, empty, pose, 1, 1, 1)
    g.close()


def test_min_score_above_the_best(gpu_ctx, matcher, maps):
    m = maps["obstacle_slam_10mx10m_5cm"]
    truth = truth_of(m["cells"])
    g = bl.OccupancyGrid.from_cells(truth, m["origin"], m["mpc"], cellsPerMeter=CPM, ctx=gpu_ctx)
    pose = (-0.75, 0.2, 0.0)
    scan = synth.raycast_scan(truth, m["origin"], 0.05, pose, pose, 1)
    centre = (pose[0] + 0.1, pose[1] - 0.1, pose[2] + 0.05)
    res, ref = compare(matcher, g, truth, m["origin"], m["mpc"], CPM, scan, centre, 4, 4, 12)
    assert res.accepted == 1 and res.score > 0
    rej, _ = compare(matcher, g, truth, m["origin"], m["mpc"], CPM, scan, centre, 4, 4, 12, min_score=res.score + 1)
    c = bl.make_pose(*centre)
    assert rej.accepted == 0 and (rej.pose.x, rej.pose.y, rej.pose.theta) == (c.x, c.y, c.theta) and rej.score == res.score
    edge, _ = compare(matcher, g, truth, m["origin"], m["mpc"], CPM, scan, centre, 4, 4, 12, min_score=res.score)
    assert edge.accepted == 1
    # an empty map: the centre, whatever the scan
    e = bl.OccupancyGrid.from_cells(np.zeros((200, 200), np.int8), m["origin"], m["mpc"], cellsPerMeter=CPM, ctx=gpu_ctx)
    res, _ = compare(matcher, e, np.zeros((200, 200), np.int8), m["origin"], m["mpc"], CPM, scan, centre, 4, 4, 12, min_score=1)
    assert (res.score, res.accepted, res.di, res.dj, res.dk) == (0, 0, 0, 0, 0)
    g.close(); e.close()


def test_argument_errors_and_volume_state(gpu_ctx, maps):
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

    with pytest.raises(bl.BotlabHipError):                       # nothing matched yet
        sm_.volume()
    ok = dict(nx=4, ny=4, ntheta=12, dtheta=DTH, max_range=8.0)
    for bad in [dict(nx=65), dict(nx=-1), dict(ny=65), dict(ny=-1), dict(ntheta=181), dict(ntheta=-1), dict(dtheta=0.0),
                dict(dtheta=-0.01), dict(dtheta=float("nan"))]:
        assert status(lambda: sm_.match(scan, c, g, **dict(ok, **bad))) == 2, bad
    n = 4097
    many = bl.LidarScan(np.full(n, 1.0, np.float32), np.zeros(n, np.float32), np.zeros(n, np.int64))
    assert status(lambda: sm_.match(many, c, g, **ok)) == 2
    many.ranges[0] = 0.0                                          # 4096 valid rays are allowed
    assert sm_.match(many, c, g, **ok).rays_used == 4096
    # null pointers, straight at the C ABI
    lib, C = gpu_ctx.lib, __import__("ctypes")
    from botlab_amd import _capi
    ls, p, r = scan.as_c(), _capi.ScanMatchParams(4, 4, 12, float(DTH), 8.0, 0, 0), _capi.ScanMatchResult()
    assert lib.bl_scanmatch_create(None, C.byref(C.c_void_p())) == 2 and lib.bl_scanmatch_create(gpu_ctx.h, None) == 2
    assert lib.bl_scanmatch_match(None, g.h, C.byref(ls), C.byref(c), C.byref(p), C.byref(r)) == 2
    assert lib.bl_scanmatch_match(sm_.h, None, C.byref(ls), C.byref(c), C.byref(p), C.byref(r)) == 2
    assert lib.bl_scanmatch_match(sm_.h, g.h, None, C.byref(c), C.byref(p), C.byref(r)) == 2
    assert lib.bl_scanmatch_match(sm_.h, g.h, C.byref(ls), None, C.byref(p), C.byref(r)) == 2
    assert lib.bl_scanmatch_match(sm_.h, g.h, C.byref(ls), C.byref(c), None, C.byref(r)) == 2
    assert lib.bl_scanmatch_match(sm_.h, g.h, C.byref(ls), C.byref(c), C.byref(p), None) == 2
    nul = _capi.Lidar(0, 5, None, None, None, None)
    assert lib.bl_scanmatch_match(sm_.h, g.h, C.byref(nul), C.byref(c), C.byref(p), C.byref(r)) == 2
    assert lib.bl_scanmatch_volume(None, None) == 2 and lib.bl_scanmatch_debug_path(None) == -1
    # the volume of a match that did not keep it
    sm_.match(scan, c, g, keep_volume=True, **ok)
    assert sm_.volume().shape == (25, 9, 9)
    sm_.match(scan, c, g, **ok)
    out = np.zeros(25 * 81, np.int32)
    assert lib.bl_scanmatch_volume(sm_.h, out.ctypes.data_as(C.c_void_p)) == 4
    sm_.close(); g.close()


def test_volume_after_a_refused_match(gpu_ctx, maps):
    """A kept volume does not outlive a later match that was refused: the library answers BL_ERR_STATE, the Python class raises and
    never hands the library a buffer of another size."""
    import ctypes as C
    m = maps["obstacle_slam_10mx10m_5cm"]
    truth = truth_of(m["cells"])
    g = bl.OccupancyGrid.from_cells(truth, m["origin"], m["mpc"], cellsPerMeter=CPM, ctx=gpu_ctx)
    pose = (-0.75, 0.2, 0.0)
    scan = synth.raycast_scan(truth, m["origin"], 0.05, pose, pose, 1)
    c = bl.make_pose(*pose)
    sm_ = bl.ScanMatcher(ctx=gpu_ctx)
    ok = dict(nx=4, ny=4, ntheta=12, dtheta=DTH, max_range=8.0)
    many = bl.LidarScan(np.full(4097, 1.0, np.float32), np.zeros(4097, np.float32), np.zeros(4097, np.int64))
    for refuse in [lambda: sm_.match(scan, c, g, keep_volume=True, **dict(ok, nx=65)),
                   lambda: sm_.match(many, c, g, keep_volume=True, **ok),
                   lambda: sm_.match(scan, c, g, **dict(ok, dtheta=0.0))]:
        sm_.match(scan, c, g, keep_volume=True, **ok)
        assert sm_.volume().shape == (25, 9, 9)
        with pytest.raises(bl.BotlabHipError):
            refuse()
        with pytest.raises(bl.BotlabHipError):
            sm_.volume()
        out = np.zeros(25 * 81, np.int32)                       # the library itself, with a buffer that would hold the old volume
        assert gpu_ctx.lib.bl_scanmatch_volume(sm_.h, out.ctypes.data_as(C.c_void_p)) == 4
    # and a kept match after the refusals serves its volume again
    sm_.match(scan, c, g, keep_volume=True, **dict(ok, nx=2))
    assert sm_.volume().shape == (25, 9, 5)
    sm_.close(); g.close()
