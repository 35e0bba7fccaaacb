"""The model of the wide scan match (tests/scan_match_wide_model.py): the block bound really bounds, the pruned matcher returns
what the exhaustive one returns -- every field, `ties` included -- and a whole-map, half-circle window recovers the pose of a
scan with no prior."""
import math

import numpy as np
import pytest

import helpers
import scan_match_model as sm
import scan_match_wide_model as smw
from botlab_amd import synth

CPM = helpers.CPM_DEFAULT
DTH = np.float32(math.radians(0.5))
WHOLE_MAPS = ["obstacle_slam_10mx10m_5cm", "convex_10mx10m_5cm", "drive_square_10mx10m_5cm"]
WHOLE_POSE = (-0.75, 0.2, math.radians(6.0))
WHOLE_WINDOW = dict(nx=100, ny=100, ntheta=90, dtheta=np.float32(math.radians(2.0)))
# blocks that any exact single-level pruner must still score on these inputs (bound >= the best score)
WHOLE_KEPT_MIN = {("obstacle_slam_10mx10m_5cm", 2): 1, ("obstacle_slam_10mx10m_5cm", 3): 5, ("obstacle_slam_10mx10m_5cm", 4): 109,
                  ("convex_10mx10m_5cm", 3): 17, ("drive_square_10mx10m_5cm", 3): 23}


def truth_of(cells):
    return np.where(cells > 0, 127, -127).astype(np.int8)


def check_bounds_and_pruning(cells, origin, mpc, ranges, thetas, centre, nx, ny, nt, dtheta, max_range, hs, min_score=0):
    """Exhaustive volume once; for every block size: bound >= block maximum everywhere, pruned == exhaustive.  Returns
    (exhaustive result, {h: pruned result})."""
    ex = smw.match_exhaustive(cells, origin, mpc, CPM, ranges, thetas, centre, nx, ny, nt, dtheta, max_range, min_score=min_score,
                              utime=5, keep_volume=True)
    vr, vt = sm.valid_rays(ranges, thetas, max_range)
    c32 = tuple(np.float32(v) for v in centre)
    out = {}
    for h in hs:
        bounds = smw.block_bounds(cells, origin, CPM, vr, vt, c32, nx, ny, nt, np.float32(dtheta), h)
        maxima = smw.block_maxima(ex["volume"], h)
        assert bounds.shape == maxima.shape
        assert int((bounds < maxima).sum()) == 0, "h=%d: %d blocks above their bound" % (h, int((bounds < maxima).sum()))
        pr = smw.match_pruned(cells, origin, mpc, CPM, ranges, thetas, centre, nx, ny, nt, dtheta, max_range, h, min_score=min_score,
                              utime=5)
        assert smw.same_result(pr, ex), (h, {f: (pr[f], ex[f]) for f in smw.RESULT_FIELDS})
        assert pr["kept"] >= pr["kept_min"] or pr["score"] == 0
        assert pr["kept_min"] == int((bounds >= ex["score"]).sum())
        out[h] = pr
    return ex, out


@pytest.mark.parametrize("name", WHOLE_MAPS)
def test_whole_map_window_recovers_the_pose(maps, name):
    """+-100 x +-100 cells x +-90 steps of 2 degrees around (0, 0, 0) on a 200 x 200 map: 7.3e6 candidates, the scan cast at
    (-0.75, 0.2, 6 deg).  The true pose is the unique best candidate (-15, 4, 3); the counts of blocks that must be scored are
    those recorded in DESIGN.md section 4.12."""
    m = maps[name]
    truth = truth_of(m["cells"])
    scan = synth.raycast_scan(truth, m["origin"], 0.05, WHOLE_POSE, WHOLE_POSE, 1000)
    ex, pruned = check_bounds_and_pruning(truth, m["origin"], m["mpc"], scan.ranges, scan.thetas, (0.0, 0.0, 0.0), max_range=8.0,
                                          hs=(2, 3, 4), nt=WHOLE_WINDOW["ntheta"], nx=100, ny=100, dtheta=WHOLE_WINDOW["dtheta"])
    assert (ex["di"], ex["dj"], ex["dk"], ex["ties"]) == (-15, 4, 3, 1), ex
    for h, pr in pruned.items():
        print("%s: B=%d blocks %d, must score %d, the model scored %d blocks / %d of %d candidates" %
              (name, 1 << h, pr["blocks"], pr["kept_min"], pr["kept"], pr["candidates_scored"], pr["candidates"]))
        if (name, h) in WHOLE_KEPT_MIN:
            assert pr["kept_min"] == WHOLE_KEPT_MIN[(name, h)]
        assert pr["candidates_scored"] * 10 <= pr["candidates"]


@pytest.mark.parametrize("w,h", [(199, 200), (187, 150), (65, 70), (1, 1), (3, 257)])
def test_ragged_grids(maps, w, h):
    """Widths that are no multiple of B, windows whose edges cut blocks, endpoints off the grid."""
    full = truth_of(maps["convex_10mx10m_5cm"]["cells"])
    cells = np.ascontiguousarray(full[:h, :w]) if h <= 200 else np.ascontiguousarray(np.tile(full, (2, 1))[:h, :w])
    origin, mpc = maps["convex_10mx10m_5cm"]["origin"], maps["convex_10mx10m_5cm"]["mpc"]
    pose = (-3.0, -2.6, -0.7)
    scan = synth.raycast_scan(cells, origin, 0.05, pose, pose, 5)
    check_bounds_and_pruning(cells, origin, mpc, scan.ranges, scan.thetas, (pose[0] + 0.1, pose[1] - 0.05, pose[2] + 0.02), 9, 6, 3,
                             DTH, 9.0, hs=(1, 2, 3, 4))
    check_bounds_and_pruning(cells, origin, mpc, scan.ranges, scan.thetas, (-4.9, -4.9, 0.3), 30, 17, 2, DTH, 9.0, hs=(2, 3, 4, 6))


def test_all_free_map_and_min_score(maps):
    cells = np.full((200, 200), -127, np.int8)
    scan = synth.raycast_scan(truth_of(maps["convex_10mx10m_5cm"]["cells"]), (-5.0, -5.0), 0.05, (0, 0, 0), (0, 0, 0), 1000)
    centre = (0.3, -0.2, 3.0)
    for min_score in (0, 1):
        ex, pruned = check_bounds_and_pruning(cells, (-5.0, -5.0), np.float32(0.05), scan.ranges, scan.thetas, centre, 14, 15, 6, DTH,
                                              8.0, hs=(3,), min_score=min_score)
        assert (ex["di"], ex["dj"], ex["dk"], ex["score"], ex["ties"], ex["accepted"]) == (0, 0, 0, 0, 29 * 31 * 13, 1 - min_score)
        assert pruned[3]["candidates_scored"] == 0


def test_ties_in_different_blocks():
    """One ray, four occupied cells far apart: four candidates in four different 4 x 4 blocks tie at the best score."""
    origin, mpc = (0.0, 0.0), np.float32(0.05)
    ranges, thetas = np.array([0.5], np.float32), np.array([0.0], np.float32)
    centre = (1.025, 1.025, 0.0)                                    # endpoint cell (30, 20) at heading 0
    cells = np.full((40, 60), -127, np.int8)
    for x, y in [(30 + 9, 20 + 2), (30 - 9, 20 - 2), (30 + 2, 20 - 9), (30 - 2, 20 + 9)]:
        cells[y, x] = 100
    ex, pruned = check_bounds_and_pruning(cells, origin, mpc, ranges, thetas, centre, 12, 12, 0, DTH, 8.0, hs=(1, 2, 3))
    assert (ex["score"], ex["ties"], ex["di"], ex["dj"]) == (100, 4, 2, -9)          # equal d2: the smallest dj
    assert pruned[2]["kept_min"] == 4


def test_tie_break_constructions():
    """test_tie_break_order's maps (tests/test_scan_match_model_cpu.py) at +-3, through the pruned form."""
    origin, mpc = (0.0, 0.0), np.float32(0.05)
    ranges, thetas = np.array([0.5], np.float32), np.array([0.0], np.float32)
    centre = (1.025, 1.025, 0.0)

    def best(occupied, nt=0):
        cells = np.full((40, 60), -127, np.int8)
        for x, y in occupied:
            cells[y, x] = 100
        ex, _ = check_bounds_and_pruning(cells, origin, mpc, ranges, thetas, centre, 3, 3, nt, DTH, 8.0, hs=(1, 2, 3))
        return ex["di"], ex["dj"], ex["dk"], ex["ties"]

    assert best([(32, 20), (30, 21)])[:2] == (0, 1)
    assert best([(31, 20), (29, 20)])[:2] == (-1, 0)
    assert best([(31, 20), (30, 19)])[:2] == (0, -1)
    assert best([(30, 21), (30, 19), (29, 20), (31, 20)])[:2] == (0, -1)
    assert best([(30, 20)], nt=1) == (0, 0, 0, 3)


def test_saturation_arithmetic():
    assert smw.saturate(2 ** 31 - 1) == 2 ** 31 - 1 and smw.saturate(2 ** 31) == 2 ** 31 - 1 and smw.saturate(7) == 7
    assert smw.saturate(8193 * 8193 * 1441) == 2 ** 31 - 1            # an all-free map at the limits: 9.7e10 candidates
