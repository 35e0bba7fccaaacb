"""The model of the correlative scan matcher (tests/scan_match_model.py) against the definition spelled as plain loops, its
tie-break order, and what the matcher is for: recovering a known offset, and tracking a trajectory from the scans alone."""
import math

import numpy as np

import helpers
import scan_match_model as sm
from botlab_amd import synth

CPM = helpers.CPM_DEFAULT
DTH = np.float32(math.radians(0.5))
CHAIN_MAPS = ["obstacle_slam_10mx10m_5cm", "convex_10mx10m_5cm", "drive_square_10mx10m_5cm"]
CHAIN_START = (-0.75, 0.2, 0.0)
CHAIN_STEPS = 60
CHAIN_TRAJ = dict(step_len=0.04, side=0.8)
CHAIN_WINDOW = dict(nx=4, ny=4, ntheta=12, dtheta=DTH)


def truth_of(cells):
    return np.where(cells > 0, 127, -127).astype(np.int8)


def chain(truth, origin, mpc, poses, window=CHAIN_WINDOW, max_range=synth.MAX_RANGE):
    """Every match centred on the previous match, no odometry at all.  Returns the corrected poses (one per scan)."""
    last = tuple(np.float32(v) for v in poses[0])
    out = []
    for k in range(1, len(poses)):
        scan = synth.raycast_scan(truth, origin, float(mpc), poses[k - 1], poses[k], 1000 + 100000 * k)
        r = sm.match(truth, origin, mpc, CPM, scan.ranges, scan.thetas, last, max_range=max_range, utime=scan.utime, **window)
        last = (r["x"], r["y"], r["theta"])
        out.append(r)
    return out


def test_model_equals_brute_force_on_small_windows(maps):
    m = maps["obstacle_slam_10mx10m_5cm"]
    truth = truth_of(m["cells"])
    scan = synth.raycast_scan(truth, m["origin"], 0.05, (-0.75, 0.2, 0.1), (-0.75, 0.2, 0.1), 1000, rays=48)
    for (nx, ny, nt), centre in [((2, 1, 1), (-0.70, 0.25, 0.08)), ((0, 3, 0), (-0.75, 0.2, 0.1)), ((3, 3, 2), (-4.95, -4.9, 2.0)),
                                 ((1, 2, 1), (-6.0, 0.0, -3.1))]:
        r = sm.match(truth, m["origin"], m["mpc"], CPM, scan.ranges, scan.thetas, centre, nx, ny, nt, DTH, 8.0)
        bf = sm.brute_force_volume(truth, m["origin"], CPM, scan.ranges, scan.thetas, centre, nx, ny, nt, DTH, 8.0)
        assert np.array_equal(r["volume"], bf)
        assert r["score"] == bf.max() and r["score_centre"] == bf[nt, ny, nx]
        assert r["ties"] == int((bf == bf.max()).sum())


def test_tie_break_order():
    # one ray along +x from the grid's middle: its endpoint cell is (30, 20) at heading 0.  Occupied cells placed so that
    # several candidates share the best score; the winner is fixed by d2, then |dk|, dk, dj, di.
    origin, mpc = (0.0, 0.0), np.float32(0.05)
    ranges, thetas = np.array([0.5], np.float32), np.array([0.0], np.float32)
    centre = (1.025, 1.025, 0.0)                                    # cell (20.5, 20.5) -> endpoint (30, 20)
    ex, ey, has = sm.endpoints(ranges, thetas, tuple(np.float32(v) for v in centre), 0, DTH, origin, CPM)
    assert (int(ex[0]), int(ey[0]), bool(has[0])) == (30, 20, True)

    def best(occupied, nt=0):
        cells = np.full((40, 60), -127, np.int8)
        for x, y in occupied:
            cells[y, x] = 100
        r = sm.match(cells, origin, mpc, CPM, ranges, thetas, centre, 3, 3, nt, DTH, 8.0)
        return r["di"], r["dj"], r["dk"], r["ties"]

    assert best([(32, 20), (30, 21)])[:2] == (0, 1)                  # d2 = 4 against d2 = 1
    assert best([(31, 20), (29, 20)])[:2] == (-1, 0)                 # same d2, same dj: the smaller di
    assert best([(31, 20), (30, 19)])[:2] == (0, -1)                 # same d2: the smaller dj before the smaller di
    assert best([(30, 21), (30, 19), (29, 20), (31, 20)])[:2] == (0, -1)
    # headings: the endpoint stays in cell (30, 20) for +-1 step of half a degree (10 cells * sin(0.5 deg) = 0.09 cell), so
    # all three headings tie at di = dj = 0: |dk| = 0 wins; with the cell one to the right every heading ties at di = 1 likewise
    di, dj, dk, ties = best([(30, 20)], nt=1)
    assert (di, dj, dk, ties) == (0, 0, 0, 3)
    # a map on which only dk = +-1 score: a 3 m ray (60 cells) moves half a cell sideways per step, off row 20 either way
    rl = np.array([3.0], np.float32)
    c3 = tuple(np.float32(v) for v in centre)
    e_m = sm.endpoints(rl, thetas, c3, -1, DTH, origin, CPM)
    e_p = sm.endpoints(rl, thetas, c3, 1, DTH, origin, CPM)
    e_0 = sm.endpoints(rl, thetas, c3, 0, DTH, origin, CPM)
    assert int(e_m[1][0]) != int(e_0[1][0]) and int(e_p[1][0]) != int(e_0[1][0])
    cells = np.full((60, 120), -127, np.int8)
    cells[int(e_m[1][0]), int(e_m[0][0])] = 100
    cells[int(e_p[1][0]), int(e_p[0][0])] = 100
    r = sm.match(cells, origin, mpc, CPM, rl, thetas, centre, 0, 0, 1, DTH, 8.0)
    assert r["score"] == 100 and r["ties"] == 2 and r["dk"] == -1                       # |dk| equal: the smaller dk


def test_all_free_map_returns_the_centre(maps):
    cells = np.full((200, 200), -127, np.int8)
    scan = synth.raycast_scan(truth_of(maps["convex_10mx10m_5cm"]["cells"]), (-5.0, -5.0), 0.05, (0, 0, 0), (0, 0, 0), 1000)
    centre = (0.3, -0.2, 3.0)
    r = sm.match(cells, (-5.0, -5.0), np.float32(0.05), CPM, scan.ranges, scan.thetas, centre, 4, 5, 6, DTH, 8.0, min_score=0)
    assert (r["di"], r["dj"], r["dk"], r["score"], r["accepted"]) == (0, 0, 0, 0, 1)
    assert r["ties"] == 9 * 11 * 13
    assert (r["x"], r["y"], r["theta"]) == tuple(np.float32(v) for v in centre)
    r = sm.match(cells, (-5.0, -5.0), np.float32(0.05), CPM, scan.ranges, scan.thetas, centre, 4, 5, 6, DTH, 8.0, min_score=1)
    assert r["accepted"] == 0 and (r["x"], r["y"], r["theta"]) == tuple(np.float32(v) for v in centre)


def test_known_offset_is_recovered(maps):
    m = maps["obstacle_slam_10mx10m_5cm"]
    truth = truth_of(m["cells"])
    pose = (-0.75, 0.2, 0.3)
    scan = synth.raycast_scan(truth, m["origin"], 0.05, pose, pose, 1000)
    centre = (pose[0] - 3 * 0.05, pose[1] + 2 * 0.05, pose[2] - 4 * float(DTH))
    r = sm.match(truth, m["origin"], m["mpc"], CPM, scan.ranges, scan.thetas, centre, 6, 6, 10, DTH, 8.0)
    assert (r["di"], r["dj"], r["dk"]) == (3, -2, 4), r
    assert r["score"] > r["score_centre"] and r["accepted"] == 1


def test_chained_matches_track_without_odometry(maps):
    """60 steps of the square trajectory on the three reference SLAM maps, every match centred on the previous one.  The chain can
    only go on tracking while its error stays inside the window (4 cells, 12 steps of half a degree): that is the bound.  The
    figures are printed (python -m pytest -s) and recorded in DESIGN.md section 4.11."""
    poses = synth.square_trajectory(CHAIN_START, CHAIN_STEPS, **CHAIN_TRAJ)
    for name in CHAIN_MAPS:
        m = maps[name]
        res = chain(truth_of(m["cells"]), m["origin"], m["mpc"], poses)
        pos = [math.hypot(float(r["x"]) - poses[k + 1][0], float(r["y"]) - poses[k + 1][1]) for k, r in enumerate(res)]
        ang = [abs(math.degrees(math.atan2(math.sin(float(r["theta"]) - poses[k + 1][2]), math.cos(float(r["theta"]) - poses[k + 1][2]))))
               for k, r in enumerate(res)]
        print("%s: worst %.3f m / %.2f deg, final %.3f m / %.2f deg, most ties %d" % (name, max(pos), max(ang), pos[-1], ang[-1],
                                                                                     max(r["ties"] for r in res)))
        assert max(pos) <= 4 * 0.05 and max(ang) <= 12 * 0.5
