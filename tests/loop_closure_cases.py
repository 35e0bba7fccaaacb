"""Named cases of the loop-closure front end (tests/loop_closure_model.py).  TEST INFRASTRUCTURE, no GPU.

Every case is a small scan history -- a 120 x 120 world of 5 cm cells ray-cast with botlab_amd.synth, a robot on a circle of 0.5 m
radius, the recorded poses the truth's steps replayed with a constant heading bias -- the parameters of a find, and `reaches`: the
condition, evaluated on the model, that shows the case takes the path it is named for.  model(case) is computed once and shared by the
CPU and the GPU tests."""
import math

import numpy as np

import botlab_amd as bl
from botlab_amd import synth

import loop_closure_model as lcm
import oracle_lib

SIZE, MPC, CPM, ORIGIN = 120, 0.05, 20.0, (-3.0, -3.0)
RADIUS, BIAS = 0.5, 0.0004
MAX_LASER, HIT, MISS = 5.0, 3, 1
# The stated edge arithmetic against the formulation of botlab_amd.find_loop_closures (np.linalg.inv, atan2(sin, cos), libm's double sine
# and cosine), measured by tests/test_loop_closure_model_cpu.py over the kept edges of the case set: info differs by at most 1.44e-8 of
# the edge's largest information entry (the 1.25 cm case, whose quantisation term is the smallest; 4.2e-9 at 5 cm), z by at most 2.5e-8.  The bounds are four times the measured values.
INFO_REL_BOUND = 4 * 1.44e-8
Z_ABS_BOUND = 4 * 2.5e-8
BASE = dict(stride=1, min_gap=6, radius=0.25, w=3, submap_cells=64, nx=3, ny=3, ntheta=3, dtheta=math.radians(0.5), max_range=8.0,
            half_life=64, min_score=0, maxLaserDistance=MAX_LASER, hitOdds=HIT, missOdds=MISS, prior=(0, 0, 0, 0))


def world():
    cells = np.zeros((SIZE, SIZE), np.int8)
    for y0, y1, x0, x1 in ((78, 83, 50, 72), (38, 43, 44, 60), (52, 70, 84, 88), (50, 66, 30, 34), (84, 90, 80, 86), (30, 34, 76, 84)):
        cells[y0:y1, x0:x1] = 100
    return synth.tile_world(cells, SIZE)


def _rel(a, b):
    c, s = math.cos(a[2]), math.sin(a[2])
    dx, dy = b[0] - a[0], b[1] - a[1]
    return np.array([c * dx + s * dy, -s * dx + c * dy, math.atan2(math.sin(b[2] - a[2]), math.cos(b[2] - a[2]))])


def trajectories(n, lap, bias=BIAS):
    t = np.arange(n) / lap * 2 * math.pi
    truth = np.stack([RADIUS * np.cos(t), RADIUS * np.sin(t), np.arctan2(np.sin(t + math.pi / 2), np.cos(t + math.pi / 2))], 1)
    rec = np.zeros_like(truth)
    rec[0] = truth[0]
    for k in range(n - 1):
        z = _rel(truth[k], truth[k + 1])
        c, s = math.cos(rec[k, 2]), math.sin(rec[k, 2])
        th = rec[k, 2] + z[2] + bias
        rec[k + 1] = [rec[k, 0] + c * z[0] - s * z[1], rec[k, 1] + s * z[0] + c * z[1], math.atan2(math.sin(th), math.cos(th))]
    return truth, rec


def history(n, lap, moving=False, rays=synth.RAYS, bias=BIAS):
    """(scans, poses): n LidarScans ray-cast at the truth and the recorded (x, y, theta, utime) as float32 / int.  Standing still every
    ray carries the scan's end time; moving, the rays are cast along the step and their times are spread over it."""
    w = world()
    truth, rec = trajectories(n, lap, bias)
    utimes = 100000 * (np.arange(n) + 1)
    scans = []
    for k in range(n):
        if moving and k > 0:
            scans.append(synth.raycast_scan(w, ORIGIN, MPC, truth[k - 1], truth[k], int(utimes[k]), rays=rays))
        else:
            s = synth.raycast_scan(w, ORIGIN, MPC, truth[k], truth[k], int(utimes[k]), rays=rays)
            scans.append(bl.LidarScan(s.ranges, s.thetas, np.full(s.num_ranges, int(utimes[k]), np.int64), utime=int(utimes[k])))
    poses = [(np.float32(rec[k, 0]), np.float32(rec[k, 1]), np.float32(rec[k, 2]), int(utimes[k])) for k in range(n)]
    return scans, poses


def _set_pose(poses, k, x=None, y=None, theta=None):
    p = poses[k]
    poses[k] = (np.float32(p[0] if x is None else x), np.float32(p[1] if y is None else y), np.float32(p[2] if theta is None else theta), p[3])


def _with_ranges(scan, ranges):
    r = np.asarray(ranges, np.float32)
    n = len(r)
    return bl.LidarScan(r, scan.thetas[:n].copy(), scan.times[:n].copy(), utime=scan.utime)


class Case:
    def __init__(self, name, scans, poses, params, reaches, capacity=None, max_rays=synth.RAYS, mpc=MPC, cpm=CPM):
        self.name, self.scans, self.poses, self.reaches = name, scans, poses, reaches
        self.mpc, self.cpm = mpc, cpm                          # of the `like` grid: the submaps' resolution
        self.params = dict(BASE, **params)
        self.capacity = capacity or len(scans)                 # of the log; below len(scans): the ring wraps
        self.max_rays = max_rays

    def retained(self):
        """what the log holds after every scan was appended"""
        return self.scans[-self.capacity:], self.poses[-self.capacity:]


_cases = None
FINE_MPC, FINE_CPM = 0.0125, 80.0
LDS_WINDOW_MAX = 152 * 1024            # SM_LDS_MAX


def _window_beyond_lds(m):
    """one candidate, and the box of its scan's endpoints at the centre heading, widened by the shifts and clipped to the submap, is
    larger than a workgroup may stage"""
    if len(m) != 1 or m[0]["ref"] is None:
        return False
    c = cases()["direct_window"]
    p, q = c.params, m[0]["q"]
    S = p["submap_cells"]
    r, t = lcm.smp.sm.valid_rays(c.scans[q].ranges, c.scans[q].thetas, p["max_range"])
    ex, ey, has = lcm.smp.sm.endpoints(r, t, tuple(np.float32(v) for v in c.poses[q][:3]), 0, np.float32(p["dtheta"]), m[0]["origin"], np.float32(FINE_CPM))
    on = has & (ex >= -p["nx"]) & (ex < S + p["nx"]) & (ey >= -p["ny"]) & (ey < S + p["ny"])
    x0, x1 = max(int(ex[on].min()) - p["nx"], 0), min(int(ex[on].max()) + p["nx"], S - 1)
    y0, y1 = max(int(ey[on].min()) - p["ny"], 0), min(int(ey[on].max()) + p["ny"], S - 1)
    return (x1 - (x0 & ~3) + 1) * (y1 - y0 + 1) > LDS_WINDOW_MAX and m[0]["ref"]["score"] > 0


def _hand_built():
    """24 scans; q = 20 recorded at (0, 0), j = 2 at (0.25, 0) and j = 5 at (-0.25, 0): d2 = 0.0625 exactly for both, every other
    older scan 0.5 m away."""
    scans, poses = history(24, 16)
    _set_pose(poses, 20, 0.0, 0.0)
    _set_pose(poses, 2, 0.25, 0.0)
    _set_pose(poses, 5, -0.25, 0.0)
    return scans, poses


def cases():
    global _cases
    if _cases is not None:
        return _cases
    two = history(32, 16)
    out = []

    def add(name, hist, params, reaches, **kw):
        out.append(Case(name, list(hist[0]), list(hist[1]), params, reaches, **kw))

    add("two_lap", two, dict(stride=1, submap_cells=130), lambda m: len(m) >= 8 and sum(c["flags"] == 0 for c in m) >= 3)
    add("none_in_radius", two, dict(radius=0.001), lambda m: len(m) == 0)
    add("short_log", (two[0][:6], two[1][:6]), dict(min_gap=12), lambda m: len(m) == 0)
    add("single", two, dict(stride=31), lambda m: len(m) == 1)
    add("wave_plus_one", history(69, 12, rays=100), dict(min_gap=3, radius=2.0, w=1, nx=2, ny=2, ntheta=2), lambda m: len(m) == 65,
        max_rays=100)
    hb = _hand_built()
    add("equal_d2", hb, dict(stride=20, radius=0.375, submap_cells=65),
        lambda m: len(m) == 1 and m[0]["j"] == 2 and m[0]["d2"][2] == m[0]["d2"][5] == min(m[0]["d2"]))
    add("at_radius", hb, dict(stride=20, radius=0.25, submap_cells=65), lambda m: len(m) == 1 and m[0]["d2"][m[0]["j"]] == 0.0625)
    below = float(np.nextafter(np.float32(0.25), np.float32(0.0)))
    add("beyond_radius", hb, dict(stride=20, radius=below, submap_cells=65),
        lambda m: len(m) == 0 and 0.0625 > below * below > 0.0625 * (1 - 2.0 ** -22))
    add("cut_start", two, dict(w=5, submap_cells=65), lambda m: any(c["j"] - 5 < 0 and c["first"] == 0 and c["count"] == c["j"] + 6 for c in m))
    add("cut_end", history(12, 16), dict(min_gap=3, radius=1.0, w=8),
        lambda m: len(m) == 8 and any(c["j"] + 8 > 11 and c["first"] + c["count"] == 12 for c in m))
    add("w0", two, dict(w=0, stride=4), lambda m: len(m) >= 2 and all(c["flags"] & lcm.TIED and not c["cells"].any() and c["count"] == 1 for c in m))
    add("wrapped_ring", two, dict(stride=2), lambda m: len(m) >= 3, capacity=24)

    scans, poses = list(two[0]), list(two[1])
    scans[20] = _with_ranges(scans[20], scans[20].ranges[:1])                              # one ray
    scans[22] = _with_ranges(scans[22], np.full(synth.RAYS, 9.0))                          # kept by the log, none valid for the matcher
    scans[24] = _with_ranges(scans[24], scans[24].ranges[:200])
    add("ray_counts", (scans, poses), dict(),
        lambda m: {c["q"]: c["valid"] for c in m}.get(20) == 1 and {c["q"]: c["valid"] for c in m}.get(22) == 0 and
        any(c["valid"] == synth.RAYS for c in m) and synth.RAYS % 64 != 0 and synth.RAYS > 256)

    scans, poses = list(two[0]), list(two[1])
    scans[20] = _with_ranges(scans[20], np.full(synth.RAYS, 7.0))                          # valid, every endpoint beyond the 3.2 m submap
    add("outside", (scans, poses), dict(stride=20),
        lambda m: len(m) == 1 and m[0]["valid"] == synth.RAYS and not m[0]["ref"]["score_volume"].any() and m[0]["flags"] & lcm.TIED)

    scans, poses = list(two[0]), list(two[1])
    _set_pose(poses, 20, x=float(poses[20][0]) + 0.25)                                     # five cells off: beyond the window of three
    add("on_edge", (scans, poses), dict(stride=20, radius=0.5, submap_cells=130), lambda m: len(m) == 1 and m[0]["flags"] == lcm.ON_EDGE)
    add("min_score", two, dict(stride=4, min_score=1 << 19, submap_cells=130),
        lambda m: len(m) >= 2 and all(c["flags"] & lcm.NOT_ACCEPTED for c in m))

    scans, poses = list(two[0]), list(two[1])
    _set_pose(poses, 20, x=float(poses[20][0]) + 0.1)                                      # two cells off, inside a window of four
    scans[20] = _with_ranges(scans[20], scans[20].ranges[:40])                             # few rays: the prior outweighs the scores
    add("prior_moves", (scans, poses), dict(stride=20, radius=0.5, submap_cells=130, nx=4, ny=4, prior=(32767, 0, 32767, 0)),
        lambda m: len(m) == 1 and (m[0]["ref"]["di"], m[0]["ref"]["dj"], m[0]["ref"]["dk"]) != tuple(m[0]["ref"]["raw_best"][:3]))
    add("moving", history(32, 16, moving=True), dict(stride=2, submap_cells=130),
        lambda m: len(m) >= 3 and any(c["flags"] == 0 for c in m))

    scans, poses = list(two[0]), list(two[1])
    big = scans[20]
    scans[20] = bl.LidarScan(np.tile(big.ranges, 15), np.tile(big.thetas, 15), np.tile(big.times, 15), utime=big.utime)
    add("too_many_rays", (scans, poses), dict(stride=10), lambda m: any(c["flags"] == lcm.TOO_MANY_RAYS and c["valid"] > 4096 for c in m),
        max_rays=15 * synth.RAYS)
    # 1.25 cm cells: the 6 m world spans 480 cells of a 512-cell submap, so the match's window is beyond the 152 KiB a workgroup may
    # stage and the scoring reads the submap directly
    add("direct_window", two, dict(stride=20, submap_cells=512, nx=2, ny=2, ntheta=2), _window_beyond_lds, mpc=FINE_MPC, cpm=FINE_CPM)
    _cases = {c.name: c for c in out}
    return _cases


def _tie_history(partners):
    """80 scans; q = 79 recorded at (0, 0) and every j of `partners` at 0.25 m from it along an axis: d2 = 0.0625 exactly for each, every
    other older scan on the circle, about 0.5 m away."""
    scans, poses = history(80, 16)
    _set_pose(poses, 79, 0.0, 0.0)
    for j, (x, y) in zip(partners, ((0.25, 0.0), (-0.25, 0.0), (0.0, 0.25))):
        _set_pose(poses, j, x, y)
    return scans, poses


def _tie(partners):
    """one candidate, the lowest of `partners`; they share the minimum of d2 exactly and every other j is farther"""
    def reaches(m):
        if len(m) != 1 or m[0]["q"] != 79 or len(m[0]["d2"]) < 71:
            return False
        d2 = m[0]["d2"]
        low = min(d2)
        return m[0]["j"] == min(partners) and low == 0.0625 and [j for j, v in enumerate(d2) if v == low] == sorted(partners)
    return reaches


LONG_N, LONG_LAP, LONG_RAYS, LONG_BIAS = 1100, 800, 24, 0.00002
LONG_SAMPLE_KEPT = 16


def _long_log(n, stride):
    """more than 1024 queries and more than 256 candidates, on both sides of query index 1024 and of candidate 256, kept ones on both
    sides; n scans and the stride are the case's own"""
    def reaches(m):
        queries = -(-n // stride)
        qi = [c["q"] // stride for c in m]                     # the query's index: the thread of k_lc_number that numbers it
        return (queries >= 1025 and len(m) >= 257 and any(v <= 1023 for v in qi) and any(v >= 1024 for v in qi) and
                any(c["flags"] == 0 for c in m[:256]) and any(c["flags"] == 0 for c in m[256:]))
    return reaches


_edge_cases = None


def edge_cases():
    """The limits cases() does not reach: kept apart from cases(), whose GPU test compares every candidate with two
    synchronous calls."""
    global _edge_cases
    if _edge_cases is not None:
        return _edge_cases
    out = []

    def add(name, hist, params, reaches, **kw):
        out.append(Case(name, list(hist[0]), list(hist[1]), params, reaches, **kw))

    # a lap of 800 scans of 24 rays and a gap of 700: the queries from 734 on have a partner, the first of the lap before
    long_params = dict(stride=1, min_gap=700, radius=0.25, w=1, submap_cells=64, nx=2, ny=2, ntheta=2)
    long_hist = history(LONG_N, LONG_LAP, rays=LONG_RAYS, bias=LONG_BIAS)
    add("long_log", long_hist, long_params, _long_log(len(long_hist[0]), long_params["stride"]), max_rays=LONG_RAYS)
    tie = dict(stride=79, radius=0.375, submap_cells=65)
    add("tie_same_lane", _tie_history((6, 70)), tie, _tie((6, 70)))                # one lane, two trips: the lane's own strict <
    add("tie_lane_order", _tie_history((3, 64)), tie, _tie((3, 64)))               # lane 3 holds j = 3, lane 0 holds j = 64: the shuffle's oj < bj
    add("tie_three", _tie_history((5, 64, 69)), tie, _tie((5, 64, 69)))
    _edge_cases = {c.name: c for c in out}
    assert not set(_edge_cases) & set(cases())
    return _edge_cases


# a second find on a handle that has just run a larger one, with other parameters
SECOND_FIND = ("two_lap", "equal_d2")
SECOND_FIND_LONG = ("long_log", "equal_d2")

_models = {}


def model(name):
    if name not in _models:
        c = cases()[name] if name in cases() else edge_cases()[name]
        scans, poses = c.retained()
        _models[name] = lcm.find(oracle_lib.load_oracle(), scans, poses, c.mpc, c.cpm, **c.params)
    return _models[name]
