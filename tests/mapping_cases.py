"""Hand-built inputs for Mapping::updateMap (bl_mapping.hip, k_map_update) and the conditions that prove, on the CPU, that each input
reaches the form of the kernel it is meant for.  TEST INFRASTRUCTURE, no GPU: tests/test_gpu_mapping_edges.py runs the cases on the
device, tests/test_mapping_cases_cpu.py runs the conditions alone.

A case is a start grid, the mapper's parameters and a few (scan, pose) updates; the first update only latches the pose.  evaluate()
runs the CPU oracle over it, keeps the grid after every update and the rays' cells (rb_slam_model.ray_cells on the oracle's moving
scan), and calls the case's condition, which raises when the input misses its path.  Scans are arrays written by hand or found by
a seeded search over the oracle's own float32 arithmetic: no world is ray-cast.

What the conditions restate of the kernel: a scan keeps the entries with range > 0.15f (the host); up to SEG_RAYS kept rays take the
segment walk, more the serial walk; the window is the box of all start and end cells of the rays with range <= max_laser, clipped to
the grid, widened to whole dwords when width % 4 == 0 and the walk is the segment walk (then the window pass is the dword pass,
otherwise the byte pass); a window of more than LDS_COUNTERS cells is cut into strips of LDS_COUNTERS // ww rows."""
import math

import numpy as np

import oracle_lib
import rb_slam_model as rbm
from botlab_amd.host import LidarScan

LDS_COUNTERS = 72 * 1024            # MAP_LDS_COUNTERS
SEG_RAYS = 1024                     # MAP_SEG_RAYS
MAX_RAYS = 8192                     # MAP_MAX_RAYS
SEG = 16                            # MAP_SEG
MIN_RANGE = np.float32(0.15)        # moving_laser_scan.cpp:24


class Case:
    def __init__(self, name, width, height, mpc, max_laser, hit, miss, start, updates, condition, origin=None):
        self.name = name
        self.width, self.height = int(width), int(height)
        self.mpc = np.float32(mpc)
        self.cpm = np.float32(1.0) / self.mpc                  # OccupancyGrid.from_cells
        self.origin = origin if origin is not None else (np.float32(-0.5 * width * float(self.mpc)), np.float32(-0.5 * height * float(self.mpc)))
        self.max_laser, self.hit, self.miss = float(max_laser), int(hit), int(miss)
        self.start = np.ascontiguousarray(start, np.int8)
        assert self.start.shape == (self.height, self.width)
        self.updates = updates                                  # [(LidarScan, (x, y, theta, utime)), ...]
        self.condition = condition                              # condition(case, refs, geo) raises AssertionError

    def centre_of(self, cx, cy):
        """Global coordinates of the point (cx, cy) in cell units."""
        return (float(self.origin[0]) + cx * float(self.mpc), float(self.origin[1]) + cy * float(self.mpc))


def kept(scan):
    return int((scan.ranges > MIN_RANGE).sum())


def geometry(orc, scan, begin, end, case):
    """The traced rays of one update: int cells (n, 4) = rb_slam_model.ray_cells, and the float end points fx, fy they are truncated
    from (mapping.cpp:45-49 in float32)."""
    cells = rbm.ray_cells(orc, scan, begin, end, case.origin, case.cpm, case.max_laser)
    rays = orc.moving_scan(scan, begin, end)
    rays = rays[rays[:, 2] <= np.float32(case.max_laser)]
    cpm = case.cpm
    sx = ((rays[:, 0].astype(np.float64) - np.float64(np.float32(case.origin[0]))) * np.float64(cpm)).astype(np.float32)
    sy = ((rays[:, 1].astype(np.float64) - np.float64(np.float32(case.origin[1]))) * np.float64(cpm)).astype(np.float32)
    fx = (rays[:, 2] * np.cos(rays[:, 3]).astype(np.float32) * cpm + sx).astype(np.float32)
    fy = (rays[:, 2] * np.sin(rays[:, 3]).astype(np.float32) * cpm + sy).astype(np.float32)
    assert np.array_equal(np.stack([np.trunc(sx), np.trunc(sy), np.trunc(fx), np.trunc(fy)], axis=1).astype(np.int64), cells)
    return dict(cells=cells, sx=sx, sy=sy, fx=fx, fy=fy, kept=kept(scan))


def walk(x, y, x2, y2):
    """Mapping::bresenham (mapping.cpp:101-127): the cells it visits, start included, end excluded."""
    dx, dy = abs(x2 - x), abs(y2 - y)
    sx, sy = (1 if x < x2 else -1), (1 if y < y2 else -1)
    err = dx - dy
    out = []
    while x != x2 or y != y2:
        out.append((x, y))
        e2 = 2 * err
        if e2 >= -dy:
            err -= dy; x += sx
        if e2 <= dx:
            err += dx; y += sy
    return out


def segment_cells(x0, y0, x1, y1, k0):
    """k_map_update's segment that starts at step k0 (a multiple of SEG) of the ray's walk: its cells, by the kernel's integer
    arithmetic (num, n, rem and the per-cell step), transcribed line by line."""
    dx, dy = abs(x1 - x0), abs(y1 - y0)
    sx, sy = (1 if x0 < x1 else -1), (1 if y0 < y1 else -1)
    K = max(dx, dy)
    k1 = min(K, k0 + SEG)
    xmajor = dx >= dy
    dmaj, dmin = (dx, dy) if xmajor else (dy, dx)
    if k0 >= k1:
        return []
    num = 2 * k0 * dmin + dmaj
    n = num // (2 * dmaj)
    rem = num - n * 2 * dmaj
    out = []
    for k in range(k0, k1):
        out.append((x0 + sx * k, y0 + sy * n) if xmajor else (x0 + sx * n, y0 + sy * k))
        rem += 2 * dmin
        if rem >= 2 * dmaj:
            rem -= 2 * dmaj; n += 1
    return out


def window(case, g):
    """(x0, y0, x1, y1) of the kernel's window before the dword alignment, (ww, wh) after it, the rows of a strip and whether the
    window pass is the dword pass; None when no traced cell lies in the grid."""
    c = g["cells"]
    if len(c) == 0:
        return None
    x0, x1 = max(int(min(c[:, 0].min(), c[:, 2].min())), 0), min(int(max(c[:, 0].max(), c[:, 2].max())), case.width - 1)
    y0, y1 = max(int(min(c[:, 1].min(), c[:, 3].min())), 0), min(int(max(c[:, 1].max(), c[:, 3].max())), case.height - 1)
    if x1 < x0 or y1 < y0:
        return None
    dword = case.width % 4 == 0 and g["kept"] <= SEG_RAYS
    ax0, ax1 = (x0 & ~3, x1 | 3) if dword else (x0, x1)
    ww, wh = ax1 - ax0 + 1, y1 - y0 + 1
    return dict(raw=(x0, y0, x1, y1), ax0=ax0, ww=ww, wh=wh, cells=ww * wh, dword=dword, rows_per_strip=max(1, min(LDS_COUNTERS // ww, wh)))


_results = {}


def evaluate(case, orc):
    """(refs, geo): the oracle's grid after every update and the traced rays of every update but the first; the case's condition has
    been checked.  Computed once per case name."""
    if case.name in _results:
        return _results[case.name]
    om = oracle_lib.OracleMapping(orc, case.max_laser, case.hit, case.miss)
    ref = case.start.copy()
    refs, geo, prev = [], [], None
    for scan, p in case.updates:
        pose = orc.pose(p[0], p[1], p[2], utime=p[3])
        geo.append(None if prev is None else geometry(orc, scan, prev, pose, case))
        om.update(scan, pose, ref, case.mpc, case.cpm, case.origin)
        refs.append(ref.copy())
        prev = pose
    assert len(case.updates) >= 2 and np.array_equal(refs[0], case.start)
    case.condition(case, refs, geo)
    for r in refs:
        r.setflags(write=False)
    _results[case.name] = (refs, geo)
    return refs, geo


# ------------------------------------------------------------------ builders
def _times(n, t0, t1):
    """n ray stamps spread over (t0, t1], the last one t1."""
    return (t0 + ((np.arange(n, dtype=np.int64) + 1) * (t1 - t0)) // n).astype(np.int64)


def _scan(ranges, dirs, t0, t1, times=None):
    """dirs: the directions the rays leave in for a robot heading 0 (the ray's angle is pose.theta - scan.theta)."""
    n = len(ranges)
    return LidarScan(np.asarray(ranges, np.float32), (-np.asarray(dirs, np.float64)).astype(np.float32), _times(n, t0, t1) if times is None else times,
                     utime=t1)


def _updates(scans_of, poses, t0=1_000_000, dt=100_000):
    out = []
    for k, p in enumerate(poses):
        t1 = t0 + k * dt
        out.append((scans_of(k, t1 - dt, t1), (p[0], p[1], p[2], t1)))
    return out


def _changed(refs, start):
    ch = np.zeros(start.shape, bool)
    prev = start
    for r in refs:
        ch |= r != prev
        prev = r
    return ch


# ---- 1: byte window pass, one strip
def byte_one_strip(orc, hit, miss):
    rng = np.random.default_rng(101)
    W, H = 203, 197
    start = rng.integers(-128, 128, (H, W)).astype(np.int8)
    poses = [(-1.5, 1.0, 0.2), (-1.4, 1.1, 0.3), (-1.35, 1.15, 0.35), (1.5, 1.0, -0.4), (1.55, 0.9, -0.5)]

    def scans_of(k, t0, t1):
        r = rng.uniform(0.2, 5.4, 290)
        r[::5] = rng.uniform(4.0, 5.0, 58)
        return _scan(r, np.arange(290) * (2 * math.pi / 290), t0, t1)

    def condition(case, refs, geo):
        assert case.width % 4 != 0
        for g in geo[1:]:
            w = window(case, g)
            assert not w["dword"] and w["cells"] <= LDS_COUNTERS and w["rows_per_strip"] == w["wh"] and g["kept"] <= SEG_RAYS
        ch = _changed(refs, case.start)
        assert ch[:, 0].any() and ch[:, W - 1].any() and ch[H - 1, :].any()

    return Case(f"byte_one_strip_{hit}_{miss}", W, H, 0.05, 5.0, hit, miss, start, _updates(scans_of, poses), condition)


# ---- 2, 3, 4: strips
def _circle_scan(n_circle, n_edge, edge_rows, centre, t0, t1):
    """n_circle rays around the whole circle, ranges in 6 .. 8 m, no further than 7.3 m along x (the window then ends inside the
    grid on both sides); n_edge rays of 7 m whose end rows step by a fifth of a cell over edge_rows +- 4."""
    d = np.arange(n_circle) * (2 * math.pi / n_circle)
    r = np.clip(7.3 / np.maximum(np.abs(np.cos(d)), 1e-9), 6.0, 8.0)
    if n_edge:
        rows = edge_rows + np.linspace(-4.0, 4.0, n_edge)
        de = np.arcsin((rows - centre[1]) / 140.0)
        d, r = np.concatenate([d, de]), np.concatenate([r, np.full(n_edge, 7.0)])
    return _scan(r, d, t0, t1)


def strips(orc, W, H, rays):
    rng = np.random.default_rng(202)
    start = rng.integers(-128, 128, (H, W)).astype(np.int8)
    poses = [(0.0, 0.0, 0.0), (0.004, 0.003, 0.002), (0.008, 0.001, 0.004), (0.011, -0.002, 0.001)]
    centre = (W / 2.0, H / 2.0)
    name = f"strips_{W}x{H}_{rays}"
    probe = Case(name + "_probe", W, H, 0.05, 8.0, 4, 1, start, None, None)
    t = 1_000_000
    g0 = geometry(orc, _circle_scan(rays - 40, 0, 0.0, centre, t, t + 1), orc.pose(0, 0, 0, utime=t), orc.pose(0, 0, 0, utime=t + 1), probe)
    g0["kept"] = rays
    w0 = window(probe, g0)
    edge = w0["raw"][1] + w0["rows_per_strip"]                  # the border between the first and the second strip, in rows

    def scans_of(k, t0, t1):
        return _circle_scan(rays - 40, 40, float(edge), centre, t0, t1)

    def condition(case, refs, geo):
        for g in geo[1:]:
            w = window(case, g)
            assert g["kept"] == rays and w["cells"] > LDS_COUNTERS and w["rows_per_strip"] < w["wh"]
            assert w["dword"] == (W % 4 == 0 and rays <= SEG_RAYS)
            if W % 4 == 0:
                assert w["raw"][0] % 4 != 0 and (w["raw"][2] + 1) % 4 != 0
            last_of_first = w["raw"][1] + w["rows_per_strip"] - 1
            c = g["cells"]
            inx = (c[:, 2] >= w["raw"][0]) & (c[:, 2] <= w["raw"][2])
            assert (inx & (c[:, 3] == last_of_first)).any() and (inx & (c[:, 3] == last_of_first + 1)).any()
        assert (_changed(refs, case.start).sum()) > 10000

    return Case(name, W, H, 0.05, 8.0, 4, 1, start, _updates(scans_of, poses), condition)


# ---- 5: ray counts
def ray_count(orc, n_kept, extra):
    rng = np.random.default_rng(500 + n_kept)
    W = H = 200
    start = rng.integers(-128, 128, (H, W)).astype(np.int8)
    poses = [(0.3, -0.2, 0.1), (0.33, -0.18, 0.15), (0.36, -0.15, 0.2)] + ([(0.4, -0.1, 0.3)] if n_kept < MAX_RAYS else [])
    total = n_kept + extra
    assert total <= MAX_RAYS

    def scans_of(k, t0, t1):
        r = rng.uniform(0.2, 5.4, total).astype(np.float32)
        drop = rng.permutation(total)[:extra]
        r[drop[0::2]] = np.float32(0.1)
        r[drop[1::2]] = MIN_RANGE                                # exactly 0.15f: not kept
        return _scan(r, rng.uniform(-math.pi, math.pi, total), t0, t1)

    def condition(case, refs, geo):
        for (scan, _), g in zip(case.updates[1:], geo[1:]):
            assert scan.num_ranges == total and int((scan.ranges > np.float32(0.15)).sum()) == n_kept == g["kept"]
            assert 0 < len(g["cells"]) <= n_kept
        assert not np.array_equal(refs[-1], case.start)

    return Case(f"ray_count_{n_kept}_of_{total}", W, H, 0.05, 5.0, 4, 1, start, _updates(scans_of, poses), condition)


def all_beyond_max(orc):
    rng = np.random.default_rng(510)
    start = rng.integers(-128, 128, (200, 200)).astype(np.int8)
    poses = [(0.0, 0.0, 0.0), (0.05, 0.0, 0.1), (0.1, 0.0, 0.2)]

    def scans_of(k, t0, t1):
        return _scan(rng.uniform(5.001, 9.0, 300), rng.uniform(-math.pi, math.pi, 300), t0, t1)

    def condition(case, refs, geo):
        for g in geo[1:]:
            assert g["kept"] == 300 and len(g["cells"]) == 0
        for r in refs:
            assert np.array_equal(r, case.start)

    return Case("all_beyond_max", 200, 200, 0.05, 5.0, 4, 1, start, _updates(scans_of, poses), condition)


def nan_and_inf(orc):
    rng = np.random.default_rng(520)
    start = rng.integers(-128, 128, (200, 200)).astype(np.int8)
    poses = [(0.0, 0.0, 0.0), (0.05, 0.0, 0.1), (0.1, 0.0, 0.2), (0.15, 0.02, 0.3)]
    n = 290

    def scans_of(k, t0, t1):
        r = rng.uniform(0.2, 4.9, n).astype(np.float32)
        r[3::17] = np.float32(np.nan)
        r[5::19] = np.float32(np.inf)
        r[0] = np.float32(np.nan)
        r[n - 1] = np.float32(np.inf)
        return _scan(r, np.arange(n) * (2 * math.pi / n), t0, t1)

    def condition(case, refs, geo):
        prev = None
        for (scan, p), g in zip(case.updates, geo):
            pose = orc.pose(p[0], p[1], p[2], utime=p[3])
            if prev is not None:
                nan, inf = np.isnan(scan.ranges), np.isinf(scan.ranges)
                assert nan.sum() > 10 and inf.sum() > 10
                ms = orc.moving_scan(scan, prev, pose)
                assert len(ms) == int((~nan).sum()) and not np.isnan(ms[:, 2]).any()            # NaN > 0.15f is false
                assert len(g["cells"]) == int((~nan & ~inf).sum())                               # inf <= max_laser is false
            prev = pose
        assert not np.array_equal(refs[-1], case.start)

    return Case("nan_and_inf", 200, 200, 0.05, 5.0, 4, 1, start, _updates(scans_of, poses), condition)


# ---- 6: counter halves and saturation
SATURATION_VALUES = np.array([-128, -127, -1, 0, 1, 126, 127], np.int8)
SATURATION_ODDS = [(127, 127), (127, 0), (0, 127), (0, 0), (1, 1), (4, 1)]


def counters(orc, form, hit, miss, shift):
    """form: "pair" (600 rays, 300 into each of two neighbouring cells of one counter dword), "one" (1024 rays into one cell),
    "serial" (1100 rays, 550 into each of the two cells).  shift moves the pattern of start values by one cell."""
    W = H = 64
    yy, xx = np.mgrid[0:H, 0:W]
    start = SATURATION_VALUES[(xx + 3 * yy + shift) % 7]
    name = f"counters_{form}_{hit}_{miss}_{shift}"
    case = Case(name, W, H, 0.05, 5.0, hit, miss, start, None, None)
    x, y = case.centre_of(32.5, 32.5)
    n_a, n_b = {"pair": (300, 300), "one": (1024, 0), "serial": (550, 550)}[form]
    r = np.concatenate([np.full(n_a, 0.4), np.full(n_b, 0.45)])             # ends at the centres of cells (40, 32) and (41, 32)
    if form != "one":
        r = r.reshape(2, -1).T.ravel()                                       # alternate the two
    poses = [(x, y, 0.0)] * 4

    def scans_of(k, t0, t1):
        return _scan(r, np.zeros(len(r)), t0, t1)

    def condition(case, refs, geo):
        for g in geo[1:]:
            c = g["cells"]
            assert len(c) == n_a + n_b == g["kept"] and (c[:, 0] == 32).all() and (c[:, 1] == 32).all()
            ends, H_ = np.unique(c[:, 2:], axis=0, return_counts=True)
            w = window(case, g)
            par = (ends[:, 0] - w["ax0"]) & 1                                # the half of the counter dword: the window's rows are even
            assert w["ww"] % 2 == 0 or w["wh"] == 1
            crossed = set()
            for e in ends:
                crossed |= set(walk(32, 32, int(e[0]), int(e[1])))
            if form == "one":
                assert len(ends) == 1 and H_[0] == 1024
            else:
                assert len(ends) == 2 and ends[0][1] == ends[1][1] and abs(ends[0][0] - ends[1][0]) == 1
                assert (ends[:, 0] - w["ax0"]).min() // 2 == (ends[:, 0] - w["ax0"]).max() // 2          # one counter dword
                assert H_[par == 0].max() >= 300 and H_[par == 1].max() >= 300
                assert any((int(e[0]), int(e[1])) in crossed for e in ends)                               # M > 0 in an end cell
            touched = np.array(sorted(crossed | {(int(e[0]), int(e[1])) for e in ends}))
            assert set(case.start[touched[:, 1], touched[:, 0]].tolist()) == set(SATURATION_VALUES.tolist())

    case.updates, case.condition = _updates(scans_of, poses), condition
    return case


# ---- 7: walk fan
FAN_DMAJ = [15, 16, 17, 31, 32, 33, 47, 48, 49]


def fan_targets(dmajs):
    t = set()
    for dmaj in dmajs:
        for dmin in {0, 1, dmaj // 2, dmaj - 1, dmaj}:
            if 0 <= dmin <= dmaj:
                for s1 in (1, -1):
                    for s2 in (1, -1):
                        t.add((s1 * dmaj, s2 * dmin)); t.add((s2 * dmin, s1 * dmaj))
    return sorted(t)


def _aim(orc, case, robot_cell, targets, seed):
    """Ranges and directions, found by a seeded search, of rays from the centre of robot_cell whose integer (dx, dy) are `targets` in
    the oracle's own arithmetic: first aimed at the centre of the end cell, then at seeded points inside it."""
    rng = np.random.default_rng(seed)
    x, y = case.centre_of(robot_cell[0] + 0.5, robot_cell[1] + 0.5)
    targets = np.asarray(targets, np.float64).reshape(-1, 2)
    off = np.zeros_like(targets)
    zero = (targets == 0).all(axis=1)                            # start cell = end cell: one ray into each quadrant of the cell
    off[zero] = np.array([[0.23 * (1 - 2 * (i & 1)), 0.23 * (1 - (i & 2))] for i in range(int(zero.sum()))], np.float64).reshape(-1, 2)
    t = 1_000_000
    b, e = orc.pose(x, y, 0.0, utime=t), orc.pose(x, y, 0.0, utime=t + 1)
    for _ in range(60):
        v = targets + off
        r = np.hypot(v[:, 0], v[:, 1]) * float(case.mpc)
        d = np.arctan2(v[:, 1], v[:, 0])
        g = geometry(orc, _scan(r, d, t, t + 1), b, e, case)
        assert len(g["cells"]) == len(targets), "a ray of the fan is too short or too long to be traced"
        got = g["cells"][:, 2:] - g["cells"][:, :2]
        bad = (got != targets).any(axis=1) | (g["cells"][:, 0] != robot_cell[0]) | (g["cells"][:, 1] != robot_cell[1])
        if not bad.any():
            return r, d, (x, y)
        off[bad] = rng.uniform(-0.3, 0.3, (int(bad.sum()), 2))
    raise AssertionError("no rays found for " + str(targets[bad].tolist()))


def _fan_case(orc, name, W, H, mpc, max_laser, robot_cell, targets, seed, repeat=1, start_seed=700):
    rng = np.random.default_rng(start_seed)
    start = rng.integers(-128, 128, (H, W)).astype(np.int8)
    case = Case(name, W, H, mpc, max_laser, 4, 1, start, None, None)
    r, d, (x, y) = _aim(orc, case, robot_cell, targets, seed)
    r, d = np.tile(r, repeat), np.tile(d, repeat)
    want = {(int(a), int(b)) for a, b in targets}

    def scans_of(k, t0, t1):
        return _scan(r, d, t0, t1)

    def condition(case, refs, geo):
        for g in geo[1:]:
            c = g["cells"]
            assert (g["kept"] > SEG_RAYS) == (repeat > 1) and len(c) == g["kept"]
            got = {(int(a), int(b)) for a, b in (c[:, 2:] - c[:, :2])}
            assert want <= got, sorted(want - got)
            assert (c >= 0).all() and (c[:, [0, 2]] < W).all() and (c[:, [1, 3]] < H).all()          # the whole walk is counted
        assert not np.array_equal(refs[-1], refs[-2])

    case.updates, case.condition = _updates(scans_of, [(x, y, 0.0)] * 3), condition
    return case


def fan(orc, serial=False):
    t = fan_targets(FAN_DMAJ)
    return _fan_case(orc, "fan_serial" if serial else "fan", 128, 128, 0.05, 5.0, (64, 64), t, 71, repeat=4 if serial else 1)


def fan_short(orc, serial=False):
    """K = 0 and K = 1: a kept ray is longer than 0.15 m, three cells of 5 cm, so these need a coarser grid (cells of 0.5 m)."""
    t = [(0, 0)] * 4 + [t for t in fan_targets([1]) if t != (0, 0)] + fan_targets([2, 3])
    return _fan_case(orc, "fan_short_serial" if serial else "fan_short", 32, 32, 0.5, 5.0, (16, 16), t, 72, repeat=30 if serial else 1)


def fan_thin(orc, side):
    sgn = 1 if side == "left" else -1
    t = [(sgn * dmaj, dmin) for dmaj in (800, 801, 815, 816, 817, 850, 895) for dmin in (0, 1, -1, 2, -2)]
    cell = (20, 32) if side == "left" else (1679, 32)
    return _fan_case(orc, "fan_thin_" + side, 1700, 64, 0.01, 9.0, cell, t, 73)


# ---- 8: the edges of the frame
def _edge_scan(rng, t0, t1, long_dirs=()):
    n = 290
    d = np.arange(n) * (2 * math.pi / n)
    d[:8] = [0.0, math.pi / 2, math.pi, -math.pi / 2, math.pi / 4, 3 * math.pi / 4, -math.pi / 4, -3 * math.pi / 4]
    r = rng.uniform(0.2, 2.5, n)
    for i, ld in enumerate(long_dirs):
        d[20 + i], r[20 + i] = ld, 4.0 + 0.1 * i
    times = _times(n, t0, t1)
    times[::2] = t1                                              # half of the rays leave from the pose itself
    return _scan(r, d, t0, t1, times=times)


def edges_inside(orc):
    rng = np.random.default_rng(800)
    start = rng.integers(-128, 128, (40, 40)).astype(np.int8)
    poses = [(-0.99, 0.0, 0.0), (-0.99, 0.05, 0.3), (0.99, 0.0, 1.0), (0.05, -0.99, 2.0), (0.0, 0.99, -1.0)]

    def scans_of(k, t0, t1):
        return _edge_scan(rng, t0, t1)

    def condition(case, refs, geo):
        border = {1: (0, 0), 2: (0, 39), 3: (1, 0), 4: (1, 39)}
        for k, (axis, cell) in border.items():
            g = geo[k]
            assert len(g["cells"]) == 290
            at = (g["sx"], g["sy"])[axis][::2]                   # the rays stamped with the pose's utime
            assert (np.trunc(at) == cell).all() and (np.abs(at - (cell + 0.5)) < 0.5).all()
            assert not np.array_equal(refs[k], refs[k - 1])

    return Case("edges_inside", 40, 40, 0.05, 5.0, 4, 1, start, _updates(scans_of, poses), condition)


def edges_outside(orc):
    rng = np.random.default_rng(810)
    start = rng.integers(-128, 128, (40, 40)).astype(np.int8)
    # 0.3 cell outside on the negative x side, then on the negative y side, then far outside: rays cross the whole grid
    poses = [(-1.015, 0.3, 0.0), (-1.015, 0.3, 0.2), (0.3, -1.015, 0.1), (-1.5, 0.0, 0.0), (0.0, -1.5, 0.0)]

    def scans_of(k, t0, t1):
        return _edge_scan(rng, t0, t1, long_dirs=(0.0, 0.1, -0.1, math.pi / 2, math.pi / 2 + 0.1))

    def condition(case, refs, geo):
        neg_start = neg_end = through = False
        for g in geo[1:]:
            c = g["cells"]
            neg_start |= bool((((g["sx"] < 0) & (g["sx"] > -1) & (c[:, 0] == 0)) | ((g["sy"] < 0) & (g["sy"] > -1) & (c[:, 1] == 0))).any())
            ingrid = (c[:, 2] >= 0) & (c[:, 2] < 40) & (c[:, 3] >= 0) & (c[:, 3] < 40)
            neg_end |= bool((ingrid & (((g["fx"] < 0) & (c[:, 2] == 0)) | ((g["fy"] < 0) & (c[:, 3] == 0)))).any())
            for q in c:
                out0 = not (0 <= q[0] < 40 and 0 <= q[1] < 40)
                out1 = not (0 <= q[2] < 40 and 0 <= q[3] < 40)
                if out0 and out1 and sum(0 <= x < 40 and 0 <= y < 40 for x, y in walk(*[int(v) for v in q])) >= 40:
                    through = True
        assert neg_start and neg_end and through
        for k in (1, 2, 3, 4):
            assert not np.array_equal(refs[k], refs[k - 1])

    return Case("edges_outside", 40, 40, 0.05, 5.0, 4, 1, start, _updates(scans_of, poses), condition)


# ---- 9: stamps
def stamps(orc):
    rng = np.random.default_rng(900)
    start = rng.integers(-128, 128, (200, 200)).astype(np.int8)
    n = 290
    T0, DT = 1_000_000, 100_000
    # the first three poses share one utime (no interpolation, the map is updated); then stamps outside [t_begin, pose.utime]
    poses = [(0.0, 0.0, 0.0, T0), (0.3, 0.1, 0.5, T0), (0.1, 0.4, -0.3, T0), (0.4, 0.4, 0.2, T0 + DT), (0.1, 0.4, 0.7, T0 + 2 * DT)]
    updates = []
    for k, p in enumerate(poses):
        r = rng.uniform(0.2, 5.3, n)
        d = np.arange(n) * (2 * math.pi / n)
        lo, hi = p[3] - DT, p[3]
        times = np.linspace(lo - 0.6 * DT, hi + 0.6 * DT, n).astype(np.int64) if k >= 3 else _times(n, lo, hi)
        updates.append((_scan(r, d, lo, hi, times=times), p))

    def condition(case, refs, geo):
        assert poses[1][3] == poses[0][3] == poses[2][3]
        for k in (1, 2):
            assert not np.array_equal(refs[k], refs[k - 1])
            g = geo[k]                                           # equal utimes: every ray leaves from the pose itself
            cx, cy = (poses[k][0] - float(case.origin[0])) * 20.0, (poses[k][1] - float(case.origin[1])) * 20.0
            assert (np.abs(g["sx"] - cx) < 1e-3).all() and (np.abs(g["sy"] - cy) < 1e-3).all()
        for k in (3, 4):
            scan, p = updates[k]
            b, e = orc.pose(*poses[k - 1][:3], utime=poses[k - 1][3]), orc.pose(*p[:3], utime=p[3])
            assert (scan.times < b.utime).sum() > 20 and (scan.times > e.utime).sum() > 20
            clamped = LidarScan(scan.ranges, scan.thetas, np.clip(scan.times, b.utime, e.utime), utime=scan.utime)
            other = geometry(orc, clamped, b, e, case)["cells"]
            outside = ((scan.times < b.utime) | (scan.times > e.utime))[(scan.ranges > MIN_RANGE) & (scan.ranges <= np.float32(case.max_laser))]
            differ = (other != geo[k]["cells"]).any(axis=1)
            assert (differ & outside).sum() > 20 and not (differ & ~outside).any()
            assert not np.array_equal(refs[k], refs[k - 1])

    return Case("stamps", 200, 200, 0.05, 5.0, 4, 1, start, updates, condition)


# ---- 10: long and thin: a walk that starts behind dmaj = 32768
LONG_DMAJ = (32768, 32780)
LONG_DMIN = (0, 1, 3, 7)


def long_thin(orc):
    """A grid of 32 800 x 8 cells, eight rays from near one short edge almost along the long axis: the smallest shape in which a
    segment starts at k0 > 0 of a walk with dmaj >= 32768, where the start's division takes 64 bits (bl_mapray_dev.h)."""
    case = _fan_case(orc, "long_thin", 32800, 8, 0.05, 1700.0, (10, 0), [(a, b) for a in LONG_DMAJ for b in LONG_DMIN], 74)
    fan_condition = case.condition

    def condition(case, refs, geo):
        fan_condition(case, refs, geo)                          # the rays have exactly these (dx, dy) and end inside the grid
        for g in geo[1:]:
            c = g["cells"]
            assert (np.maximum(np.abs(c[:, 2] - c[:, 0]), np.abs(c[:, 3] - c[:, 1])) >= 32768).any() and g["kept"] <= SEG_RAYS

    case.condition = condition
    return case


# ---- 11: a start far outside the grid: coordinates past 2^23, a start of the walk whose numerator passes 2^32
FAR_CELL = (-8_500_000, -1_000_000)
FAR_REACH = 200                              # every grid cell of a far ray lies within this many steps of its end


def far_numerators(cells):
    """2 k dmin + dmaj at k = dmaj - FAR_REACH for rays (n, 4): what the walk's first division takes in where the rays reach the grid."""
    dx, dy = np.abs(cells[:, 2] - cells[:, 0]), np.abs(cells[:, 3] - cells[:, 1])
    dmaj, dmin = np.maximum(dx, dy), np.minimum(dx, dy)
    return 2 * (dmaj - FAR_REACH) * dmin + dmaj


def far_start(orc):
    """A standing robot 8.5 million cells from a grid of 64 x 64, eight rays that end in the grid.  Their start cells lie between 2^23
    and 2^24 (BL_RAY_CELL_LIMIT is 2^24, not less), and where they reach the grid the numerator 2 k dmin + dmaj of the walk's start is
    past 2^32 (the division must be the 64-bit one there)."""
    rng = np.random.default_rng(1100)
    W = H = 64
    start = rng.integers(-128, 128, (H, W)).astype(np.int8)
    case = Case("far_start", W, H, 0.05, 1.0e6, 4, 1, start, None, None)
    x, y = case.centre_of(FAR_CELL[0] + 0.5, FAR_CELL[1] + 0.5)
    v = np.array([(8.5 + 6 * i - FAR_CELL[0], 5.5 + 7 * i - FAR_CELL[1]) for i in range(8)], np.float64)
    r, d = np.hypot(v[:, 0], v[:, 1]) * 0.05, np.arctan2(v[:, 1], v[:, 0])

    def condition(case, refs, geo):
        for g in geo[1:]:
            c = g["cells"]
            assert len(c) == 8 == g["kept"]
            assert (np.abs(c[:, 0]) > 1 << 23).all() and (np.abs(c) < 1 << 24).all()
            assert (c[:, 2:] > 64 - FAR_REACH).all() and (c[:, 2:] < FAR_REACH).all() and (far_numerators(c) >= 1 << 32).all()
        assert (refs[-1] != refs[-2]).sum() > 100

    case.updates, case.condition = _updates(lambda k, t0, t1: _scan(r, d, t0, t1), [(x, y, 0.0)] * 3), condition
    return case


# ------------------------------------------------------------------ the list
RAY_COUNTS = [(1, 37), (64, 0), (65, 37), (1023, 0), (1024, 37), (1025, 0), (2048, 37), (2049, 0), (8192, 0)]

BUILDERS = {}
for _h, _m in [(4, 1), (60, 45)]:
    BUILDERS[f"byte_one_strip_{_h}_{_m}"] = (lambda orc, h=_h, m=_m: byte_one_strip(orc, h, m))
for _w, _hh, _r in [(301, 301, 400), (304, 300, 400), (304, 300, 1500), (301, 301, 1500)]:
    BUILDERS[f"strips_{_w}x{_hh}_{_r}"] = (lambda orc, w=_w, h=_hh, r=_r: strips(orc, w, h, r))
for _k, _e in RAY_COUNTS:
    BUILDERS[f"ray_count_{_k}_of_{_k + _e}"] = (lambda orc, k=_k, e=_e: ray_count(orc, k, e))
BUILDERS["all_beyond_max"] = all_beyond_max
BUILDERS["nan_and_inf"] = nan_and_inf
BUILDERS["fan"] = fan
BUILDERS["fan_serial"] = lambda orc: fan(orc, serial=True)
BUILDERS["fan_short"] = fan_short
BUILDERS["fan_short_serial"] = lambda orc: fan_short(orc, serial=True)
BUILDERS["fan_thin_left"] = lambda orc: fan_thin(orc, "left")
BUILDERS["fan_thin_right"] = lambda orc: fan_thin(orc, "right")
BUILDERS["edges_inside"] = edges_inside
BUILDERS["edges_outside"] = edges_outside
BUILDERS["stamps"] = stamps
BUILDERS["long_thin"] = long_thin
BUILDERS["far_start"] = far_start

_cases = {}


def get(name, orc):
    if name not in _cases:
        _cases[name] = BUILDERS[name](orc)
        assert _cases[name].name == name
    return _cases[name]
