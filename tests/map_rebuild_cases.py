"""Hand-built inputs for the map rebuild (bl_scanlog_rebuild) and the conditions that show, on the CPU, that each input reaches the path
it is meant for.  TEST INFRASTRUCTURE, no GPU: tests/test_gpu_map_rebuild.py runs the cases on the device,
tests/test_map_rebuild_model_cpu.py runs the model and the conditions alone.

A case is a grid (shape, frame, base cells), the entries of a log (scan, pose), and the arguments of one rebuild: a window of the log,
poses (recorded or others), a previous pose or none, max_laser and the odds.  evaluate() computes, once per case, the definition
(map_rebuild_model.truth: sequential oracle updates), the restated fold (map_rebuild_model.fold) and the sum-then-clamp result, checks
fold == truth, and calls the case's condition with the counts of chunks, pairs and clamped cells.  Scans are arrays written by hand:
no world is ray-cast."""
import math

import numpy as np

import map_rebuild_model as mm
from botlab_amd.host import LidarScan

T0, DT = 1_000_000, 100_000


class Case:
    def __init__(self, name, width, height, mpc, origin, base, entries, max_laser, hit, miss, condition, first=0, count=None, prev=None,
                 poses=None, saturates=False):
        self.name = name
        self.width, self.height = int(width), int(height)
        self.mpc = np.float32(mpc)
        self.cpm = np.float32(1.0) / self.mpc                  # OccupancyGrid.from_cells
        self.origin = (np.float32(origin[0]), np.float32(origin[1]))
        self.base = np.ascontiguousarray(base, np.int8)
        assert self.base.shape == (self.height, self.width)
        self.entries = entries                                  # [(LidarScan, (x, y, theta, utime)), ...]: the log, oldest first
        self.max_laser, self.hit, self.miss = float(max_laser), int(hit), int(miss)
        self.first = int(first)
        self.count = len(entries) - self.first if count is None else int(count)
        self.prev = prev                                        # (x, y, theta, utime) or None
        self.poses = poses                                      # None: the recorded poses of the window
        self.condition = condition                              # condition(case, result) raises AssertionError
        self.saturates = saturates                              # sum-then-clamp must differ from the truth

    def window(self):
        w = self.entries[self.first:self.first + self.count]
        return [s for s, _ in w], (self.poses if self.poses is not None else [p for _, p in w])


_results = {}


def evaluate(case, orc):
    """dict(truth, fold, naive, chunks, pairs, clamped, info) of a case, computed once; fold == truth and the condition are checked."""
    if case.name in _results:
        return _results[case.name]
    scans, poses = case.window()
    args = (scans, poses, case.prev, case.base, case.mpc, case.cpm, case.origin, case.max_laser, case.hit, case.miss)
    truth = mm.truth(orc, *args)
    folded, info = mm.fold(orc, *args)
    assert np.array_equal(folded, truth), f"{case.name}: the chunked fold differs from the sequential oracle in {(folded != truth).sum()} cells"
    nv = mm.naive(case.base, info["per_scan"], case.hit, case.miss)
    res = dict(truth=truth, fold=folded, naive=nv, chunks=info["chunks"], pairs=len(info["pairs"]), clamped=int((nv != truth).sum()), info=info)
    print(f"{case.name}: scans {info['scans']} chunks {res['chunks']} pairs {res['pairs']} tiles {info['tiles']} "
          f"cells where sum-then-clamp differs {res['clamped']} changed {(truth != case.base).sum()}")
    if case.saturates:
        assert res["clamped"] > 0, f"{case.name}: sum-then-clamp gives the truth here, the case cannot tell the two rules apart"
    case.condition(case, res)
    truth.setflags(write=False)
    _results[case.name] = res
    return res


# ------------------------------------------------------------------ builders
def _times(n, t0, t1):
    return (t0 + ((np.arange(n, dtype=np.int64) + 1) * (t1 - t0)) // n).astype(np.int64)


def _scan(ranges, dirs, t0, t1, at_end=False):
    """dirs: the directions the rays leave in for a robot heading 0.  at_end: every ray stamped t1 (it leaves from the pose itself)."""
    n = len(ranges)
    times = np.full(n, t1, np.int64) if at_end else _times(n, t0, t1)
    return LidarScan(np.asarray(ranges, np.float32), (-np.asarray(dirs, np.float64)).astype(np.float32), times, utime=t1)


def _circle(rng, n, lo, hi, t0, t1, at_end=False):
    return _scan(rng.uniform(lo, hi, n), np.arange(n) * (2 * math.pi / n), t0, t1, at_end)


def _entries(rng, path, n=290, lo=0.2, hi=2.5, at_end=()):
    """One circle scan per pose of `path` ((x, y, theta) list), utimes T0, T0 + DT, ...; at_end: the indices whose rays all carry the
    pose's utime."""
    return [(_circle(rng, n, lo, hi, T0 + (k - 1) * DT, T0 + k * DT, k in at_end), (p[0], p[1], p[2], T0 + k * DT)) for k, p in enumerate(path)]


def _drift(n, x=0.0, y=0.0, step=0.01):
    return [(x + step * k, y + 0.5 * step * math.sin(0.7 * k), 0.05 * k) for k in range(n)]


def _centred(width, height, mpc):
    return (-0.5 * width * mpc, -0.5 * height * mpc)


def _any(case, res):
    assert not np.array_equal(res["truth"], case.base)


# ---- scan counts around the chunk size
COUNTS = [1, 2, mm.CHUNK - 1, mm.CHUNK, mm.CHUNK + 1, 3 * mm.CHUNK + 1]


def counts(orc, n_active, with_prev):
    """n_active scans change cells: with a previous pose the log holds n_active entries, without one n_active + 1 (the first latches)."""
    rng = np.random.default_rng(1000 + n_active)
    W = H = 96
    base = rng.integers(-128, 128, (H, W)).astype(np.int8)
    path = _drift(n_active + 1)
    ent = _entries(rng, path)
    prev = None
    if with_prev:
        prev, ent = ent[0][1], ent[1:]

    def condition(case, res):
        assert res["info"]["scans"] == n_active and res["chunks"] == -(-n_active // mm.CHUNK)
        assert res["pairs"] == 4 * res["chunks"]                # 2 x 2 tiles, a robot in the middle
        _any(case, res)

    return Case(f"counts_{n_active}_{'prev' if with_prev else 'latch'}", W, H, 0.05, _centred(W, H, 0.05), base, ent, 5.0, 3, 1, condition, prev=prev,
                saturates=n_active >= 2)


def count_one(orc):
    """count = 1 without a previous pose: the scan latches its pose and nothing changes."""
    rng = np.random.default_rng(1001)
    base = rng.integers(-128, 128, (96, 96)).astype(np.int8)

    def condition(case, res):
        assert res["info"]["scans"] == 0 and res["chunks"] == 0 and res["pairs"] == 0 and np.array_equal(res["truth"], case.base)

    return Case("count_one", 96, 96, 0.05, _centred(96, 96, 0.05), base, _entries(rng, _drift(3)), 5.0, 3, 1, condition, first=1, count=1)


# ---- pose jumps
def leave_and_return(orc):
    """Three chunks: in the left tile, in the right tile, back in the left tile.  The left tile has pairs in chunks 0 and 2, not 1."""
    rng = np.random.default_rng(1100)
    W, H = 192, 64
    o = _centred(W, H, 0.05)
    left, right = (o[0] + 1.6, 0.0), (o[0] + 8.0, 0.0)
    C = mm.CHUNK
    path = [(left[0], left[1], 0.0)] + [((left if k // C != 1 else right)[0] + 0.005 * k, 0.003 * k, 0.1 * k) for k in range(3 * C)]
    ent = _entries(rng, path, hi=1.0, at_end=(1 + C, 1 + 2 * C))         # the two jumps are not interpolated
    base = rng.integers(-128, 128, (H, W)).astype(np.int8)

    def condition(case, res):
        assert res["chunks"] == 3 and sorted(res["info"]["pairs"]) == [(0, 0), (0, 2), (2, 1)]
        _any(case, res)

    return Case("leave_and_return", W, H, 0.05, o, base, ent, 5.0, 3, 1, condition, saturates=True)


def jump_8m(orc):
    """An 8 m jump inside one scan: its rays leave from poses all along the way, the chunk's box spans the grid."""
    rng = np.random.default_rng(1110)
    W, H = 203, 117
    o = _centred(W, H, 0.05)
    path = [(-4.0 + 0.01 * k, 0.2, 0.0) for k in range(6)] + [(4.0 + 0.01 * k, -0.3, 1.0) for k in range(6)]
    base = rng.integers(-128, 128, (H, W)).astype(np.int8)

    def condition(case, res):
        assert res["chunks"] == 1 and res["pairs"] == res["info"]["tiles"] == 8
        b = res["info"]["per_scan"][5][2]                       # the jumping scan
        assert b[2] - b[0] > 160
        _any(case, res)

    return Case("jump_8m", W, H, 0.05, o, base, _entries(rng, path), 5.0, 3, 1, condition, saturates=True)


# ---- saturation and order
SAT_BASES = [-128, -100, 0, 100, 127]
SAT_ODDS = [(3, 1), (127, 127)]
_sat_entries = []


def saturation(orc, base_value, hit, miss):
    """2048 rays from a standing robot, 20 scans (two chunks): the start cell is crossed by every ray; along each of 64 directions the
    rays end at 1.0 m and at 1.5 m, so the end cells of the short ones are crossed by the long ones -- a hit and a miss in the same
    scan, both saturating with odds of 127, and again in the next scan.  The last six scans reach 2.0 m everywhere: they cross
    cells the first fourteen have driven to +127, which sum-then-clamp cannot follow."""
    W = H = 96
    if not _sat_entries:
        i = np.arange(2048)
        r = np.where((i // 64) % 2 == 0, 1.0, 1.5)
        d = (i % 64) * (2 * math.pi / 64)
        _sat_entries.extend((_scan(r if k < 15 else np.full(2048, 2.0), d, T0 + (k - 1) * DT, T0 + k * DT), (0.012, 0.013, 0.0, T0 + k * DT))
                            for k in range(21))
    base = np.full((H, W), base_value, np.int8)

    def condition(case, res):
        hits, misses, _ = res["info"]["per_scan"][0]
        assert res["chunks"] == 2 and misses.max() == 2048 and misses[48, 48] == 2048
        both = (hits >= 16) & (misses >= 16)                    # with odds of 127 both adds pass 255
        assert both.sum() >= 32
        _any(case, res)

    return Case(f"saturation_{base_value}_{hit}_{miss}", W, H, 0.05, _centred(W, H, 0.05), base, list(_sat_entries), 5.0, hit, miss, condition,
                saturates=True)


# ---- shapes
def small_grid_all_sides(orc):
    """A grid smaller than one tile; the rays leave it on all four sides."""
    rng = np.random.default_rng(1300)
    W = H = 40
    base = rng.integers(-128, 128, (H, W)).astype(np.int8)
    ent = _entries(rng, _drift(6, x=0.1, y=-0.1), lo=2.0, hi=4.0)

    def condition(case, res):
        assert res["info"]["tiles"] == 1 and res["pairs"] == 1
        ch = res["truth"] != case.base
        assert ch[0, :].any() and ch[H - 1, :].any() and ch[:, 0].any() and ch[:, W - 1].any()

    return Case("small_grid_all_sides", W, H, 0.05, _centred(W, H, 0.05), base, ent, 5.0, 3, 1, condition)      # (misses only: no order to get wrong)


def scan_outside(orc):
    """One scan taken 30 m away from the grid: its box is empty."""
    rng = np.random.default_rng(1310)
    W, H = 96, 70
    base = rng.integers(-128, 128, (H, W)).astype(np.int8)
    path = _drift(3) + [(30.0, 30.0, 0.3)] + _drift(3, x=0.2)
    ent = _entries(rng, path, at_end=(3, 4))

    def condition(case, res):
        boxes = [b for _, _, b in res["info"]["per_scan"]]
        assert boxes[2] is None and all(b is not None for i, b in enumerate(boxes) if i != 2)
        _any(case, res)

    return Case("scan_outside", W, H, 0.05, _centred(W, H, 0.05), base, ent, 5.0, 3, 1, condition)


def max_laser_half(orc):
    rng = np.random.default_rng(1320)
    W = H = 96
    base = rng.integers(-128, 128, (H, W)).astype(np.int8)
    ent = _entries(rng, _drift(5), lo=0.2, hi=2.0)

    def condition(case, res):
        for (s, _), (hits, _, _) in zip(case.entries[1:], res["info"]["per_scan"]):
            cut = int((s.ranges > np.float32(case.max_laser)).sum())
            assert 100 < cut < 190 and hits.sum() == 290 - cut
        _any(case, res)

    return Case("max_laser_half", W, H, 0.05, _centred(W, H, 0.05), base, ent, 1.1, 3, 1, condition)


def zero_kept(orc):
    """The third entry keeps no ray (every range <= 0.15); it still moves the previous pose of the fourth."""
    rng = np.random.default_rng(1330)
    W = H = 96
    base = rng.integers(-128, 128, (H, W)).astype(np.int8)
    ent = _entries(rng, _drift(5, step=0.05))
    s, p = ent[2]
    r = s.ranges.copy()
    r[:] = 0.1
    r[::3] = mm.MIN_RANGE
    ent[2] = (LidarScan(r, s.thetas, s.times, utime=s.utime), p)

    def condition(case, res):
        hits, misses, box = res["info"]["per_scan"][1]
        assert box is None and hits.sum() == 0 and misses.sum() == 0
        _any(case, res)

    return Case("zero_kept", W, H, 0.05, _centred(W, H, 0.05), base, ent, 5.0, 3, 1, condition)


def ray_count(orc, n):
    rng = np.random.default_rng(1340 + n)
    W, H = 203, 117
    base = rng.integers(-128, 128, (H, W)).astype(np.int8)
    path = _drift(4, x=-1.0, y=0.3, step=0.03)
    ent = [(_scan(rng.uniform(0.2, 5.4, n), rng.uniform(-math.pi, math.pi, n), T0 + (k - 1) * DT, T0 + k * DT), (p[0], p[1], p[2], T0 + k * DT))
           for k, p in enumerate(path)]

    def condition(case, res):
        for s, _ in case.entries:
            assert int((s.ranges > mm.MIN_RANGE).sum()) == n
        assert case.width % 4 != 0
        _any(case, res)

    return Case(f"ray_count_{n}", W, H, 0.05, _centred(W, H, 0.05), base, ent, 5.0, 3, 1, condition, saturates=n >= 720)


# ---- the time rule
def equal_utime(orc):
    """Entries 2 and 3 carry one utime: no interpolation for entry 3, whatever its rays' stamps say."""
    rng = np.random.default_rng(1400)
    W = H = 96
    base = rng.integers(-128, 128, (H, W)).astype(np.int8)
    ent = _entries(rng, _drift(6, step=0.08))
    s, p = ent[3]
    ent[3] = (s, (p[0], p[1], p[2], ent[2][1][3]))

    def condition(case, res):
        assert case.entries[2][1][3] == case.entries[3][1][3] != case.entries[4][1][3]
        s3, p3 = case.entries[3]
        assert len(set(s3.times.tolist())) > 100
        c = mm.ray_cells(orc, s3, mm._opose(orc, case.entries[2][1]), mm._opose(orc, p3), case.origin, case.cpm, case.max_laser)
        assert len(np.unique(c[:, :2], axis=0)) == 1            # every ray leaves from the one start cell
        _any(case, res)

    return Case("equal_utime", W, H, 0.05, _centred(W, H, 0.05), base, ent, 5.0, 3, 1, condition)


# ---- poses and windows
def other_poses(orc):
    """The window rebuilt at poses that are not the recorded ones."""
    rng = np.random.default_rng(1500)
    W = H = 96
    base = rng.integers(-128, 128, (H, W)).astype(np.int8)
    ent = _entries(rng, _drift(20))
    moved = [(p[0] + 0.3, p[1] - 0.2, p[2] + 0.4, p[3]) for _, p in ent]

    def condition(case, res):
        rec = mm.truth(orc, [s for s, _ in case.entries], [p for _, p in case.entries], None, case.base, case.mpc, case.cpm, case.origin,
                       case.max_laser, case.hit, case.miss)
        assert not np.array_equal(rec, res["truth"])

    return Case("other_poses", W, H, 0.05, _centred(W, H, 0.05), base, ent, 5.0, 3, 1, condition, poses=moved, saturates=True)


RING_CAPACITY, RING_APPENDS, RING_WINDOW = 8, 11, 5


def ring_all(orc):
    """What a ring of 8 holds after 11 appends: the last 8, the oldest first."""
    rng = np.random.default_rng(1600)
    W = H = 96
    base = rng.integers(-128, 128, (H, W)).astype(np.int8)
    ent = _entries(rng, _drift(RING_APPENDS, step=0.03))
    return Case("ring_all", W, H, 0.05, _centred(W, H, 0.05), base, ent[RING_APPENDS - RING_CAPACITY:], 5.0, 3, 1, _any), ent


def ring_window(orc):
    """The last 5 of them, primed with the pose before the window."""
    case, ent = ring_all(orc)
    held = case.entries
    first = len(held) - RING_WINDOW
    return Case("ring_window", case.width, case.height, 0.05, case.origin, case.base, held, 5.0, 3, 1, _any, first=first, prev=held[first - 1][1]), ent


def other_frame(orc):
    """The log of other_poses (at its recorded poses) into a 10 cm grid with another origin."""
    src = other_poses(orc)
    rng = np.random.default_rng(1700)
    W, H = 70, 50
    base = rng.integers(-128, 128, (H, W)).astype(np.int8)

    def condition(case, res):
        assert res["info"]["tiles"] == 2
        _any(case, res)

    return Case("other_frame", W, H, 0.1, (-2.9, -2.2), base, src.entries, 5.0, 3, 1, condition, saturates=True)


# ---- long and thin: walks that start behind dmaj = 32768
LONG_DMAJ, LONG_DMIN = (32772, 32778), (0, 1, 3, 7)


def long_thin(orc):
    """A grid of 32 800 x 8 cells (513 tiles in a row) and two scans of eight rays from near one short edge, almost along the long axis,
    ending inside the grid: every tile but the first takes up a walk with dmaj >= 32768 at k0 > 0, where the start's division takes
    64 bits (bl_mapray_dev.h)."""
    rng = np.random.default_rng(1800)
    W, H = 32800, 8
    o = (-820.0, -0.2)
    base = rng.integers(-128, 128, (H, W)).astype(np.int8)
    v = np.array([(a, b) for a in LONG_DMAJ for b in LONG_DMIN], np.float64)
    path = [(o[0] + (10.5 + k) * 0.05, o[1] + 0.3 * 0.05, 0.0) for k in range(3)]
    ent = [(_scan(np.hypot(v[:, 0], v[:, 1]) * 0.05, np.arctan2(v[:, 1], v[:, 0]), T0 + (k - 1) * DT, T0 + k * DT), (p[0], p[1], p[2], T0 + k * DT))
           for k, p in enumerate(path)]

    def condition(case, res):
        assert res["info"]["scans"] == 2 and res["chunks"] == 1 and res["pairs"] == res["info"]["tiles"] == 513
        for k in (1, 2):
            c = mm.ray_cells(orc, ent[k][0], mm._opose(orc, ent[k - 1][1]), mm._opose(orc, ent[k][1]), case.origin, case.cpm, case.max_laser)
            dx, dy = np.abs(c[:, 2] - c[:, 0]), np.abs(c[:, 3] - c[:, 1])
            assert len(c) == len(v) and (dx >= 32768).all() and sorted(set(dy.tolist())) == list(LONG_DMIN)
            assert (c >= 0).all() and (c[:, [0, 2]] < W).all() and (c[:, [1, 3]] < H).all()
        assert (res["truth"] != case.base).sum() > 32768

    return Case("long_thin", W, H, 0.05, o, base, ent[1:], 1700.0, 3, 1, condition, prev=ent[0][1])


# ------------------------------------------------------------------ the list
BUILDERS = {"count_one": count_one}
for _n in COUNTS:
    if _n > 1:
        BUILDERS[f"counts_{_n}_latch"] = (lambda orc, n=_n: counts(orc, n, False))
    BUILDERS[f"counts_{_n}_prev"] = (lambda orc, n=_n: counts(orc, n, True))
BUILDERS["leave_and_return"] = leave_and_return
BUILDERS["jump_8m"] = jump_8m
for _b in SAT_BASES:
    for _h, _m in SAT_ODDS:
        BUILDERS[f"saturation_{_b}_{_h}_{_m}"] = (lambda orc, b=_b, h=_h, m=_m: saturation(orc, b, h, m))
BUILDERS["small_grid_all_sides"] = small_grid_all_sides
BUILDERS["scan_outside"] = scan_outside
BUILDERS["max_laser_half"] = max_laser_half
BUILDERS["zero_kept"] = zero_kept
BUILDERS["ray_count_720"] = lambda orc: ray_count(orc, 720)
BUILDERS["ray_count_8192"] = lambda orc: ray_count(orc, 8192)
BUILDERS["equal_utime"] = equal_utime
BUILDERS["other_poses"] = other_poses
BUILDERS["ring_all"] = lambda orc: ring_all(orc)[0]
BUILDERS["ring_window"] = lambda orc: ring_window(orc)[0]
BUILDERS["other_frame"] = other_frame
BUILDERS["long_thin"] = long_thin

_cases = {}


def get(name, orc):
    if name not in _cases:
        _cases[name] = BUILDERS[name](orc)
        assert _cases[name].name == name
    return _cases[name]
