"""Named cases of loop closure by place recognition (tests/place_model.py).  TEST INFRASTRUCTURE, no GPU.

Every case is a small scan history in the world of loop_closure_cases -- a robot on a circle, the scans ray-cast standing still at the
true poses, a second visit of the same spots with a constant heading offset and, where stated, recorded poses that drifted -- the
parameters of a find_places, and `reaches`: the condition, evaluated on the model (place_model.find's four results), that shows the
case takes the path it is named for.  model(name) is computed once and shared by the CPU and the GPU tests.

k_pr_match's layout, which the three same-scan cases name: partners are taken in groups of four, group g = j // 4 belongs to wave
g % 16 on its trip g // 16."""
import math

import numpy as np

import botlab_amd as bl
from botlab_amd import synth

import loop_closure_cases as lcc
import loop_closure_model as lcm
import oracle_lib
import place_model as pm

MPC, CPM, ORIGIN = lcc.MPC, lcc.CPM, lcc.ORIGIN
# The drift case's bound on a kept edge's z against the true relative pose of j and q.  Pose mode on loop_closure_cases' two_lap case,
# measured with edge_error() below over its 17 kept edges (tests/test_place_model_cpu.py prints and re-checks it): 0.004486 m and
# 0.004958 rad at most.  The bound is twice that: the place centre adds no error of its own to a converged match.
# The drift case has two_lap's submap of 130 cells; its own kept edges lie within 0.0048 m and 0.0080 rad (at stride 1: 0.0079 m and
# 0.0091 rad).  With a 64-cell submap the same history has kept edges up to 0.0114 rad off: fewer walls inside the submap to hold
# the heading.
TWO_LAP_POS_ERROR, TWO_LAP_ANG_ERROR = 0.004486, 0.004958
DRIFT_POS_BOUND, DRIFT_ANG_BOUND = 2 * TWO_LAP_POS_ERROR, 2 * TWO_LAP_ANG_ERROR
DRIFT_RADIUS = 0.5                     # the pair search's radius, which the second lap's recorded poses lie beyond
DRIFT_XY = (0.6, 0.4)                  # what the recorded poses have drifted by when the first lap ends

# the match window of the revisit cases: the heading read off a shift is good to two sectors (11.25 degrees), the partner to one log
# entry (0.157 m on the 1.5 m circle of 60 scans)
WIDE = dict(nx=5, ny=5, ntheta=32, dtheta=math.radians(0.5))
BASE = dict(stride=1, min_gap=4, w=1, submap_cells=64, nx=2, ny=2, ntheta=2, dtheta=math.radians(1.0), max_range=8.0, half_life=64,
            min_score=0, maxLaserDistance=lcc.MAX_LASER, hitOdds=lcc.HIT, missOdds=lcc.MISS, prior=(0, 0, 0, 0),
            bins_per_meter=4.0, place_max_range=8.0, dilate=1, min_key=16384, min_bits=8)


def _wrap(a):
    return math.atan2(math.sin(a), math.cos(a))


def lap_truth(n, lap, radius, offset):
    """n poses on a circle, `lap` to a turn, heading along the tangent; from the second lap on the heading is turned by `offset`"""
    t = np.arange(n) / lap * 2 * math.pi
    th = [_wrap(v + math.pi / 2 + (offset if k >= lap else 0.0)) for k, v in enumerate(t)]
    return np.stack([radius * np.cos(t), radius * np.sin(t), np.array(th)], 1)


def lap_history(n, lap, radius=0.5, offset=0.0, rays=synth.RAYS, drift=(0.0, 0.0), drift_from=0):
    """(scans, poses, truth): the scans ray-cast standing still at the truth; the recorded poses are the truth moved by a drift that
    grows evenly from entry `drift_from` to the end of the first lap, where it is `drift`, and stays there"""
    w = lcc.world()
    truth = lap_truth(n, lap, radius, offset)
    utimes = 100000 * (np.arange(n) + 1)
    scans, poses = [], []
    for k in range(n):
        s = synth.raycast_scan(w, ORIGIN, MPC, truth[k], truth[k], int(utimes[k]), rays=rays)
        scans.append(bl.LidarScan(s.ranges, s.thetas, np.full(s.num_ranges, int(utimes[k]), np.int64), utime=int(utimes[k])))
        f = min(max((k - drift_from) / (lap - drift_from), 0.0), 1.0)
        dx, dy = drift[0] * f, drift[1] * f
        poses.append((np.float32(truth[k, 0] + dx), np.float32(truth[k, 1] + dy), np.float32(truth[k, 2]), int(utimes[k])))
    return scans, poses, truth


def _scan(scan, ranges=None, thetas=None):
    r = np.asarray(scan.ranges if ranges is None else ranges, np.float32)
    t = np.asarray(scan.thetas[:len(r)] if thetas is None else thetas, np.float32)
    return bl.LidarScan(r.copy(), t.copy(), scan.times[:len(r)].copy(), utime=scan.utime)


def edge_error(z, truth_j, truth_q):
    """(metres, radians) between an edge's z and the true pose of q seen from the true pose of j"""
    want = lcc._rel(truth_j, truth_q)
    return float(math.hypot(z[0] - want[0], z[1] - want[1])), abs(_wrap(z[2] - want[2]))


class Case(lcc.Case):
    def __init__(self, name, scans, poses, params, reaches, truth=None, **kw):
        lcc.Case.__init__(self, name, scans, poses, {}, reaches, **kw)
        self.params = dict(BASE, **params)
        self.truth = truth


def _second_lap(lap, offset):
    """every query of the second lap: its partner within one log entry of the true revisit, its shift within two sectors of the offset"""
    want = offset * 64 / (2 * math.pi)

    def reaches(m):
        pl = [p for p in m[2] if p["q"] >= lap]
        if len(pl) < 7:
            return False
        for p in pl:
            d = (int(p["shift"]) - want) % 64
            if abs(int(p["j"]) - (int(p["q"]) - lap)) > 1 or min(d, 64 - d) > 2 or p["partner"] != p["j"]:
                return False
        return any(c["flags"] == 0 for c in m[3])
    return reaches


def _same_scan(ja, jb, q):
    """the scan of q logged at ja and jb as well (and entry 7, the true revisit, given another scan): both reach key 65536 at shift 0,
    the lower wins"""
    def reaches(m):
        d, pl = m[0], m[2][-1]
        return (pl["q"] == q and np.array_equal(d[ja], d[q]) and np.array_equal(d[jb], d[q]) and pl["key"] == 65536 and
                pl["j"] == min(ja, jb) and pl["shift"] == 0 and
                sum(np.array_equal(d[j], d[q]) for j in range(q - 4)) == 2)
    return reaches


_cases = None
_long = None
SMALL_N, SMALL_LAP = 24, 16
TIE = dict(stride=23, dilate=0, min_gap=4)                       # the queries 0 (no partner: last < 0) and 23 (last = 18)
# (same_scan_two_trips: 72 scans, the queries 0 and 71, last = 66)


def cases():
    global _cases
    if _cases is not None:
        return _cases
    out = []

    def add(name, hist, params, reaches, **kw):
        out.append(Case(name, list(hist[0]), list(hist[1]), params, reaches, truth=hist[2], **kw))

    lap = 60
    for name, off in (("revisit_plus_100", math.radians(100.0)), ("revisit_minus_37", math.radians(-37.0))):
        add(name, lap_history(70, lap, radius=1.5, offset=off), dict(WIDE, min_gap=50, w=3), _second_lap(lap, off))
    # the drift builds up on the far side of the loop, entries 14 to 60: the submaps of the partners 0 .. 10 (w = 3) are undisturbed
    add("drift", lap_history(72, lap, radius=1.5, offset=math.radians(100.0), drift=DRIFT_XY, drift_from=14),
        dict(WIDE, min_gap=59, w=3, stride=2, submap_cells=130), lambda m: sum(c["flags"] == 0 for c in m[3]) >= 1)

    small = lap_history(SMALL_N, SMALL_LAP)
    flat = np.full(synth.RAYS, 2.0, np.float32)

    def small_with(changes):
        """the small history with the ranges (or the whole scan) of some entries replaced; times and utime stay the entry's own"""
        scans = list(small[0])
        for k, v in changes.items():
            scans[k] = v if isinstance(v, bl.LidarScan) else _scan(scans[k], v)
        return scans, small[1], small[2]

    # ---- ties
    add("tie_all_shifts", small_with({23: flat, 3: flat}), TIE,
        lambda m: m[2][-1]["j"] == 3 and m[2][-1]["shift"] == 0 and m[2][-1]["key"] == 65536 and
        len(set(pm.overlaps(m[0][23], m[0][3]).tolist())) == 1)
    half = np.tile(small[0][5].ranges[:145], 2)                                   # symmetric under a half turn
    add("tie_half_turn", small_with({3: half, 23: np.roll(half, 45)}), TIE, _half_turn)
    add("same_scan_two_waves", small_with({2: small[0][23].ranges, 6: small[0][23].ranges, 7: small[0][8].ranges}), TIE, _same_scan(2, 6, 23))       # groups 0 and 1
    far = lap_history(72, lap, radius=1.5, offset=math.radians(100.0))
    far[0][2], far[0][66] = _scan(far[0][2], far[0][71].ranges), _scan(far[0][66], far[0][71].ranges)
    add("same_scan_two_trips", far, dict(TIE, stride=71), _same_scan(2, 66, 71))                               # groups 0 and 16: wave 0
    add("same_scan_one_group", small_with({2: small[0][23].ranges, 3: small[0][23].ranges, 7: small[0][8].ranges}), TIE, _same_scan(2, 3, 23))       # group 0

    # ---- empty scans, the two thresholds
    none = np.full(synth.RAYS, 9.0, np.float32)                                   # kept by the log, beyond max_range
    add("empty_scans", small_with({0: none, 23: none}), dict(TIE, min_bits=0, min_key=0),
        lambda m: m[1][0] == 0 and m[1][23] == 0 and tuple(m[2][-1])[1:5] == (0, 0, 0, 0) and m[2][-1]["partner"] == 0 and len(m[3]) == 1)
    add("min_bits_query", small_with({23: small[0][23].ranges[:5]}), TIE,
        lambda m: 0 < m[1][23] < 8 and m[2][-1]["j"] == -1 and m[2][-1]["bits_q"] == m[1][23] and len(m[3]) == 0)
    few = {j: small[0][j].ranges[:3] for j in range(3)}
    add("min_bits_partners", small_with(few), dict(stride=7, min_gap=4),
        lambda m: (m[1][:3] < 8).all() and (m[1][:3] > 0).all() and m[2][1]["q"] == 7 and m[2][1]["j"] == -1 and m[2][2]["j"] >= 3)
    key23 = int(pm.find(None, small[0], small[1], MPC, CPM, with_candidates=False, **dict(BASE, stride=23))[2][-1]["key"])
    add("min_key_at", small, dict(stride=23, min_key=key23), lambda m: m[2][-1]["key"] == key23 and m[2][-1]["partner"] == m[2][-1]["j"] >= 0)
    add("min_key_above", small, dict(stride=23, min_key=key23 + 1),
        lambda m: m[2][-1]["key"] == key23 and m[2][-1]["partner"] == -1 and m[2][-1]["j"] >= 0 and len(m[3]) == 0)

    # ---- the descriptor's edges.  No candidate (min_key beyond every key): a scan with NaN thetas is neither traced nor matched.
    th = small[0][23].thetas.copy()
    th[0:40] -= np.float32(2 * math.pi)                                           # negative
    th[40:80] += np.float32(2 * math.pi)                                          # above 2 pi
    th[80:90] = [1024.0, -1024.0, np.nextafter(np.float32(1024), np.float32(2000)), -1025.0, 2000.0, -3.0e9, np.inf, -np.inf, 1e30, 1023.99]
    th[90:100] = np.nan
    add("thetas", small_with({23: _scan(small[0][23], thetas=th), 2: _scan(small[0][2], thetas=th)}), dict(stride=23, min_key=65536, dilate=0),
        lambda m: len(m[3]) == 0 and m[2][-1]["j"] >= 0 and m[2][-1]["key"] < 65536 and 0 < m[1][23] and
        not np.array_equal(m[0][23], pm.descriptor(small[0][23].ranges, small[0][23].thetas, 4.0, 8.0)))
    rb = small[0][23].ranges.copy()
    rb[:12] = [0.25, 0.5, 0.75, np.nextafter(np.float32(0.25), np.float32(0)), 3.875, 4.0, np.nextafter(np.float32(4.0), np.float32(0)), 5.0, 6.0,
               np.nextafter(np.float32(6.5), np.float32(0)), 6.5, 0.15]
    add("bin_borders", small_with({23: rb}), dict(stride=23, bins_per_meter=8.0, place_max_range=6.5, min_key=0),
        lambda m: (m[0][23][0] >> 31) & 1 == 1 and m[0][23][0] & 0b1010100 == 0b1010100 and len(m[3]) == 1)
    add("second_trip", small, dict(stride=23),
        lambda m: synth.RAYS > 256 and not np.array_equal(m[0][23], pm.descriptor(small[0][23].ranges[:256], small[0][23].thetas[:256], 4.0, 8.0)))

    # ---- the query list, the ring
    add("stride_3", small, dict(stride=3), lambda m: len(m[2]) == 8 and (m[2]["j"][:2] == -1).all() and (m[2]["j"][2:] >= 0).all() and len(m[3]) >= 2)
    add("wrapped_ring", small, dict(stride=5, min_gap=3), lambda m: len(m[0]) == 17 and len(m[3]) >= 1, capacity=17)

    # ---- the signed step
    back = lap_history(SMALL_N, SMALL_LAP, offset=math.pi)
    add("shift_32", back, dict(stride=1, min_gap=10, nx=3, ny=3, ntheta=8, dtheta=math.radians(1.0)),
        lambda m: any(c["shift"] == 32 and abs(float(c["centre"][2])) > math.pi for c in m[3]))
    add("shift_63", lap_history(SMALL_N, SMALL_LAP, offset=-2 * math.pi / 64), dict(stride=1, min_gap=10, nx=3, ny=3, ntheta=8, dtheta=math.radians(1.0)),
        lambda m: any(c["shift"] == 63 for c in m[3]))

    # ---- dilation
    add("dilate_0", small, dict(stride=4, dilate=0, min_key=0), lambda m: len(m[3]) >= 2)
    add("dilate_1", small, dict(stride=4, dilate=1, min_key=0), _differs_from("dilate_0"))

    # ---- the gate's flags in place mode
    add("min_score", small, dict(stride=23, min_score=1 << 19), lambda m: len(m[3]) == 1 and m[3][0]["flags"] & lcm.NOT_ACCEPTED)
    add("w0", small, dict(stride=23, w=0), lambda m: len(m[3]) == 1 and m[3][0]["flags"] & lcm.TIED and not m[3][0]["cells"].any())
    add("on_edge", lap_history(SMALL_N, SMALL_LAP, offset=math.radians(8.0)), dict(stride=1, min_gap=10, ntheta=1, nx=1, ny=1),
        lambda m: any(c["flags"] & lcm.ON_EDGE for c in m[3]))
    big = small[0][23]
    many = bl.LidarScan(np.tile(big.ranges, 15), np.tile(big.thetas, 15), np.tile(big.times, 15), utime=big.utime)
    add("too_many_rays", small_with({23: many}), dict(stride=23),
        lambda m: len(m[3]) == 1 and m[3][0]["flags"] == lcm.TOO_MANY_RAYS and m[3][0]["valid"] > 4096, max_rays=15 * synth.RAYS)
    _cases = {c.name: c for c in out}
    return _cases


def _half_turn(m):
    """the query's descriptor repeats after 32 sectors, so s and s + 32 overlap alike; the best shift is the lower of its pair"""
    d, pl = m[0], m[2][-1]
    ov = pm.overlaps(d[23], d[int(pl["j"])]) if pl["j"] >= 0 else None
    return (pl["j"] >= 0 and np.array_equal(d[23][:32], d[23][32:]) and np.array_equal(ov[:32], ov[32:]) and 0 < pl["shift"] < 32 and
            pl["overlap"] == ov.max())


def _differs_from(other):
    def reaches(m):
        o = model(other)
        return len(m[3]) >= 2 and (m[2]["key"] != o[2]["key"]).any() and (m[2]["j"] >= 0).sum() == (o[2]["j"] >= 0).sum()
    return reaches


LONG_N, LONG_LAP, LONG_RAYS = 1100, 800, 24
LONG_SAMPLE_KEPT = 8


def long_case():
    """more than 1024 queries and more than 256 candidates on both sides of query index 1024: k_lc_number's second trip in place mode
    and k_lc_records' second workgroup.  A lap of 800 scans of 24 rays, a gap of 700."""
    global _long
    if _long is None:
        hist = lap_history(LONG_N, LONG_LAP, rays=LONG_RAYS)

        def reaches(m):
            qi = [c["q"] for c in m[3]]
            return (len(m[2]) >= 1025 and len(m[3]) >= 257 and any(v <= 1023 for v in qi) and any(v >= 1024 for v in qi) and
                    any(c["flags"] == 0 for c in m[3][:256]) and any(c["flags"] == 0 for c in m[3][256:]))
        _long = Case("long_log", list(hist[0]), list(hist[1]), dict(stride=1, min_gap=700, w=1, min_key=0, min_bits=1), reaches, truth=hist[2],
                     max_rays=LONG_RAYS)
    return _long


_models = {}


def model(name):
    """place_model.find's (words, bits, places, candidates) of a case"""
    if name not in _models:
        c = long_case() if name == "long_log" else cases()[name]
        scans, poses = c.retained()
        _models[name] = pm.find(oracle_lib.load_oracle(), scans, poses, c.mpc, c.cpm, **c.params)
    return _models[name]
