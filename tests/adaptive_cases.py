"""Hand-built inputs for the adaptive particle count (bl_pf_set_adaptive): clouds whose bins are decided here, not by a filter run, and
the chains of commanded counts that put a resampling update at a chosen (active, next) pair.

A case is a cloud of exactly `cap` poses with the adaptive parameters it is counted under.  It reaches k_kld_count as the parents
of one resampling update: uploaded with equal units and drawn with rand_value = MID the draw is the identity (asserted where it is
used), so the parent in slot j -- and with it the workgroup of k_kld_count that sees it, 1024 slots each -- is pose j.
tests/test_adaptive_cases_cpu.py proves on the model alone that every case is what its name says; tests/test_gpu_adaptive_edges.py
holds the device against the model on them.  Every pose lies inside +-3.4 m and +-pi: the free interior of a 10 m map."""
import collections
import math

import numpy as np

import adaptive_model as am

MID = am.RAND_MAX // 2                       # equal weights drawn with this rand() value: output m takes record m
WG = 1024                                    # parents per workgroup of k_kld_count (KLD_PER_WG)
LIM = am.IDX_LIM
BXY, BTH = 0.1, math.radians(10.0)
EXACT_EPS = 10.0                             # n(k) < k for every k >= 2: no capacity is reached, k_sat = cap + 1, the count is exact
Z = 2.326
PI_F = np.float32(math.pi)

Case = collections.namedtuple("Case", "name cap x y th params k")       # k: the distinct bins the builder states (proved in the CPU test)

SIZES = [2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097]      # a wave, a workgroup of 256, one pass of 1024: each +- 1


def _case(name, x, y, th, params, k):
    x, y, th = (np.ascontiguousarray(v, dtype=np.float32) for v in (x, y, th))
    assert x.shape == y.shape == th.shape and x.ndim == 1
    return Case(name, int(x.size), x, y, th, params, k)


def _params(cap, min_particles=2, eps=EXACT_EPS, bxy=BXY, bth=BTH):
    return am.Params(min(min_particles, cap), eps, Z, bxy, bth)


def grid_xy(pos, bxy=BXY, side=64):
    """Centres of the cells pos (integers in [0, side^2)) of a side x side board of bin_xy bins around the origin."""
    pos = np.asarray(pos, dtype=np.int64)
    half = side // 2
    x = ((pos % side) - half + 0.5) * bxy
    y = ((pos // side) - half + 0.5) * bxy
    return x.astype(np.float32), y.astype(np.float32)


# ---------------------------------------------------------------- A1: sizes
def own_bin(cap):
    """Every particle in an (x, y) bin of its own: k = cap."""
    x, y = grid_xy(np.arange(cap), side=66)
    return _case(f"own_bin_{cap}", x, y, np.full(cap, 0.05, np.float32), _params(cap), cap)


def one_bin(cap):
    """Distinct poses, all inside one bin: k = 1."""
    t = np.arange(cap, dtype=np.float64) / cap
    return _case(f"one_bin_{cap}", 0.01 + 0.08 * t, -0.09 + 0.08 * t, 0.01 + 0.1 * t, _params(cap), 1)


# ---------------------------------------------------------------- A2: edges
def edge_values(bxy=BXY):
    """Multiples of bin_xy on both sides of zero as floats, and the float below each (0.3f is above 3 * 0.1, 0.7f below 7 * 0.1)."""
    e = np.float32(np.arange(-20, 21) * bxy)
    return np.concatenate([e, np.nextafter(e, np.float32(-np.inf))])


THETA_EDGES = np.array([-PI_F, PI_F, np.nextafter(-PI_F, np.float32(0)), np.nextafter(PI_F, np.float32(0)), 0.0, -0.0], np.float32)


def edges(bxy=BXY):
    """x on the edges (y, theta fixed), y on the edges (x, theta fixed), theta at +-pi, their inward neighbours and +-0."""
    e = edge_values(BXY)                     # (the same floats under either bin width)
    n, t = e.size, THETA_EDGES.size
    x = np.concatenate([e, np.full(n, 0.05, np.float32), np.full(t, -3.05, np.float32)])       # (the thetas: away from both edge families)
    y = np.concatenate([np.full(n, 0.05, np.float32), e, np.full(t, -3.05, np.float32)])
    th = np.concatenate([np.full(2 * n, 0.05, np.float32), THETA_EDGES])
    return _case(f"edges_{bxy}", x, y, th, _params(x.size, bxy=bxy), {BXY: 88, 0.5: 24}[bxy])


# ---------------------------------------------------------------- A3: clamps
CLAMP_BIN = 1e-6                             # the clamp of 2^20 bins lies at 1.048 576 m / rad
CLAMP_Q = [LIM - 2, LIM - 1, LIM, LIM + 5, LIM + 1000, -LIM + 1, -LIM, -LIM - 1, -LIM - 5, -LIM - 1000]
CLAMP_BASE = np.float32(0.25)


def clamp_value(q):
    """A float inside bin q of CLAMP_BIN (its middle: half a bin is four floats wide there)."""
    return np.float32((q + 0.5) * CLAMP_BIN)


def clamps():
    """On each axis alone: one bin inside, on and beyond either clamp; the other two coordinates at CLAMP_BASE."""
    v = np.array([clamp_value(q) for q in CLAMP_Q], np.float32)
    n = v.size
    cols = []
    for axis in range(3):
        c = np.full(3 * n, CLAMP_BASE, np.float32)
        c[axis * n:(axis + 1) * n] = v
        cols.append(c)
    return _case("clamps", cols[0], cols[1], cols[2], _params(3 * n, bxy=CLAMP_BIN, bth=CLAMP_BIN), 12)


# ---------------------------------------------------------------- A4: deduplication levels (4096 parents: four workgroups)
DEDUP_CAP = 4 * WG
FINE_BIN = 0.001                             # 4096 bins of it span +-2.048 (m or rad)


def dedup_same_in_each_wg():
    """1024 distinct keys, the same 1024 in every workgroup: each is new in LDS four times and new in the global table once."""
    x, y = grid_xy(np.arange(DEDUP_CAP) % WG)
    return _case("dedup_same_in_each_wg", x, y, np.full(DEDUP_CAP, 0.05, np.float32), _params(DEDUP_CAP), WG)


def dedup_equal_per_wg():
    """Every workgroup holds 1024 copies of a key of its own."""
    x, y = grid_xy(np.arange(DEDUP_CAP) // WG * 67)
    return _case("dedup_equal_per_wg", x, y, np.full(DEDUP_CAP, 0.05, np.float32), _params(DEDUP_CAP), 4)


def dedup_one_common():
    """One key present in every workgroup (at a different slot each time), and 1023 private ones each."""
    j = np.arange(DEDUP_CAP)
    w, s = j // WG, j % WG
    pos = np.where(s == 17 * w, 0, j)
    pos = np.where((s == 0) & (w > 0), w * WG + 17 * w, pos)      # (the slot the common key took gives its cell to slot 0)
    x, y = grid_xy(pos)
    return _case("dedup_one_common", x, y, np.full(DEDUP_CAP, 0.05, np.float32), _params(DEDUP_CAP), 1 + 4 * (WG - 1))


def dedup_axis(axis):
    """4096 keys that differ in one field only (x: bits 42-62, y: bits 21-41, theta: bits 0-20); the others positive."""
    v = ((np.arange(DEDUP_CAP) - DEDUP_CAP // 2 + 0.5) * FINE_BIN).astype(np.float32)
    cols = [np.full(DEDUP_CAP, 0.0505, np.float32) for _ in range(3)]
    cols[axis] = v
    return _case(f"dedup_only_{'xyt'[axis]}", cols[0], cols[1], cols[2], _params(DEDUP_CAP, bxy=FINE_BIN, bth=FINE_BIN), DEDUP_CAP)


def dedup_cases():
    return [dedup_same_in_each_wg(), dedup_equal_per_wg(), dedup_one_common()] + [dedup_axis(a) for a in range(3)]


# ---------------------------------------------------------------- A5: the early stop
KSAT_SETUPS = [(1500, 0.3, 805), (2048, 0.2, 729)]       # (cap, epsilon, k_sat) at z = 2.326: two workgroups each


def ksat_case(cap, eps, distinct):
    """cap parents over `distinct` keys, dealt round-robin: the first workgroup alone already holds min(distinct, 1024) of them."""
    x, y = grid_xy(np.arange(cap) % distinct)
    return _case(f"ksat_{cap}_{distinct}", x, y, np.full(cap, 0.05, np.float32), _params(cap, eps=eps), distinct)


def ksat_cases():
    return [ksat_case(cap, eps, d) for cap, eps, ks in KSAT_SETUPS for d in (ks - 1, ks, cap)]


def count_cases():
    out = [f(cap) for cap in SIZES for f in (own_bin, one_bin)]
    return out + [edges(BXY), edges(0.5), clamps()] + dedup_cases() + ksat_cases()


def as_particles(case, utime, dtype):
    """The cloud as particles_t.particles (pose = parent pose, weight 1 / cap)."""
    p = np.zeros(case.cap, dtype)
    p["x"] = p["p_x"] = case.x
    p["y"] = p["p_y"] = case.y
    p["theta"] = p["p_theta"] = case.th
    p["utime"] = p["p_utime"] = int(utime)
    p["weight"] = 1.0 / case.cap
    return p


def explicit_bins(x, y, th, bxy, bth):
    """The set of clamped (floor(x / bxy), floor(y / bxy), floor(theta / bth)) triples, by math.floor on Python floats."""
    def q(v, b):
        return min(max(math.floor(v / b), -LIM), LIM - 1)
    return {(q(a, bxy), q(b, bxy), q(c, bth)) for a, b, c in zip(np.float32(x).astype(float), np.float32(y).astype(float), np.float32(th).astype(float))}


# ---------------------------------------------------------------- B: commanded counts
# A cloud inside one bin counts k = 1, so next = min_particles: setAdaptive(min_particles=t) commands t (it restarts next at the
# active count, so one settling update at active -> active comes first), setAdaptive(None) commands the capacity at once.
ONE_BIN = dict(epsilon=0.01, z=Z, binXY=100.0, binTheta=100.0)       # the whole map, one sign of x, y and theta: one bin
TRACK_START = (-0.75, 0.2, 1.5)              # x < 0 < y, theta: the cloud around it stays in the bin (-1, 0, 0)

CHAINS = {                                   # name -> (capacity, targets: a count, or None for "off: back to the capacity")
    "two_and_wave": (4096, [2, None, 63, None, 64, None, 65, 64, 65]),
    "chunk_and_tile": (4096, [127, 128, 129, None, 511, 512, 513, None, 511, 513]),
    "strict_par_min": (8192, [4095, None, 4096, None, 4097, None]),
}
REQUIRED_PAIRS = {
    "two_and_wave": [(4096, 2), (2, 4096), (4096, 63), (4096, 64), (4096, 65), (65, 64), (64, 65)],
    "chunk_and_tile": [(127, 128), (128, 129), (511, 512), (512, 513), (511, 513)],      # 128: strict chunks; 512: MCL_BLOCK = SCAN_TILE
    "strict_par_min": [(8192, 4095), (4095, 8192), (8192, 4096), (4096, 8192), (8192, 4097), (4097, 8192)],   # STRICT_PAR_MIN = 4096 as active and next
}
PARITY_CHAINS = {"shrink_grow_2": (4096, [2, None]), "wave_65_64": (4096, [65, 64]), "tile_511_513": (4096, [511, 513])}
PARITY_PAIRS = {"shrink_grow_2": [(4096, 2), (2, 4096)], "wave_65_64": [(65, 64)], "tile_511_513": [(511, 513)]}


def chain_pairs(cap, targets):
    """The (active, next) pair of every resampling update of a chain, the first (capacity -> capacity, the uploaded record) included."""
    active, nxt, pairs = cap, cap, [(cap, cap)]
    for t in targets:
        if t is not None:                    # settle: draws `active` again, and its count (k = 1) makes next = t
            pairs.append((active, active))
            nxt = t
        else:
            nxt = cap
        pairs.append((active, nxt))
        active = nxt
    return pairs


def track_cloud(cap, dtype, utime, seed=None):
    """A converged cloud around TRACK_START (equal weights), as tests/test_gpu_uploaded_weights.py's."""
    rng = np.random.default_rng(cap if seed is None else seed)
    p = np.zeros(cap, dtype)
    p["x"] = (TRACK_START[0] + 0.02 * rng.standard_normal(cap)).astype(np.float32)
    p["y"] = (TRACK_START[1] + 0.02 * rng.standard_normal(cap)).astype(np.float32)
    p["theta"] = (TRACK_START[2] + 0.05 * rng.standard_normal(cap)).astype(np.float32)
    for f in ("x", "y", "theta"):
        p["p_" + f] = p[f]
    p["utime"] = p["p_utime"] = int(utime)
    p["weight"] = 1.0 / cap
    return p


# ---------------------------------------------------------------- the map and the scan of the count and all-floor tests
FREE_SIDE, FREE_MPC = 200, np.float32(0.05)
FREE_ORIGIN = (np.float32(-5.0), np.float32(-5.0))


def free_map():
    """200 x 200 cells, all free (log-odds -60): every likelihood on it is 0, every weight the floor."""
    return np.full((FREE_SIDE, FREE_SIDE), -60, np.int8)


def short_scan(t_end_us, rays=64, rng_m=1.0, ray_dt_us=345):
    """(ranges, thetas, times, utime) of a scan of 64 one-metre rays, thetas 2 pi i / rays, times ending at t_end_us."""
    i = np.arange(rays)
    thetas = (2.0 * np.pi * i / rays).astype(np.float32)
    times = (t_end_us - (rays - 1 - i) * ray_dt_us).astype(np.int64)
    return np.full(rays, rng_m, np.float32), thetas, times, int(t_end_us)


FLOOR_CAP, FLOOR_ACTIVE, FLOOR_NEXT = 4096, 300, 777     # C: 4096 -> 300, all-floor updates at 300, then 300 -> 777 -> 4096


def travel_scans():
    """The two scans of the free-map tests and the odometry they end at: the filter goes back and forth between the two poses."""
    from botlab_amd.host import LidarScan
    scans = [LidarScan(*short_scan(1_100_000)), LidarScan(*short_scan(1_200_000))]
    odo = [TRACK_START, (TRACK_START[0] + 0.02, TRACK_START[1], TRACK_START[2])]
    return scans, odo


def floor_update(oracle, opf):
    """On the reference filter opf: latch the odometry, then one moved update with the short scan on the all-free map (drawn with MID:
    the identity on equal weights); the result of the moved update."""
    scans, odo = travel_scans()
    args = (free_map(), FREE_MPC, np.float32(1.0 / np.float64(FREE_MPC)), FREE_ORIGIN)
    assert not opf.update(oracle.pose(*odo[0], utime=scans[0].utime), scans[0], *args, 1)["moved"]
    res = opf.update(oracle.pose(*odo[1], utime=scans[1].utime), scans[1], *args, MID)
    assert res["moved"]
    return res


def serial_floor_weight(n):
    """computeNormalizedPosterior on n floor weights: 0.001 / (0.001 + 0.001 + ..., n terms, added in sequence)."""
    s = 0.0
    for _ in range(n):
        s += 0.001
    return 0.001 / s
