"""The model of the beam sensor model: a numpy restatement of the definition in include/botlab_hip.h ("beam model"), which the HIP
kernels of botlab_amd/csrc/bl_beam.hip must reproduce value for value: first, K, z, z* and p of every used ray, the score of every
pose and the weight units.

The geometry is the obstacle layer's (scan_match_model.endpoints at heading step 0, grid_position); the walk is the reference's
Bresenham variant in its closed form (obstacle_layer_model.walk), start cell included, end cell excluded, carried on to the far cell.
Behind the end cells everything is an exact integer.  The one floating-point step -- the tables -- is make_tables(), compared on its
own against bl_beam_tables; cast() and scores() take whichever tables they are given.
"""
import math

import numpy as np

from scan_match_model import MIN_RANGE, endpoints, grid_position

F32 = np.float32
MAX_RAYS = 4096
MAX_REACH_CELLS = 4096
OFF_GRID = -2 ** 63
TWO30 = 1073741824.0
DEFAULTS = dict(max_range=5.0, occ_min=1, sigma_cells=1.0, z_hit=0.7, z_short=0.1, z_max=0.05, z_rand=0.15, lam=0.1,
                blocked_factor=0.1, hit_cut=64, span=1 << 22, ray_stride=1)


class ArgError(Exception):
    """What the library answers with BL_ERR_ARG."""


def _lround(x):
    return int(math.floor(x + 0.5)) if x >= 0 else -int(math.floor(-x + 0.5))


def params(**kw):
    """DEFAULTS with the float members narrowed to float32, as bl_beam_params_t holds them."""
    p = dict(DEFAULTS, **kw)
    for k in ("max_range", "sigma_cells", "z_hit", "z_short", "z_max", "z_rand", "lam", "blocked_factor"):
        p[k] = float(F32(p[k]))
    return p


def params_ok(p):
    """bl_beam_set_params' rule.  The three floors are asked of the values before their max(1, .): Rand at the largest legal reach."""
    f = [p[k] for k in ("max_range", "sigma_cells", "z_hit", "z_short", "z_max", "z_rand", "lam", "blocked_factor")]
    if not all(math.isfinite(v) for v in f):
        return False
    if not (F32(p["max_range"]) > MIN_RANGE and p["sigma_cells"] > 0 and min(f[2:]) >= 0):
        return False
    if not (1 <= p["occ_min"] <= 127 and 1 <= p["hit_cut"] <= 1023 and 0 < p["span"] <= 2 ** 40 and 1 <= p["ray_stride"] <= 64):
        return False
    if max(TWO30 * p["z_hit"], TWO30 * p["z_short"] * p["lam"], TWO30 * p["z_rand"], TWO30 * p["z_max"],
           TWO30 * p["z_max"] * p["blocked_factor"]) > 2.0 ** 31:
        return False
    if _lround(TWO30 * p["z_rand"] / 4096.0) < 1 or _lround(TWO30 * p["z_max"]) < 1 or _lround(TWO30 * p["z_max"] * p["blocked_factor"]) < 1:
        return False                                                        # some p could be 0
    top = _lround(TWO30 * p["z_hit"]) + _lround(TWO30 * p["z_short"] * p["lam"]) + _lround(TWO30 * p["z_rand"])
    return max(top, _lround(TWO30 * p["z_max"]), _lround(TWO30 * p["z_max"] * p["blocked_factor"])) <= 2 ** 31 - 1


def reach_cells(p, cpm):
    return math.ceil(float(F32(p["max_range"])) * float(F32(cpm)))


def make_tables(p, cpm):
    """The tables of bl_beam_tables for a map of cells_per_meter cpm, in double."""
    reach = reach_cells(p, cpm)
    if not reach <= MAX_REACH_CELLS:
        raise ArgError("reach")
    s = p["sigma_cells"]
    hit = [_lround(TWO30 * p["z_hit"] * math.exp(-((d / 4.0) * (d / 4.0)) / (2.0 * s * s))) for d in range(1024)]
    short = [_lround(TWO30 * p["z_short"] * p["lam"] * math.exp(-p["lam"] * c)) for c in range(1024)]
    lt = [_lround(65536.0 * math.log(1.0 + i / 256.0)) for i in range(256)]
    return dict(hit=np.array(hit, np.uint32), short=np.array(short, np.uint32), lt=np.array(lt, np.uint32),
                rand=max(1, _lround(TWO30 * p["z_rand"] / reach)), max_free=max(1, _lround(TWO30 * p["z_max"])),
                max_blocked=max(1, _lround(TWO30 * p["z_max"] * p["blocked_factor"])), ln2=_lround(65536.0 * math.log(2.0)), reach=reach)


def unit_table():
    """U[0 .. 256] of bl_beam_unit_table."""
    return np.array([max(1, _lround(1048576.0 * math.pow(2.0, -20.0 * j / 256.0))) for j in range(257)], np.uint32)


def lg(p, t):
    """The integer logarithm (Q16 nats) of uint32 p >= 1, elementwise."""
    p = np.asarray(p, dtype=np.int64)
    assert p.min(initial=1) >= 1 and p.max(initial=1) < 2 ** 31
    e = np.zeros(p.shape, np.int64)
    for b in range(1, 31):
        e[p >= (1 << b)] = b
    mant = (((p << (31 - e)) & 0xFFFFFFFF) >> 23) & 255
    return (e - 30) * int(t["ln2"]) + t["lt"].astype(np.int64)[mant]


def isqrt(v):
    """floor(sqrt(v)) of non-negative int64, elementwise and exact."""
    v = np.asarray(v, dtype=np.int64)
    r = np.floor(np.sqrt(v.astype(np.float64))).astype(np.int64)
    r = np.where(r * r > v, r - 1, r)
    return np.where((r + 1) * (r + 1) <= v, r + 1, r)


def quarter(ax, ay, bx, by):
    return isqrt(16 * ((ax - bx) ** 2 + (ay - by) ** 2))


def used_rays(ranges, thetas, p):
    """(ranges, thetas, is_max) of the used rays: the non-dropped ones in scan order, every ray_stride-th from the first."""
    ranges = np.asarray(ranges, dtype=np.float32)
    thetas = np.asarray(thetas, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        keep = np.isfinite(ranges) & (ranges > MIN_RANGE)
    r, t = ranges[keep][::p["ray_stride"]], thetas[keep][::p["ray_stride"]]
    if len(r) > MAX_RAYS:
        raise ArgError("rays")
    return r, t, r >= F32(p["max_range"])


def pose_start(pose, origin, cpm, w, h):
    """The start cell, or None for a pose that scores OFF_GRID."""
    pose = tuple(F32(v) for v in pose)
    if not all(math.isfinite(float(v)) for v in pose):
        return None
    px, py = grid_position(pose[0], pose[1], origin, F32(cpm))
    if not (abs(float(px)) < 2.0 ** 30 and abs(float(py)) < 2.0 ** 30):
        return None
    sx, sy = int(np.trunc(px)), int(np.trunc(py))
    return (sx, sy) if 0 <= sx < w and 0 <= sy < h else None


def window(box, reach, W, H):
    """(x0, y0, w, h) of the window a workgroup stages: the bounding box (x0, y0, x1, y1) of its start cells widened by reach + 2 and
    clipped to the W x H grid, the left edge rounded down and the width up to a multiple of 4 (the rows are copied as words when W is
    one; a column at or beyond W holds 0).  It is staged when w * h <= window_bytes.  No result depends on it, only the path."""
    pad = reach + 2
    x0 = max(box[0] - pad, 0) & ~3
    y0 = max(box[1] - pad, 0)
    w = ((min(box[2] + pad, W - 1) - x0 + 1) + 3) & ~3
    h = min(box[3] + pad, H - 1) - y0 + 1
    return x0, y0, w, h


def cast(cells, origin, cpm, rays, pose, p, t):
    """Per used ray of one pose: first, K, z, zstar, p (int64 each; -1, -1, -1, -1, 0 for a ray dropped by `has`; z = -1 for a max
    reading, zstar = -1 without an expected hit), or None for an off-grid pose.  rays = used_rays(...)."""
    cells = np.asarray(cells)
    h, w = cells.shape
    s = pose_start(pose, origin, cpm, w, h)
    if s is None:
        return None
    r, th, is_max = rays
    n = len(r)
    pose = tuple(F32(v) for v in pose)
    ex, ey, has_e = endpoints(r, th, pose, 0, F32(0), origin, cpm)
    mx, my, has_m = endpoints(np.full(n, F32(p["max_range"]), np.float32), th, pose, 0, F32(0), origin, cpm)
    ok = has_m & (has_e | is_max)
    dx, dy = np.abs(mx - s[0]), np.abs(my - s[1])
    stx, sty = np.where(s[0] < mx, 1, -1), np.where(s[1] < my, 1, -1)
    K = np.maximum(dx, dy)
    kmax = int(K[ok].max(initial=0))
    k = np.arange(max(kmax, 1), dtype=np.int64)[None, :]
    xmaj = (dx >= dy)[:, None]
    dmaj, dmin = np.maximum(np.maximum(dx, dy), 1)[:, None], np.minimum(dx, dy)[:, None]
    minor = (2 * k * dmin + dmaj) // (2 * dmaj)
    xs = s[0] + stx[:, None] * np.where(xmaj, k, minor)
    ys = s[1] + sty[:, None] * np.where(xmaj, minor, k)
    inside = (xs >= 0) & (xs < w) & (ys >= 0) & (ys < h) & (k < K[:, None])
    occ = np.zeros(xs.shape, bool)
    occ[inside] = cells[ys[inside], xs[inside]] >= p["occ_min"]
    any_hit = occ.any(axis=1)
    first = np.where(any_hit, occ.argmax(axis=1), K)
    rows = np.arange(n)
    fi = np.minimum(first, max(kmax, 1) - 1)
    zstar = np.where(any_hit, quarter(xs[rows, fi], ys[rows, fi], s[0], s[1]), -1)
    z = np.where(is_max, -1, quarter(ex, ey, s[0], s[1]))
    hit = t["hit"].astype(np.int64)[np.minimum(np.abs(z - zstar), p["hit_cut"])]
    short = t["short"].astype(np.int64)[np.minimum(np.maximum(z, 0) >> 2, 1023)]
    p_ret = np.where(any_hit, hit, 0) + np.where(~any_hit | (z < zstar), short, 0) + int(t["rand"])
    pv = np.where(is_max, np.where(any_hit, int(t["max_blocked"]), int(t["max_free"])), p_ret)
    out = dict(first=first, K=K, z=z, zstar=zstar, p=pv)
    for name, dropped in (("first", -1), ("K", -1), ("z", -1), ("zstar", -1), ("p", 0)):
        out[name] = np.where(ok, out[name], dropped).astype(np.int64)
    return out


def scores(cells, origin, cpm, ranges, thetas, poses, p, t):
    """int64 [n]: S of every pose (OFF_GRID for the poses that take no part)."""
    rays = used_rays(ranges, thetas, p)
    out = np.empty(len(poses), np.int64)
    for i, pose in enumerate(poses):
        c = cast(cells, origin, cpm, rays, pose, p, t)
        out[i] = OFF_GRID if c is None else int(lg(c["p"][c["p"] > 0], t).sum())
    return out


def units(S, span, U=None):
    """uint32 [n]: the weight units of the scores S."""
    U = unit_table() if U is None else U
    S = np.asarray(S, dtype=np.int64)
    on = S != OFF_GRID
    out = np.ones(len(S), np.uint32)
    if on.any():
        smax = int(S[on].max())
        j = [min(256, ((smax - int(v)) * 256) // int(span)) for v in S[on]]
        out[on] = U[np.array(j, np.int64)]
    return out
