"""The model of path shortcutting (include/botlab_hip.h, "path shortcutting"), restated in Python integers and numpy: the definition
the HIP kernels are checked against, byte for byte.

  ok_table        ok per L1 distance n, from the distance table of nav_field_model
  ok_cells        ok per cell
  cover           the cells of cover(a, b), by the formula over the bounding box (plain Python: the definition as written)
  length          L: math.isqrt
  isqrt_np        the same for int64 arrays (a float root put right by integer compares; checked against math.isqrt by the tests)
  visible         vis[j, s]: (j - s, j) is an edge -- numpy over all j of one span, the formula evaluated per major step
  shortcut        THE MODEL: (kept indices, cost, input cost) of one path of cells
  shortcut_poses  the pose form
"""
import math

import numpy as np

import nav_field_model as nm

MAX_POINTS = 8192
MAX_PATHS = 4096
MAX_WAYPOINT_COST = 1 << 20
WINDOW_BYTES = 64 * 1024


class Params:
    def __init__(self, clearance=0.2, max_span=64, waypoint_cost=1024):
        self.clearance = float(clearance)
        self.max_span = int(max_span)
        self.waypoint_cost = int(waypoint_cost)

    def valid(self):
        return (math.isfinite(self.clearance) and 1 <= self.max_span <= MAX_POINTS and 0 <= self.waypoint_cost <= MAX_WAYPOINT_COST)


def ok_table(f, clearance):
    return np.array([1 if float(f[n]) > float(clearance) * 1.000001 else 0 for n in range(len(f))], np.uint8)


def ok_cells(l1, okt):
    idx = np.minimum(l1.astype(np.int64), len(okt) - 1)
    return (l1 != nm.NONE16) & (okt[idx] != 0)


def ok_of_map(cells, clearance):
    """ok per cell of a map of log-odds cells."""
    h, w = cells.shape
    return ok_cells(nm.l1_distances(cells), ok_table(nm.dist_table(w, h), clearance))


def cover(dx, dy):
    """The offsets (u, v) of cover((0, 0), (dx, dy))."""
    out = []
    for v in range(min(0, dy), max(0, dy) + 1):
        for u in range(min(0, dx), max(0, dx) + 1):
            if 2 * abs(u * dy - v * dx) <= abs(dx) + abs(dy):
                out.append((u, v))
    return out


def length(dx, dy):
    return math.isqrt((dx * dx + dy * dy) << 20)


def isqrt_np(a):
    a = np.asarray(a, np.int64)
    r = np.floor(np.sqrt(a.astype(np.float64))).astype(np.int64)
    for _ in range(4):
        r = r - (r * r > a)
        r = r + ((r + 1) * (r + 1) <= a)
    return r


def length_np(dx, dy):
    dx, dy = np.asarray(dx, np.int64), np.asarray(dy, np.int64)
    return isqrt_np((dx * dx + dy * dy) << 20)


def window_staged(cells_xy):
    """The window rule of one path: its bounding box's ok bits, rows padded to 32 bits, fit WINDOW_BYTES."""
    q = np.asarray(cells_xy, np.int64).reshape(-1, 2)
    if len(q) == 0:
        return True
    bw, bh = int(q[:, 0].max() - q[:, 0].min()) + 1, int(q[:, 1].max() - q[:, 1].min()) + 1
    return ((bw + 31) // 32 * 4) * bh <= WINDOW_BYTES


def _pairs_ok(okc, xa, ya, xb, yb):
    """Per pair: every cell of cover(a, b) is ok.  Major axis t = 0 .. A, minor w = 0 .. B from a towards b: the cell (t, w) is in the
    cover iff 2 |t B - w A| <= A + B and it is inside the bounding box; per t every w near t B / A is put to that test.  (Pairs that
    have failed, or have reached their end, leave the arrays: this only saves time.)"""
    dx, dy = xb - xa, yb - ya
    adx, ady = np.abs(dx), np.abs(dy)
    xmaj = adx >= ady
    A, B = np.where(xmaj, adx, ady), np.where(xmaj, ady, adx)
    sx, sy = np.where(dx < 0, -1, 1), np.where(dy < 0, -1, 1)
    good = np.ones(len(xa), bool)
    idx = np.arange(len(xa))
    for t in range(int(A.max(initial=0)) + 1):
        idx = idx[good[idx] & (t <= A[idx])]
        if len(idx) == 0:
            break
        a_, b_, xm = A[idx], B[idx], xmaj[idx]
        centre = (t * b_) // np.maximum(a_, 1)
        for k in (-1, 0, 1, 2):
            w = centre + k
            inside = (w >= 0) & (w <= b_) & (2 * np.abs(t * b_ - w * a_) <= a_ + b_)
            x = np.where(xm, xa[idx] + sx[idx] * t, xa[idx] + sx[idx] * w)
            y = np.where(xm, ya[idx] + sy[idx] * w, ya[idx] + sy[idx] * t)
            x, y = np.where(inside, x, xa[idx]), np.where(inside, y, ya[idx])
            good[idx] &= ~inside | okc[y, x]
    return good


def visible(okc, cells_xy, max_span):
    """vis[j, s] for s = 0 .. S, S = min(max_span, m - 1): (j - s, j) is an edge."""
    q = np.asarray(cells_xy, np.int64).reshape(-1, 2)
    m = len(q)
    S = max(min(int(max_span), m - 1), 0)
    vis = np.zeros((m, S + 1), bool)
    if S >= 1:
        vis[1:, 1] = True
    if S >= 2:
        jj = np.concatenate([np.arange(s, m) for s in range(2, S + 1)])
        ss = np.concatenate([np.full(m - s, s) for s in range(2, S + 1)])
        a, b = q[jj - ss], q[jj]
        vis[jj, ss] = _pairs_ok(okc, a[:, 0], a[:, 1], b[:, 0], b[:, 1])
    return vis


def visible_matrix(okc, cells_xy, max_span):
    """uint8 [m, m]: [j, i] = 1 iff (i, j) is an edge (what bl_shortcut_debug_visible returns)."""
    vis = visible(okc, cells_xy, max_span)
    m = vis.shape[0]
    out = np.zeros((m, m), np.uint8)
    for s in range(1, vis.shape[1]):
        j = np.arange(s, m)
        out[j, j - s] = vis[s:, s]
    return out


def dp(xy, vis, waypoint_cost):
    """(cost[], pred[]) over the edges of vis[j, s]."""
    q = np.asarray(xy, np.int64).reshape(-1, 2)
    m = len(q)
    cost = np.zeros(m, np.int64)
    pred = np.zeros(m, np.int64)
    S = vis.shape[1] - 1
    for j in range(1, m):
        lo = max(j - S, 0)
        i = np.arange(lo, j)                                         # ascending: argmin takes the smallest i of a tie
        e = vis[j, j - i]
        c = cost[lo:j] + length_np(q[j, 0] - q[lo:j, 0], q[j, 1] - q[lo:j, 1]) + waypoint_cost
        c = np.where(e, c, np.iinfo(np.int64).max)
        k = int(np.argmin(c))
        cost[j], pred[j] = c[k], i[k]
    return cost, pred


def shortcut(okc, cells_xy, p):
    """THE MODEL.  (kept indices as int32, cost, input cost)."""
    q = np.asarray(cells_xy, np.int64).reshape(-1, 2)
    m = len(q)
    assert p.valid() and m <= MAX_POINTS
    h, w = okc.shape
    assert m == 0 or (q[:, 0].min() >= 0 and q[:, 0].max() < w and q[:, 1].min() >= 0 and q[:, 1].max() < h)
    if m <= 1:
        return np.arange(m, dtype=np.int32), 0, 0
    cost, pred = dp(q, visible(okc, q, p.max_span), p.waypoint_cost)
    keep = [m - 1]
    while keep[-1] > 0:
        keep.append(int(pred[keep[-1]]))
    d = np.diff(q, axis=0)
    in_cost = int(length_np(d[:, 0], d[:, 1]).sum()) + (m - 1) * p.waypoint_cost
    return np.array(keep[::-1], np.int32), int(cost[m - 1]), in_cost


def pose_cells(poses, origin, cpm, w, h):
    """The cells of a POSE array, or None if a pose is off the grid."""
    out = []
    for k in range(len(poses)):
        c = nm.pose_cell((poses["x"][k], poses["y"][k]), origin, cpm, w, h)
        if c is None:
            return None
        out.append(c)
    return np.array(out, np.int64).reshape(-1, 2)


def shortcut_poses(okc, poses, origin, cpm, p):
    """The pose form: (kept poses as a POSE array, cost, input cost)."""
    h, w = okc.shape
    q = pose_cells(poses, origin, cpm, w, h)
    assert q is not None
    keep, cost, in_cost = shortcut(okc, q, p)
    out = poses[keep].copy()
    for s in range(1, len(keep)):
        dx, dy = int(q[keep[s], 0] - q[keep[s - 1], 0]), int(q[keep[s], 1] - q[keep[s - 1], 1])
        if dx or dy:
            out["theta"][s] = np.float32(math.atan2(float(dy), float(dx)))
    return out, cost, in_cost
