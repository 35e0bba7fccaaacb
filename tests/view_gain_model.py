"""The model of the view gain (include/botlab_hip.h, "view gain") and of plan_path_to_frontier_by_gain, restated in numpy: the
definition the HIP kernel is checked against for equality.  Everything is integers apart from the ray table, which is formed in
double with the C library's cos, sin and lround -- the ones the library's host code calls.

  ray_ends        the end offset of every ray
  walk            the Bresenham walk of the definition from (0, 0) to one end offset
  walks           the walks of a whole table, padded to one array (the walk is relative: the same for every candidate)
  seen_mask       THE MODEL: the seen set of one candidate as a (2R + 1)^2 window, vectorised over rays x steps
  gain / gains    the number of cells in it
  window_bound    the number of unknown cells in the window (gain can never exceed it)
  partially_explored, frontier_cells, near_frontier_candidates   test inputs: a map known only around one spot, and the cells
                  near its known/unknown border
  choose          the planner's choice (plan_path_to_frontier_by_gain) from nav_field_model's costs, traversability and labels
"""
import ctypes
import ctypes.util
import math

import numpy as np

import nav_field_model as nm

_libm = ctypes.CDLL(ctypes.util.find_library("m"))
_libm.cos.restype = ctypes.c_double
_libm.cos.argtypes = [ctypes.c_double]
_libm.sin.restype = ctypes.c_double
_libm.sin.argtypes = [ctypes.c_double]
_libm.lround.restype = ctypes.c_long
_libm.lround.argtypes = [ctypes.c_double]


class Params:
    def __init__(self, radius_cells=60, n_rays=360, occupied_above=0, unknown_lo=0, unknown_hi=0):
        self.radius_cells, self.n_rays = int(radius_cells), int(n_rays)
        self.occupied_above, self.unknown_lo, self.unknown_hi = int(occupied_above), int(unknown_lo), int(unknown_hi)


def ray_ends(radius_cells, n_rays):
    out = np.zeros((n_rays, 2), np.int32)
    for k in range(n_rays):
        t = 2.0 * math.pi * float(k) / float(n_rays)
        out[k] = (_libm.lround(float(radius_cells) * _libm.cos(t)), _libm.lround(float(radius_cells) * _libm.sin(t)))
    return out


def walk(ex, ey):
    """The cells of the line from (0, 0) to (ex, ey), start excluded, end included."""
    ex, ey = int(ex), int(ey)
    dx, dy = abs(ex), abs(ey)
    sx, sy = (ex > 0) - (ex < 0), (ey > 0) - (ey < 0)
    err, x, y = dx - dy, 0, 0
    out = []
    while (x, y) != (ex, ey):
        e2 = 2 * err
        if e2 >= -dy:
            err -= dy
            x += sx
        if e2 <= dx:
            err += dx
            y += sy
        out.append((x, y))
        assert len(out) <= dx + dy
    return out


def walks(ends):
    """(ox, oy, valid), each (rays, longest walk): the offsets every ray visits, in order."""
    lines = [walk(ex, ey) for ex, ey in ends]
    n = max([len(l) for l in lines] + [1])
    ox, oy = np.zeros((len(lines), n), np.int64), np.zeros((len(lines), n), np.int64)
    valid = np.zeros((len(lines), n), bool)
    for k, l in enumerate(lines):
        if l:
            a = np.array(l, np.int64)
            ox[k, :len(l)], oy[k, :len(l)], valid[k, :len(l)] = a[:, 0], a[:, 1], True
    return ox, oy, valid


def seen_mask(cells, p, w_table, x, y):
    """THE MODEL.  (2R + 1, 2R + 1) uint8, 0 / 1: the seen set of the candidate (x, y) in the window around it."""
    h, w = cells.shape
    r = p.radius_cells
    out = np.zeros((2 * r + 1, 2 * r + 1), np.uint8)
    if not (0 <= x < w and 0 <= y < h):
        return out
    ox, oy, valid = w_table
    gx, gy = x + ox, y + oy
    inside = (gx >= 0) & (gx < w) & (gy >= 0) & (gy < h)
    v = cells[np.clip(gy, 0, h - 1), np.clip(gx, 0, w - 1)].astype(np.int64)
    stop = valid & (~inside | (v > p.occupied_above))
    alive = valid & ~np.logical_or.accumulate(stop, axis=1)
    seen = alive & (v >= p.unknown_lo) & (v <= p.unknown_hi)
    out[oy[seen] + r, ox[seen] + r] = 1
    return out


def gain(cells, p, w_table, x, y):
    return int(seen_mask(cells, p, w_table, x, y).sum())


def gains(cells, p, cands, ends=None):
    """uint32 gain of every candidate (x, y); `ends`: the ray table to use (default: ray_ends of p)."""
    w_table = walks(ray_ends(p.radius_cells, p.n_rays) if ends is None else ends)
    return np.array([gain(cells, p, w_table, int(x), int(y)) for x, y in cands], np.uint32)


def window_bound(cells, p, x, y):
    """The unknown cells in the (2R + 1)^2 window around (x, y), the cell itself left out: no gain exceeds it."""
    h, w = cells.shape
    r = p.radius_cells
    x0, x1, y0, y1 = max(x - r, 0), min(x + r, w - 1), max(y - r, 0), min(y + r, h - 1)
    if x0 > x1 or y0 > y1:
        return 0
    win = cells[y0:y1 + 1, x0:x1 + 1].astype(np.int64)
    unk = (win >= p.unknown_lo) & (win <= p.unknown_hi)
    n = int(unk.sum())
    if 0 <= x < w and 0 <= y < h and unk[y - y0, x - x0]:
        n -= 1
    return n


# ------------------------------------------------------------------------------------------------------------ test inputs
def partially_explored(cells, keep=30):
    """The map as known from one spot: every cell farther (Euclidean) than `keep` cells from a free cell near the median of the free
    cells is set to 0 (unknown).  Returns (cells, (x, y) of that free cell)."""
    ys, xs = np.nonzero(cells < 0)
    mx, my = np.median(xs), np.median(ys)
    k = int(np.argmin((xs - mx) ** 2 + (ys - my) ** 2))
    cx, cy = int(xs[k]), int(ys[k])
    yy, xx = np.ogrid[:cells.shape[0], :cells.shape[1]]
    return np.where((xx - cx) ** 2 + (yy - cy) ** 2 <= keep * keep, cells, 0).astype(np.int8), (cx, cy)


def frontier_cells(cells):
    """(n, 2) x, y in row-major order: the unknown cells (log-odds 0) with a free 4-neighbour (log-odds < 0)."""
    h, w = cells.shape
    pad = np.full((h + 2, w + 2), 127, np.int64)
    pad[1:-1, 1:-1] = cells
    free = (pad[:-2, 1:-1] < 0) | (pad[2:, 1:-1] < 0) | (pad[1:-1, :-2] < 0) | (pad[1:-1, 2:] < 0)
    ys, xs = np.nonzero((cells == 0) & free)
    return np.stack([xs, ys], axis=1).astype(np.int64)


def two_frontier_map():
    """A 200 x 200 map (5 cm cells, origin (-5, -5)) on which the cheapest frontier is not the most informative one: a free room
    x 60..139, y 80..119 in occupied space, a dead-end niche of unknown cells (x 50..59, y 94..105) in its left wall and the whole
    right wall open onto an unmapped hall (x 140..199, y 40..159).  The robot stands at cell (70, 100), a few steps from the niche.
    Returns (cells, origin, metres per cell, robot cell)."""
    cells = np.full((200, 200), 100, np.int8)
    cells[80:120, 60:140] = -100
    cells[94:106, 50:60] = 0
    cells[40:160, 140:200] = 0
    return cells, (np.float32(-5.0), np.float32(-5.0)), np.float32(0.05), (70, 100)


def near_frontier_candidates(cells, reach=3):
    """(n, 2) x, y in row-major order: the free cells within Chebyshev distance `reach` of a frontier cell."""
    h, w = cells.shape
    near = np.zeros((h, w), bool)
    for x, y in frontier_cells(cells):
        near[max(y - reach, 0):y + reach + 1, max(x - reach, 0):x + reach + 1] = True
    ys, xs = np.nonzero(near & (cells < 0))
    return np.stack([xs, ys], axis=1).astype(np.int64)


# ------------------------------------------------------------------------------------------------------------ the planner
def choose(cells, l1, trav, pen, robot_cell, frontier_xy, owner, reach, p, ends=None, stride=1, min_gain=1, gain_weight=1):
    """plan_path_to_frontier_by_gain's choice.  frontier_xy: the frontier cells in order, owner[i] the frontier cell i belongs to.
    Returns None when no candidate survives, else dict(cell=(x, y), frontier, gain, cost, candidates, field) -- field: the
    navigation field rooted at the robot's cell."""
    tcell, _ = nm.cell_tables(l1, trav, pen)
    h, w = tcell.shape
    if robot_cell is None:
        return None
    field = nm.dijkstra(l1, trav, pen, [robot_cell], 0)
    mask, label = nm.goal_set(tcell, frontier_xy, reach)                      # traversable, within reach; lowest frontier cell
    ys, xs = np.nonzero(mask & (field != nm.UNREACHED))
    sel = (xs % stride == 0) & (ys % stride == 0)
    xs, ys = xs[sel], ys[sel]
    if len(xs) == 0:
        return None
    g = gains(cells, p, np.stack([xs, ys], axis=1), ends).astype(np.int64)
    best = None
    for i in range(len(xs)):
        if g[i] < min_gain:
            continue
        cost = int(field[ys[i], xs[i]])
        key = (-(int(gain_weight) * int(g[i]) - cost), cost, int(ys[i]), int(xs[i]))
        if best is None or key < best[0]:
            best = (key, i)
    if best is None:
        return None
    i = best[1]
    return dict(cell=(int(xs[i]), int(ys[i])), frontier=int(owner[int(label[ys[i], xs[i]])]), gain=int(g[i]), cost=int(field[ys[i], xs[i]]),
                candidates=len(xs), field=field)
