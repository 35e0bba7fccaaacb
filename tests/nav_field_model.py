"""The model of the navigation field (include/botlab_hip.h, "navigation field"), restated in Python: the definition the HIP kernels
are checked against, bit for bit.  Everything here is integers apart from the two per-distance tables, which are formed in double
with math.pow -- the libm the library's host code calls.

  l1_distances     n(c): integer L1 distance to the nearest cell with log-odds >= 0 (0xFFFF: the map has none)
  dist_table       f[n] = f[n - 1] + 0.1f, the float a distance grid shows at L1 distance n
  tables           traversable(n), penalty(n)
  goal_set         the goal mask and labels of a list of goal cells and a reach
  dijkstra         THE MODEL: a textbook heap Dijkstra from the goal set
  tile_fixed_point a second, independent implementation that mimics the device's schedule (numpy sweeps over 32 x 32 tiles with
                   a one-cell halo, to a fixed point, in a given tile order)
  certificate      a vectorised Bellman check of a field: None when it is THE solution, else what is wrong
  descend          the path from a start pose
"""
import ctypes
import ctypes.util
import heapq
import math

import numpy as np

UNREACHED = 0xFFFFFFFF
NONE16 = 0xFFFF
TILE = 32
# the moves in the order ties break by
MOVES = [(1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, 1), (1, -1), (-1, -1)]
STEP = [10, 10, 10, 10, 14, 14, 14, 14]
_libm = ctypes.CDLL(ctypes.util.find_library("m"))
_libm.atan2f.restype = ctypes.c_float
_libm.atan2f.argtypes = [ctypes.c_float, ctypes.c_float]
THETA = [np.float32(_libm.atan2f(float(dy), float(dx))) for dx, dy in MOVES]      # the C library's atan2f, as the library's host code calls it


class Params:
    def __init__(self, minDistanceToObstacle=0.2, maxDistanceWithCost=2.0, distanceCostExponent=1.0, obstacle_gain=50, reach_cells=0):
        self.minDistanceToObstacle = float(minDistanceToObstacle)
        self.maxDistanceWithCost = float(maxDistanceWithCost)
        self.distanceCostExponent = float(distanceCostExponent)
        self.obstacle_gain = int(obstacle_gain)
        self.reach_cells = int(reach_cells)


def l1_distances(cells):
    """Two-pass L1 distance transform; sources are the cells with log-odds >= 0 (obstacle_distance_grid.cpp:100-118)."""
    h, w = cells.shape
    big = 1 << 28
    d = np.where(cells >= 0, 0, big).astype(np.int64)
    for x in range(1, w):
        d[:, x] = np.minimum(d[:, x], d[:, x - 1] + 1)
    for x in range(w - 2, -1, -1):
        d[:, x] = np.minimum(d[:, x], d[:, x + 1] + 1)
    for y in range(1, h):
        d[y] = np.minimum(d[y], d[y - 1] + 1)
    for y in range(h - 2, -1, -1):
        d[y] = np.minimum(d[y], d[y + 1] + 1)
    return np.where(d >= big, NONE16, d).astype(np.uint16)


def dist_table(w, h):
    f = np.zeros(w + h + 1, np.float32)
    for n in range(1, len(f)):
        f[n] = np.float32(f[n - 1] + np.float32(0.1))
    return f


def tables(f, p):
    trav = np.zeros(len(f), np.uint8)
    pen = np.zeros(len(f), np.int32)
    min_d, max_d = p.minDistanceToObstacle, p.maxDistanceWithCost
    for n in range(len(f)):
        d = float(f[n])
        if not d > min_d * 1.000001:
            continue
        trav[n] = 1
        if d >= max_d or max_d <= min_d:
            continue
        pen[n] = int(math.floor(p.obstacle_gain * math.pow((max_d - d) / (max_d - min_d), p.distanceCostExponent)))
    return trav, pen


def cell_tables(l1, trav, pen):
    """Per cell: traversable (bool) and penalty (int64)."""
    idx = np.minimum(l1.astype(np.int64), len(trav) - 1)
    t = (l1 != NONE16) & (trav[idx] != 0)
    return t, np.where(t, pen[idx], 0).astype(np.int64)


def goal_set(tcell, goals, reach):
    """(mask, label): label = lowest index of a listed in-grid cell within Chebyshev distance `reach`, -1 off the goal set."""
    h, w = tcell.shape
    label = np.full((h, w), -1, np.int64)
    for k in range(len(goals) - 1, -1, -1):
        gx, gy = int(goals[k][0]), int(goals[k][1])
        if not (0 <= gx < w and 0 <= gy < h):
            continue
        label[max(gy - reach, 0):gy + reach + 1, max(gx - reach, 0):gx + reach + 1] = k
    label[~tcell] = -1
    return label >= 0, label


def allowed_moves(tcell):
    """allowed[m][y, x]: the move m from (x, y) stays in the grid, between traversable cells, and cuts no corner."""
    h, w = tcell.shape
    pad = np.zeros((h + 2, w + 2), bool)
    pad[1:-1, 1:-1] = tcell

    def sh(dx, dy):
        return pad[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    out = []
    for dx, dy in MOVES:
        a = tcell & sh(dx, dy)
        if dx and dy:
            a = a & sh(dx, 0) & sh(0, dy)
        out.append(a)
    return out


def dijkstra(l1, trav, pen, goals, reach):
    """THE MODEL.  uint32 field."""
    tcell, pcell = cell_tables(l1, trav, pen)
    h, w = tcell.shape
    mask, _ = goal_set(tcell, goals, reach)
    allowed = [a.ravel().tolist() for a in allowed_moves(tcell)]
    pc = pcell.ravel().tolist()
    inf = float("inf")
    dist = [inf] * (w * h)
    heap = []
    for i in np.flatnonzero(mask.ravel()).tolist():
        dist[i] = 0
        heap.append((0, i))
    heapq.heapify(heap)
    offs = [dy * w + dx for dx, dy in MOVES]
    while heap:
        d, i = heapq.heappop(heap)
        if d > dist[i]:
            continue
        for m in range(8):
            # the move i -> j is allowed exactly when j -> i is: the rule is symmetric
            if not allowed[m][i]:
                continue
            j = i + offs[m]
            nd = d + STEP[m] + pc[j]
            if nd < dist[j]:
                dist[j] = nd
                heapq.heappush(heap, (nd, j))
    out = np.array([UNREACHED if v == inf else v for v in dist], dtype=np.uint64).reshape(h, w)
    assert int(out[out != UNREACHED].max(initial=0)) < UNREACHED
    return out.astype(np.uint32)


def _best_via_moves(f, allowed, inf):
    """min over allowed moves of step + f(neighbour), inf where there is none; f int64 with inf for UNREACHED."""
    h, w = f.shape
    pad = np.full((h + 2, w + 2), inf, np.int64)
    pad[1:-1, 1:-1] = f
    best = np.full((h, w), inf, np.int64)
    for m, (dx, dy) in enumerate(MOVES):
        nb = pad[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
        cand = np.where(allowed[m] & (nb < inf), nb + STEP[m], inf)
        best = np.minimum(best, cand)
    return best


def tile_fixed_point(l1, trav, pen, goals, reach, order="forward", seed=0, tile=TILE):
    """The device's schedule on the CPU: rounds over a list of tiles; a tile is swept in place (with a one-cell halo of the
    neighbouring tiles' current values) until nothing in it changes, and lists the neighbouring tiles for the next round when a
    cell on the shared edge or corner got lower.  `order`: forward / reverse / random order of the tiles inside a round -- the
    result must not depend on it.  Returns (field, rounds)."""
    tcell, pcell = cell_tables(l1, trav, pen)
    h, w = tcell.shape
    mask, _ = goal_set(tcell, goals, reach)
    inf = np.int64(1) << 40
    f = np.where(mask, 0, inf).astype(np.int64)
    allowed = allowed_moves(tcell)
    tx_n, ty_n = (w + tile - 1) // tile, (h + tile - 1) // tile
    rng = np.random.default_rng(seed)
    todo = set()
    for y, x in zip(*np.nonzero(mask)):
        for oy in (-1, 0, 1):
            for ox in (-1, 0, 1):
                ux, uy = x // tile + ox, y // tile + oy
                if 0 <= ux < tx_n and 0 <= uy < ty_n:
                    todo.add((uy, ux))
    rounds = 0
    while todo:
        rounds += 1
        lst = sorted(todo)
        if order == "reverse":
            lst.reverse()
        elif order == "random":
            rng.shuffle(lst)
        nxt = set()
        for ty, tx in lst:
            y0, x0 = ty * tile, tx * tile
            y1, x1 = min(y0 + tile, h), min(x0 + tile, w)
            hy0, hx0, hy1, hx1 = max(y0 - 1, 0), max(x0 - 1, 0), min(y1 + 1, h), min(x1 + 1, w)
            sub = f[hy0:hy1, hx0:hx1].copy()
            sub_allowed = [a[hy0:hy1, hx0:hx1] for a in allowed]
            inner = np.zeros(sub.shape, bool)
            inner[y0 - hy0:y1 - hy0, x0 - hx0:x1 - hx0] = True
            psub = pcell[hy0:hy1, hx0:hx1]
            before = sub.copy()
            while True:
                best = _best_via_moves(sub, sub_allowed, inf)
                cand = np.where(best < inf, best + psub, inf)
                lower = inner & (cand < sub)
                if not lower.any():
                    break
                sub[lower] = cand[lower]
            got = sub[y0 - hy0:y1 - hy0, x0 - hx0:x1 - hx0]
            low = got < before[y0 - hy0:y1 - hy0, x0 - hx0:x1 - hx0]
            f[y0:y1, x0:x1] = got
            if low.any():
                edges = dict(w=low[:, 0].any(), e=low[:, -1].any() and x1 - x0 == tile, s=low[0, :].any(), n=low[-1, :].any() and y1 - y0 == tile)
                for oy in (-1, 0, 1):
                    for ox in (-1, 0, 1):
                        if (ox, oy) == (0, 0) or not (0 <= tx + ox < tx_n and 0 <= ty + oy < ty_n):
                            continue
                        if ox and oy:
                            hit = low[0 if oy < 0 else -1, 0 if ox < 0 else -1]
                        elif ox:
                            hit = edges["w"] if ox < 0 else edges["e"]
                        else:
                            hit = edges["s"] if oy < 0 else edges["n"]
                        if hit:
                            nxt.add((ty + oy, tx + ox))
        todo = nxt
    return np.where(f >= inf, UNREACHED, f).astype(np.uint32), rounds


def certificate(field, l1, trav, pen, goals, reach):
    """None iff `field` is the navigation field of these inputs: goal cells 0, every other reached cell satisfies the equation,
    cells that are not traversable are UNREACHED, and no UNREACHED traversable cell has an allowed move to a reached cell.
    (Steps cost at least 10, so a field that passes is the unique solution.)  Otherwise a description of the first thing wrong."""
    tcell, pcell = cell_tables(l1, trav, pen)
    mask, _ = goal_set(tcell, goals, reach)
    inf = np.int64(1) << 40
    f = np.where(field == UNREACHED, inf, field.astype(np.int64))
    if field.shape != l1.shape:
        return "shape"
    if (f[mask] != 0).any():
        return "a goal cell is not 0"
    if (f[~tcell] != inf).any():
        return "a cell that is not traversable is reached"
    best = _best_via_moves(f, allowed_moves(tcell), inf)
    want = np.where(best < inf, best + pcell, inf)
    rest = tcell & ~mask
    bad = rest & (f < inf) & (f != want)
    if bad.any():
        y, x = np.argwhere(bad)[0]
        return f"cell ({x}, {y}) holds {int(f[y, x])}, the equation gives {int(want[y, x])}"
    bad = rest & (f >= inf) & (best < inf)
    if bad.any():
        y, x = np.argwhere(bad)[0]
        return f"cell ({x}, {y}) is UNREACHED beside a reached cell"
    return None


def pose_cell(pose_xy, origin, cpm, w, h):
    """global_position_to_grid_cell of a pose (float32 x, y), or None off the grid."""
    vx = (float(np.float32(pose_xy[0])) - float(np.float32(origin[0]))) * float(np.float32(cpm))
    vy = (float(np.float32(pose_xy[1])) - float(np.float32(origin[1]))) * float(np.float32(cpm))
    if not (vx > -1.0 and vx < w and vy > -1.0 and vy < h):
        return None
    return int(vx), int(vy)


def descend_cells(field, tcell, allowed, mask, cell):
    """The cells of the path from `cell` (the start cell excluded) and the move into each."""
    h, w = field.shape
    out = []
    if cell is None:
        return out
    x, y = cell
    if not tcell[y, x] or field[y, x] == UNREACHED:
        return out
    while not mask[y, x]:
        best, bm = None, -1
        for m, (dx, dy) in enumerate(MOVES):
            if not allowed[m][y, x]:
                continue
            v = int(field[y + dy, x + dx])
            if v == UNREACHED:
                continue
            if best is None or v + STEP[m] < best:
                best, bm = v + STEP[m], m
        assert bm >= 0 and int(field[y + MOVES[bm][1], x + MOVES[bm][0]]) < int(field[y, x])
        x, y = x + MOVES[bm][0], y + MOVES[bm][1]
        out.append((x, y, bm))
    return out


POSE = np.dtype([("utime", "<i8"), ("x", "<f4"), ("y", "<f4"), ("theta", "<f4"), ("_pad", "<f4")])


def descend(field, l1, trav, pen, goals, reach, start, origin, mpc, cpm, _cache=None):
    """(poses as a POSE array, label, field(start)) for a start pose (utime, x, y, theta)."""
    if _cache is None:
        tcell, _ = cell_tables(l1, trav, pen)
        _cache = (tcell, allowed_moves(tcell), *goal_set(tcell, goals, reach))
    tcell, allowed, mask, label = _cache
    h, w = field.shape
    cell = pose_cell((start[1], start[2]), origin, cpm, w, h)
    cost = UNREACHED
    if cell is not None and tcell[cell[1], cell[0]]:
        cost = int(field[cell[1], cell[0]])
    steps = descend_cells(field, tcell, allowed, mask, cell)
    poses = np.zeros(1 + len(steps), POSE)
    poses[0] = (int(start[0]), np.float32(start[1]), np.float32(start[2]), np.float32(start[3]), 0)
    for k, (x, y, m) in enumerate(steps):
        px = np.float32(float(np.float32(origin[0])) + float(x) * float(np.float32(mpc)))
        py = np.float32(float(np.float32(origin[1])) + float(y) * float(np.float32(mpc)))
        poses[k + 1] = (int(start[0]), px, py, THETA[m], 0)
    end = (steps[-1][0], steps[-1][1]) if steps else cell
    lab = -1
    if end is not None and cost != UNREACHED and mask[end[1], end[0]]:
        lab = int(label[end[1], end[0]])
    return poses, lab, cost


def descend_cache(l1, trav, pen, goals, reach):
    """(traversable cells, allowed moves, goal mask, goal labels): what the descents of one field share."""
    tcell, _ = cell_tables(l1, trav, pen)
    return (tcell, allowed_moves(tcell), *goal_set(tcell, goals, reach))


def path_cost(cells_xy, allowed, pcell, mask):
    """The price of a chain of cells (start first) in this metric: steps plus the penalty of every cell outside the goal set; None
    if a step is not an allowed move (allowed = allowed_moves(tcell), pcell from cell_tables)."""
    total = 0
    for (x0, y0), (x1, y1) in zip(cells_xy[:-1], cells_xy[1:]):
        if (x1 - x0, y1 - y0) not in MOVES:
            return None
        m = MOVES.index((x1 - x0, y1 - y0))
        if not allowed[m][y0, x0]:
            return None
        total += STEP[m] + (0 if mask[y0, x0] else int(pcell[y0, x0]))
    return total
