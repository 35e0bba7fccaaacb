"""Hand-built grids that take the navigation field (botlab_amd/csrc/bl_navfield.hip) down the paths no map reaches, one kernel path
at a time.  Plain numpy and the model (tests/nav_field_model.py): no oracle, no GPU.

Cells are FREE (-100) or SOURCE (+100).  With params() -- minDistanceToObstacle 0.05 -- exactly the source cells are not traversable
(f[1] = 0.1f > 0.05), so a single cell is an obstacle, and the penalty is non-zero up to L1 distance 4 (f[4] = 0.4f < 0.45).

Worlds, by name (world()):
  small_HxW            one source at (0, 0): grids of one tile and less, a side of 1, a second tile column one cell wide
  corner_S_CX_CY_D_P   S x S, the four cells round the tile corner (CX, CY): diagonal D (MOVES[4 + D]) through it, blocking pattern P
  big                  1024 rows x 1056 columns = 1056 tiles, 3 % single-cell sources: a goal in every tile, so round 1 lists more
                       tiles than a round has workgroups
  strip / strip_t      4192 x 32 (131 tiles in a column) and its transpose: the goal tile is 130 tile steps from the far one
  strip_short          the first 1056 rows of strip: small enough for nm.tile_fixed_point
  serpentine           64 x 64, a one-cell corridor that crosses the tile border in every second row
  open40               40 x 40, one source in the middle: the grid's border and cell (0, 0) are traversable

case(name) gives a Case: world, params, goals and the start poses its paths are taken from; solved(name) adds the model's field and
model_paths(name) the model's descents, each computed once per process."""
import functools
import os
import re
from collections import namedtuple

import numpy as np

import helpers
import nav_field_model as nm

CPM = helpers.CPM_DEFAULT
MPC = np.float32(0.05)
ORIGIN = (np.float32(-3.0), np.float32(-2.0))
ZERO = (np.float32(0.0), np.float32(0.0))
FREE, SOURCE = -100, 100
TILE = nm.TILE
HIP = os.path.join(os.path.dirname(helpers.HERE), "botlab_amd", "csrc", "bl_navfield.hip")

SMALL_SHAPES = [(1, 1), (1, 7), (9, 1), (31, 31), (32, 32), (33, 33), (31, 65), (65, 31)]     # (h, w), in the order they run on one handle
DIAGONALS = nm.MOVES[4:]                                                                    # (+x+y), (-x+y), (+x-y), (-x-y)
PATTERNS = ["open", "x_side", "y_side", "target"]
CORNERS = {64: [(32, 32)], 96: [(32, 32), (64, 32), (32, 64), (64, 64)]}
BIG_H, BIG_W = 1024, 1056
STRIP_ROWS, STRIP_SHORT_ROWS = 4192, 1056
GAIN_LAST_OK = 3957                                 # 1081344 * (14 + 3957) <= 4294967294 < 1081344 * (14 + 3958)

World = namedtuple("World", "cells origin")
Case = namedtuple("Case", "name world params goals starts")


def params(**kw):
    kw.setdefault("obstacle_gain", 50)
    return nm.Params(0.05, 0.45, 1.0, **kw)


def relax_grid_of_the_source():
    """NAV_RELAX_GRID as bl_navfield.hip defines it"""
    with open(HIP) as f:
        m = re.findall(r"^#define\s+NAV_RELAX_GRID\s+(\d+)", f.read(), re.M)
    assert len(m) == 1, m
    return int(m[0])


# ---------------------------------------------------------------------------------------------------------------- worlds
def _small(h, w):
    c = np.full((h, w), FREE, np.int8)
    c[0, 0] = SOURCE
    return c


def corner_cells(cx, cy, d):
    """The four cells round the tile corner (cx, cy) as diagonal d sees them: A the cell the move leaves, B the diagonal target,
    X and Y the side cells in the move's x and y direction."""
    sx, sy = DIAGONALS[d]
    a = (cx - 1 if sx > 0 else cx, cy - 1 if sy > 0 else cy)
    return dict(A=a, B=(a[0] + sx, a[1] + sy), X=(a[0] + sx, a[1]), Y=(a[0], a[1] + sy), d=(sx, sy))


def _corner(size, cx, cy, d, pattern):
    c = np.full((size, size), FREE, np.int8)
    c[size - 1, 0] = SOURCE                         # a grid without a source has no traversable cell; this one is far from every pattern
    k = corner_cells(cx, cy, d)
    hit = dict(open=None, x_side="X", y_side="Y", target="B")[pattern]
    if hit:
        c[k[hit][1], k[hit][0]] = SOURCE
    return c


def _random_sources(h, w, share, seed):
    c = np.full((h, w), FREE, np.int8)
    c[np.random.default_rng(seed).random((h, w)) < share] = SOURCE
    return c


def _strip(keep_row):
    c = _random_sources(STRIP_ROWS, TILE, 0.02, 4192)
    c[:, 0] = c[:, TILE - 1] = SOURCE
    c[keep_row, 10:20] = FREE
    return c


def _serpentine():
    c = np.full((64, 64), FREE, np.int8)
    c[:, 0] = c[:, 63] = SOURCE
    for y in range(1, 64, 2):
        c[y, :] = SOURCE
        c[y, 62 if (y // 2) % 2 == 0 else 1] = FREE
    return c


def _open40():
    c = np.full((40, 40), FREE, np.int8)
    c[20, 20] = SOURCE
    return c


@functools.lru_cache(maxsize=None)
def world(name):
    k = name.split("_")
    if k[0] == "small":
        h, w = (int(v) for v in k[1].split("x"))
        return World(_small(h, w), ORIGIN)
    if k[0] == "corner":
        return World(_corner(int(k[1]), int(k[2]), int(k[3]), int(k[4]), "_".join(k[5:])), ORIGIN)
    if name == "big":
        return World(_random_sources(BIG_H, BIG_W, 0.03, 1056), ORIGIN)
    if name == "strip":
        return World(_strip(5), ORIGIN)
    if name == "strip_short":
        return World(_strip(5)[:STRIP_SHORT_ROWS].copy(), ORIGIN)
    if name == "strip_t":
        return World(np.ascontiguousarray(_strip(STRIP_ROWS - 6).T), ORIGIN)
    if name == "serpentine":
        return World(_serpentine(), ORIGIN)
    if name == "open40":
        return World(_open40(), ZERO)               # origin 0: the float32 pose of cell coordinate -1.0 is exactly -1 cell
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def l1(world_name):
    return nm.l1_distances(world(world_name).cells)


def tables(world_name, p):
    h, w = world(world_name).cells.shape
    return nm.tables(nm.dist_table(w, h), p)


def traversable(world_name, p):
    trav, pen = tables(world_name, p)
    return nm.cell_tables(l1(world_name), trav, pen)[0]


def expected_floats(world_name):
    """What the distance grid of this world must show: the model's f[n(c)]"""
    n = l1(world_name)
    f = nm.dist_table(n.shape[1], n.shape[0])
    return np.where(n == nm.NONE16, np.float32(-1.0), f[np.minimum(n, len(f) - 1)])


# ---------------------------------------------------------------------------------------------------------------- poses
def pose_at(origin, cx, cy, theta=0.0, utime=0):
    """(utime, x, y, theta): the float32 pose at the cell coordinates (cx, cy), formed as tests/test_gpu_nav_field.py forms it"""
    return (int(utime), np.float32(float(origin[0]) + cx * float(MPC)), np.float32(float(origin[1]) + cy * float(MPC)), np.float32(theta))


def cell_coordinate(origin, v, axis):
    """The double the library truncates to a cell: (pose - origin) * cellsPerMeter on the pose's float32"""
    return (float(np.float32(v)) - float(np.float32(origin[axis]))) * float(np.float32(CPM))


def _centres(origin, cells_xy):
    return [pose_at(origin, x + 0.5, y + 0.5, theta=0.01 * (i % 300) - 1.5, utime=500 + i) for i, (x, y) in enumerate(cells_xy)]


def _first_traversable(tcell, y, x_from):
    xs = np.flatnonzero(tcell[y, x_from:])
    return (x_from + int(xs[0]), y)


# the starts at the low edge of open40: (cell coordinates, the cell they must resolve to or None for "off the grid")
EDGE_STARTS = [
    ((-0.5, 3.5), (0, 3)), ((3.5, -0.5), (3, 0)), ((-0.999, -0.999), (0, 0)), ((39.5, 39.5), (39, 39)), ((7.25, 12.75), (7, 12)),
    ((-1.0, 3.5), None), ((3.5, -1.0), None), ((40.0, 3.5), None), ((3.5, 40.0), None),
    ((float("nan"), 3.5), None), ((3.5, float("nan")), None), ((float("inf"), 3.5), None), ((3.5, float("inf")), None),
    ((float("-inf"), 3.5), None), ((3.5, float("-inf")), None),
    ((20.5, 20.5), (20, 20)),                       # on the grid, on the source cell: not traversable
]


# ---------------------------------------------------------------------------------------------------------------- cases
def small_name(h, w):
    return "small_%dx%d" % (h, w)


def corner_name(size, cx, cy, d, pattern):
    return "corner_%d_%d_%d_%d_%s" % (size, cx, cy, d, pattern)


def corner_names():
    return [corner_name(size, cx, cy, d, p) for size in sorted(CORNERS) for cx, cy in CORNERS[size] for d in range(4) for p in PATTERNS]


def big_goals():
    """The first traversable cell of every tile in row-major order, tiles in row-major order"""
    tcell = traversable("big", params())
    out = []
    for ty in range(BIG_H // TILE):
        for tx in range(BIG_W // TILE):
            i = int(np.flatnonzero(tcell[ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE].ravel())[0])
            out.append((tx * TILE + i % TILE, ty * TILE + i // TILE))
    return out


def _batch_of_70(world_name, far, near):
    """One long descent (from `far`) among 69 short ones: more than one 64-thread workgroup of k_nav_paths"""
    cells = near[:40] + [far] + near[40:69]
    assert len(cells) == 70
    return _centres(world(world_name).origin, cells)


@functools.lru_cache(maxsize=None)
def case(name):
    k = name.split("_")
    if k[0] == "small":
        h, w = world(name).cells.shape
        tcell = traversable(name, params())
        ys, xs = np.nonzero(tcell)
        return Case(name, name, params(), [(w - 1, h - 1), (w + 3, -2)], _centres(ORIGIN, list(zip(xs.tolist(), ys.tolist()))))
    if k[0] == "corner":
        c = corner_cells(int(k[2]), int(k[3]), int(k[4]))
        goal = (c["B"][0] + 6 * c["d"][0], c["B"][1] + 6 * c["d"][1])
        return Case(name, name, params(), [goal], _centres(ORIGIN, [c["A"]]))
    if name == "big":
        return Case(name, "big", params(), big_goals(), [])
    if name == "big_gain_edge":                     # exponent 0: every cell within maxDistanceWithCost pays the whole gain
        return Case(name, "big", nm.Params(0.05, 0.45, 0.0, obstacle_gain=GAIN_LAST_OK), big_goals(), [])
    if name == "strip":
        tcell = traversable("strip", params())
        near = [_first_traversable(tcell, 5 + 4 * i, 1 + (7 * i) % 25) for i in range(69)]
        near[0] = (15, 5)                           # the goal cell itself: one pose
        return Case(name, "strip", params(), [(15, 5)], _batch_of_70("strip", _first_traversable(tcell, STRIP_ROWS - 2, 12), near))
    if name == "strip_short":
        return Case(name, "strip_short", params(), [(15, 5)], [])
    if name == "strip_t":
        return Case(name, "strip_t", params(), [(STRIP_ROWS - 6, 15)], [])
    if name == "serpentine":
        near = [(1 + (5 * i) % 62, 2 * (i % 6)) for i in range(69)]         # near[0] is the goal cell
        return Case(name, "serpentine", params(), [(1, 0)], _batch_of_70("serpentine", (1, 62), near))
    if name == "edge_starts":
        return Case(name, "open40", params(), [(30, 30)], [pose_at(ZERO, cx, cy, theta=0.25, utime=900 + i) for i, ((cx, cy), _) in enumerate(EDGE_STARTS)])
    every = _centres(ZERO, [(x, y) for y in range(40) for x in range(40)])
    if name == "reach_all":                         # every window covers the grid; the off-grid cell is skipped: label 1
        return Case(name, "open40", params(reach_cells=1024), [(100, 100), (5, 5), (6, 6)], every)
    if name == "reach_clipped":
        return Case(name, "open40", params(reach_cells=3), [(0, 0), (39, 39)], every[::7])
    raise KeyError(name)


FAR_START = 40                                      # the index of the long descent in a batch of 70


@functools.lru_cache(maxsize=None)
def solved(name):
    """(l1, trav, pen, goals, params, the model's field)"""
    c = case(name)
    trav, pen = tables(c.world, c.params)
    return l1(c.world), trav, pen, c.goals, c.params, nm.dijkstra(l1(c.world), trav, pen, c.goals, c.params.reach_cells)


@functools.lru_cache(maxsize=None)
def model_paths(name):
    """[(poses, label, cost)] of nm.descend from every start of the case"""
    c = case(name)
    n, trav, pen, goals, p, field = solved(name)
    cache = nm.descend_cache(n, trav, pen, goals, p.reach_cells)
    w = world(c.world)
    return [nm.descend(field, n, trav, pen, goals, p.reach_cells, s, w.origin, MPC, CPM, _cache=cache) for s in c.starts]


def tile_steps(goal, cell):
    """Chebyshev distance, in tiles, between the tiles of two cells: no round before this one can list the tile of `cell`"""
    return max(abs(goal[0] // TILE - cell[0] // TILE), abs(goal[1] // TILE - cell[1] // TILE))


def path_moves(poses):
    """The (dx, dy) of every step of a model path, read back from the thetas"""
    thetas = [t.tobytes() for t in nm.THETA]
    return [nm.MOVES[thetas.index(p["theta"].tobytes())] for p in poses[1:]]
