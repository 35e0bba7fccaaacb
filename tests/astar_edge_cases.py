"""Inputs that take search_for_path to the edges no fixture map reaches, and a CPU model that says which edge each one reaches.

Worlds (plain numpy, no oracle, no GPU):
  corridor(H, kind, bx, bh, rows_total)   a 3400-cell-long walled corridor: along it fCost climbs to the fCost < INT16_MAX rule
                                          (astar.cpp:103,124), a tooth in it makes the open list drain to empty
  ring(W, H, t)                           an occupied block with a free band t cells wide along all four edges of the grid: every
                                          search runs on border cells and round corner cells

model() is the reference's search (astar.cpp:75-135) over an explicit array heap with libstdc++'s __adjust_heap / __push_heap index
operations (tests/tools/walk_ahead_model.py without its early-walk bookkeeping); besides pops and pushes it counts what a case
exists for: refused pushes, the extreme fCosts, the list's length, border and corner pops, and where a capacity would end it.

CASES is the list both test files run; reference(orc) runs the CPU oracle over it once per process."""
import hashlib
import json
import os
from collections import namedtuple

import numpy as np

import helpers

MPC = np.float32(0.05)
CORRIDOR_W = 3400
TWIN_ROWS = 160                                   # 3400 x 160 = 544 000 cells > 524 288: the forms that ask for cell lines two steps ahead
FLAT = (0.1, 0.1, 1.0)                            # maxDistanceWithCost == min: get_oCost is 0 everywhere, fCost is pure geometry
REF = (0.1, 1.0, 1.0)                             # the reference's own parameters for a 0.1 m robot (motion_planner.cpp:105-110)
MAX_POPS = 150_000                                # every case stays below this: a condition of the suite's run time


def corridor(H, kind=None, bx=0, bh=0, rows_total=None):
    cells = np.full((H, CORRIDOR_W), -80, np.int8)
    cells[0, :] = cells[H - 1, :] = 90
    cells[:, 0] = cells[:, CORRIDOR_W - 1] = 90
    mid = H // 2
    if kind == "centre":
        cells[mid - bh // 2:mid - bh // 2 + bh, bx] = 90
    elif kind == "wall":
        cells[1:1 + bh, bx] = 90
    else:
        assert kind is None
    if rows_total is not None:
        cells = np.concatenate([cells, np.full((rows_total - H, CORRIDOR_W), 90, np.int8)])
    return cells


def ring(W, H, t):
    cells = np.full((H, W), 90, np.int8)
    cells[:t, :] = cells[H - t:, :] = -80
    cells[:, :t] = cells[:, W - t:] = -80
    return cells


def centre(origin, c):
    """the pose coordinate at the centre of cell c"""
    return float(origin) + (c + 0.5) * 0.05


def cell_of(v, o, cpm=helpers.CPM_DEFAULT):
    """global_position_to_grid_cell on the pose's FLOAT coordinate (grid_utils.hpp:33-38): the cast truncates towards zero"""
    return int((float(np.float32(v)) - float(np.float32(o))) * float(np.float32(cpm)))


World = namedtuple("World", "key cells origin")
_worlds = {}


def world(key):
    """key: ("corridor", H, kind, bx, bh, rows_total) with origin (0, 0), or ("ring", W, H, t, ox, oy)"""
    if key not in _worlds:
        if key[0] == "corridor":
            _worlds[key] = World(key, corridor(*key[1:]), (np.float32(0.0), np.float32(0.0)))
        else:
            _worlds[key] = World(key, ring(*key[1:4]), (np.float32(key[4]), np.float32(key[5])))
    return _worlds[key]


# name; world key; start and goal (x, y) poses; (min, maxDistanceWithCost, exponent); (pops, pushes, poses) the oracle must give, or
# None where the row only has to equal the model / its twin / the JSON; want: the property the case exists for, as bounds on model()'s
# counts; twin_of: the plain corridor whose result this 160-row grid must equal
Case = namedtuple("Case", "name world start goal params expect want twin_of")


def _corridor_case(name, H, kind, bx, bh, D, expect, want, params=FLAT, rows_total=None, twin_of=None):
    mid = H // 2
    return Case(name, ("corridor", H, kind, bx, bh, rows_total), (centre(0, 5), centre(0, mid)), (centre(0, 5 + D), centre(0, mid)), params,
                expect, want, twin_of)


# (name, H, kind, bx, bh, D, (pops, pushes, poses), properties) -- the counts were confirmed by the CPU oracle and by model() independently
_CORRIDORS = [
    ("h9_d3275", 9, None, 0, 0, 3275, (3275, 9822, 3276), dict(found=True, refused=(1, 1), f_max=(32764, 32764))),
    ("h9_d3276", 9, None, 0, 0, 3276, (3276, 3275, 3277), dict(found=True, refused=(6551, 6551), longest=(1, 1), short_iterations=(3276, 3276))),
    ("h9_d3277", 9, None, 0, 0, 3277, (1, 0, 1), dict(found=False, refused=(4, 4), longest=(1, 1))),
    ("h15_centre_d3262", 15, "centre", 40, 3, 3262, (48695, 80279, 3269), dict(found=True, refused=(0, 0), longest=(33165, 33165))),
    ("h15_centre_d3270", 15, "centre", 40, 3, 3270, (41469, 54572, 3277), dict(found=True, refused=(20205, 20205), f_max=(32762, 32762),
                                                                               longest=(19740, 19740))),
    ("h15_wall8_d3270", 15, "wall", 40, 8, 3270, (26493, 33626, 3277), dict(found=True, refused=(13094, 13094), longest=(10691, 10691))),
    ("h15_wall10_bx40", 15, "wall", 40, 10, 3270, (792, 791, 1), dict(found=False, refused=(1, None), longest=(3, 255))),
    ("h15_wall10_bx1700", 15, "wall", 1700, 10, 3270, (36241, 36240, 1), dict(found=False, refused=(1, None), longest=(11293, 11293))),
    ("h15_wall10_bx3200", 15, "wall", 3200, 10, 3270, (68620, 68619, 1), dict(found=False, refused=(1, None), longest=(21116, 21116))),
]
# With maxDistanceWithCost 1.0 the obstacle cost is negative (-799 on the centre line of the H 9 corridor, -599 beside it) and the cut
# moves with it: along the centre line fCost = 10 D - 799, so D 3356 is the last goal that is reached (fCost 32761, the rows beside the
# line refused: ONE entry throughout, pops D, pushes D - 1) and D 3357 the first whose four first pushes are all refused.
_CORRIDORS_REF = [
    ("h9_ref_d3320", 9, None, 0, 0, 3320, (3320, 9958, 3321), dict(found=True, refused=(0, 0), f_max=(32615, 32615))),
    ("h9_ref_d3356", 9, None, 0, 0, 3356, (3356, 3355, 3357), dict(found=True, refused=(6711, 6711), f_max=(32761, 32761), longest=(1, 1))),
    ("h9_ref_d3357", 9, None, 0, 0, 3357, (1, 0, 1), dict(found=False, refused=(4, 4))),
]

CORRIDOR_CASES = [_corridor_case(*row) for row in _CORRIDORS] + [_corridor_case(*row, params=REF) for row in _CORRIDORS_REF]
TWIN_CASES = [_corridor_case(row[0] + "_160rows", *row[1:6], None, None, rows_total=TWIN_ROWS, twin_of=row[0]) for row in _CORRIDORS]

# ---- the reference's early exits (astar.cpp:40-62: 0 pops, 0 pushes, the 1-pose path), on the H 9 corridor
_S9 = (centre(0, 5), centre(0, 4))
_H9 = ("corridor", 9, None, 0, 0, None)
EARLY_EXIT_CASES = [
    Case("exit_start_is_goal", _H9, _S9, (centre(0, 5) + 0.01, centre(0, 4) - 0.01), FLAT, (0, 0, 1), None, None),
    Case("exit_goal_on_wall", _H9, _S9, (centre(0, 105), centre(0, 0)), FLAT, (0, 0, 1), None, None),
    Case("exit_goal_beside_grid_x", _H9, _S9, (-0.03, centre(0, 4)), FLAT, (0, 0, 1), None, None),       # truncation lands it in column 0: a wall cell
    Case("exit_goal_beside_grid_y", _H9, _S9, (centre(0, 105), -0.03), FLAT, (0, 0, 1), None, None),     # ... in row 0
    Case("exit_start_outside", _H9, (-20.0, centre(0, 4)), (centre(0, 105), centre(0, 4)), FLAT, (0, 0, 1), None, None),
]

# ---- border worlds
RING_SMALL = ("ring", 61, 37, 6, -3.0, -2.0)
RING_LARGE = ("ring", 1031, 521, 4, -3.0, -2.0)            # 537 151 cells > 524 288
RING_CHECKED = Case("ring61_corner_to_corner", RING_SMALL, (centre(-3.0, 60), centre(-2.0, 0)), (centre(-3.0, 0), centre(-2.0, 36)), FLAT,
                    (4876, 5496, 97), dict(found=True, border_pops=(260, 260)), None)
RING_JSON = os.path.join(helpers.GOLDEN, "astar_edge_cases.json")


def ring_cases():
    """the pairs of tests/golden/astar_edge_cases.json (tests/tools/make_astar_edge_cases.py)"""
    with open(RING_JSON) as f:
        rows = json.load(f)
    out = []
    for k, r in enumerate(rows):
        key = ("ring", *r["ring"], *r["origin"])
        out.append(Case("ring%dx%d_%02d" % (r["ring"][0], r["ring"][1], k), key, tuple(r["start"]), tuple(r["goal"]), FLAT,
                        (r["pops"], r["pushes"], r["poses"]), dict(found=True, border_pops=(1, None)), None))
    return out


def all_cases():
    return CORRIDOR_CASES + TWIN_CASES + EARLY_EXIT_CASES + [RING_CHECKED] + ring_cases()


# ---------------------------------------------------------------------------------------------------------------- the CPU model
def model(dist, origin, start, goal, params, cap=None, cpm=helpers.CPM_DEFAULT):
    """dist: the oracle's distance grid (H, W) float32.  Returns a dict: pops, pushes, found, poses, refused (pushes the f < 32767 rule
    turned away), f_max / f_min (of the entries pushed), longest (open list), short_iterations (entered with <= 1 entry), border_pops,
    corner_pops {(x, y): n}, last_move (dx, dy into the goal), and with cap=n capacity_at = (pops, pushes) at which a push first finds
    the list n entries long: the pop of that iteration counted, the refused push not (k_astar's C++ loop)."""
    mind, maxd, expo = params
    assert expo == 1.0
    H, W = dist.shape
    ex, ey = cell_of(goal[0], origin[0], cpm), cell_of(goal[1], origin[1], cpm)
    sx, sy = cell_of(start[0], origin[0], cpm), cell_of(start[1], origin[1], cpm)
    out = dict(pops=0, pushes=0, found=False, poses=1, refused=0, f_max=None, f_min=None, longest=0, short_iterations=0, border_pops=0,
               corner_pops={}, last_move=None, capacity_at=None)
    d64 = dist.astype(np.float64)
    valid_a = d64 > np.float64(mind) * 1.000001                                                   # isValid (astar.cpp:140-149)
    ocost_a = np.zeros((H, W), np.int64)
    band = (d64 > np.float64(mind)) & (d64 < np.float64(maxd))
    ocost_a[band] = (np.float64(maxd) - (dist[band] * np.float32(2000)).astype(np.float64)).astype(np.int64)   # the float product, then double; the cast truncates
    in_grid = lambda x, y: 0 <= x < W and 0 <= y < H
    if not (in_grid(ex, ey) and valid_a[ey, ex]) or not (in_grid(sx, sy) and valid_a[sy, sx]) or (sx, sy) == (ex, ey):
        return out
    valid = valid_a.ravel().tolist()
    ocost = ocost_a.ravel().tolist()
    closed_parent = {}                                    # cell -> parent cell of the FIRST closed entry (is_member / get_member)
    keys, ents = [0], [(sy * W + sx, 0, -1)]              # entry: (cell, gCost, parent cell)
    corners = {(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)}
    pops = pushes = refused = short = border = 0
    longest = 1
    f_max, f_min = None, None
    while keys:
        n = len(keys)
        short += n <= 1
        # ---- std::pop_heap + pop_back: the hole descends to a leaf, the former last entry climbs from there (stl_heap.h:214-262)
        (tcell, tg, tpar) = ents[0]
        vk, ve = keys.pop(), ents.pop()
        n -= 1
        if n > 0:
            hole, second = 0, 0
            while second < (n - 1) // 2:
                second = 2 * (second + 1)
                if keys[second] > keys[second - 1]:
                    second -= 1
                keys[hole], ents[hole] = keys[second], ents[second]
                hole = second
            if (n & 1) == 0 and second == (n - 2) // 2:
                second = 2 * (second + 1)
                keys[hole], ents[hole] = keys[second - 1], ents[second - 1]
                hole = second - 1
            while hole > 0 and keys[(hole - 1) // 2] > vk:
                par = (hole - 1) // 2
                keys[hole], ents[hole] = keys[par], ents[par]
                hole = par
            keys[hole], ents[hole] = vk, ve
        pops += 1
        cx, cy = tcell % W, tcell // W
        if tcell not in closed_parent:
            closed_parent[tcell] = tpar
        if cx == 0 or cy == 0 or cx == W - 1 or cy == H - 1:
            border += 1
            if (cx, cy) in corners:
                out["corner_pops"][(cx, cy)] = out["corner_pops"].get((cx, cy), 0) + 1
        # ---- expand_node (astar.cpp:213-233) in its order; a goal neighbour ends the search, the neighbours before it were pushed
        done = full = False
        for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1)):
            kx, ky = cx + dx, cy + dy
            if not in_grid(kx, ky):
                continue
            kcell = ky * W + kx
            if not valid[kcell]:
                continue
            if kx == ex and ky == ey:
                done = True
                out["last_move"] = (dx, dy)
                break
            if kcell in closed_parent:
                continue
            ax, ay = abs(ex - kx), abs(ey - ky)
            h = 14 * ay + 10 * (ax - ay) if ax >= ay else 14 * ax + 10 * (ay - ax)
            fn = tg + 10 + h + ocost[kcell]
            if not fn < 32767:                                                                     # astar.cpp:103,124
                refused += 1
                continue
            if cap is not None and len(keys) == cap:
                full = True
                break
            keys.append(fn); ents.append((kcell, tg + 10, tcell))                                 # push_back + std::push_heap
            hole = len(keys) - 1
            e = ents[hole]
            while hole > 0 and keys[(hole - 1) // 2] > fn:
                par = (hole - 1) // 2
                keys[hole], ents[hole] = keys[par], ents[par]
                hole = par
            keys[hole], ents[hole] = fn, e
            pushes += 1
            f_max = fn if f_max is None else max(f_max, fn)
            f_min = fn if f_min is None else min(f_min, fn)
        longest = max(longest, len(keys))
        if full:
            out["capacity_at"] = (pops, pushes)
            break
        if done:
            out["found"] = True
            steps, c, start_cell = 1, tcell, sy * W + sx                                          # makePath (astar.cpp:235-274)
            while c != start_cell:
                steps += 1
                c = closed_parent[c]
            out["poses"] = 1 + steps
            break
    out.update(pops=pops, pushes=pushes, refused=refused, f_max=f_max, f_min=f_min, longest=longest, short_iterations=short, border_pops=border)
    return out


def check_want(case, m):
    """the property the case exists for, on the model's counts"""
    for k, v in (case.want or {}).items():
        if k == "found":
            assert m["found"] is v, (case.name, k, m["found"])
        else:
            lo, hi = v
            assert m[k] is not None and m[k] >= lo and (hi is None or m[k] <= hi), (case.name, k, m[k], v)


# ---------------------------------------------------------------------------------------------------------------- the oracle, once
_reference = {}


def reference(orc, case):
    """What the CPU oracle says: dict(dist, path (structured array), stats (pops, pushes)).  Computed once per process and case; the
    distance grid once per world."""
    if case.name not in _reference:
        w = world(case.world)
        dkey = ("dist",) + w.key
        if dkey not in _reference:
            _reference[dkey] = orc.set_distances(w.cells, MPC, helpers.CPM_DEFAULT, w.origin)
        dist = _reference[dkey]
        path, stats = orc.search(orc.pose(*case.start, 0.3), orc.pose(*case.goal, 0.0), dist, MPC, helpers.CPM_DEFAULT, w.origin,
                                 case.params[0], case.params[1], exponent=case.params[2], cap=4096)
        _reference[case.name] = dict(dist=dist, path=path, stats=(int(stats[0]), int(stats[1])))
    return _reference[case.name]


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
