"""The view-gain model (tests/view_gain_model.py) against an independent plain-loop implementation of the definition
(include/botlab_hip.h, "view gain") -- seen sets and counts -- on partially explored versions of the golden maps, the properties
the definition implies, and the planner's choice on a constructed map.  No GPU: this is what the kernel is compared with."""
import math

import numpy as np
import pytest

import nav_field_model as nm
import view_gain_model as vm

MAPS = ["obstacle_slam_10mx10m_5cm", "convex_10mx10m_5cm", "drive_square_10mx10m_5cm", "astar_maze"]
P = vm.Params(60, 360)


# ---- the independent implementation: one cell at a time, a Python set
def _loop_ends(r, k_rays):
    out = []
    for k in range(k_rays):
        t = 2.0 * math.pi * k / k_rays
        vx, vy = r * math.cos(t), r * math.sin(t)
        out.append((int(math.copysign(math.floor(abs(vx) + 0.5), vx)), int(math.copysign(math.floor(abs(vy) + 0.5), vy))))
    return out


def _loop_seen(cells, p, ends, cx, cy):
    h, w = cells.shape
    seen = set()
    if not (0 <= cx < w and 0 <= cy < h):
        return seen
    for ex, ey in ends:
        ex, ey = int(ex), int(ey)
        dx, dy = abs(ex), abs(ey)
        sx = 1 if ex > 0 else (-1 if ex < 0 else 0)
        sy = 1 if ey > 0 else (-1 if ey < 0 else 0)
        err, x, y = dx - dy, 0, 0
        while not (x == ex and y == ey):
            e2 = 2 * err
            if e2 >= -dy:
                err -= dy
                x += sx
            if e2 <= dx:
                err += dx
                y += sy
            gx, gy = cx + x, cy + y
            if gx < 0 or gy < 0 or gx >= w or gy >= h:
                break
            v = int(cells[gy, gx])
            if v > p.occupied_above:
                break
            if p.unknown_lo <= v <= p.unknown_hi:
                seen.add((gx, gy))
    return seen


def _mask_as_set(mask, r, cx, cy):
    ys, xs = np.nonzero(mask)
    return set((int(x) - r + cx, int(y) - r + cy) for x, y in zip(xs, ys))


def test_ray_table_equals_the_plain_loop():
    for r, k in [(60, 360), (1, 8), (255, 4096), (100, 360), (7, 1), (33, 77)]:
        assert [tuple(e) for e in vm.ray_ends(r, k).tolist()] == _loop_ends(r, k), (r, k)
    e = vm.ray_ends(60, 360)
    assert tuple(e[0]) == (60, 0) and tuple(e[90]) == (0, 60) and np.abs(e).max() == 60


def test_walk_is_the_definition():
    assert vm.walk(0, 0) == []
    assert vm.walk(3, 0) == [(1, 0), (2, 0), (3, 0)]
    assert vm.walk(-2, -2) == [(-1, -1), (-2, -2)]
    for ex, ey in [(5, 2), (-7, 3), (1, -9), (255, 254), (-60, 0), (0, 13)]:
        l = vm.walk(ex, ey)
        assert l[-1] == (ex, ey) and len(l) == max(abs(ex), abs(ey)) and len(set(l)) == len(l)
        assert all(max(abs(x1 - x0), abs(y1 - y0)) == 1 for (x0, y0), (x1, y1) in zip([(0, 0)] + l[:-1], l))


@pytest.mark.parametrize("name", MAPS)
def test_model_equals_the_plain_loop_on_partially_explored_maps(maps, name):
    cells, _ = vm.partially_explored(maps[name]["cells"])
    cands = vm.near_frontier_candidates(cells, 3)
    assert len(cands) >= 50, (name, len(cands))
    ends = vm.ray_ends(P.radius_cells, P.n_rays)
    wt = vm.walks(ends)
    got = vm.gains(cells, P, cands)
    sample = cands[::4]
    lo, hi = 1 << 30, 0
    for (x, y), g in zip(sample, got[::4]):
        want = _loop_seen(cells, P, ends, int(x), int(y))
        mask = vm.seen_mask(cells, P, wt, int(x), int(y))
        assert _mask_as_set(mask, P.radius_cells, int(x), int(y)) == want, (name, x, y)
        assert int(g) == len(want) == int(mask.sum())
        lo, hi = min(lo, len(want)), max(hi, len(want))
    for (x, y), g in zip(cands, got):
        assert int(g) <= vm.window_bound(cells, P, int(x), int(y))
    print(name, "candidates", len(cands), "gain", lo, "..", hi)
    assert hi > 0


@pytest.mark.parametrize("name", ["empty", "narrow"])
def test_no_unknown_cells_no_gain(maps, name):
    cells = maps[name]["cells"]
    if (cells == 0).any():                              # the property is about maps without unknown cells
        cells = np.where(cells == 0, -1, cells).astype(np.int8)
    h, w = cells.shape
    cands = [(x, y) for y in range(0, h, 17) for x in range(0, w, 17)]
    assert not vm.gains(cells, P, cands).any()


def test_blocking_ring_gives_zero():
    cells = np.zeros((61, 61), np.int8)
    cells[29:32, 29:32] = 100
    cells[30, 30] = 0
    assert vm.gains(cells, vm.Params(20, 64), [(30, 30)])[0] == 0
    cells[29, 29] = 0                                   # a gap in the ring, on a diagonal ray
    assert vm.gains(cells, vm.Params(20, 64), [(30, 30)])[0] > 0


def _symmetries():
    return [("identity", lambda a: a, lambda x, y, w, h: (x, y), lambda ex, ey: (ex, ey)),
            ("flip x", lambda a: a[:, ::-1], lambda x, y, w, h: (w - 1 - x, y), lambda ex, ey: (-ex, ey)),
            ("flip y", lambda a: a[::-1, :], lambda x, y, w, h: (x, h - 1 - y), lambda ex, ey: (ex, -ey)),
            ("rotate 180", lambda a: a[::-1, ::-1], lambda x, y, w, h: (w - 1 - x, h - 1 - y), lambda ex, ey: (-ex, -ey)),
            ("transpose", lambda a: a.T, lambda x, y, w, h: (y, x), lambda ex, ey: (ey, ex)),
            ("transpose, flip x", lambda a: a.T[:, ::-1], lambda x, y, w, h: (h - 1 - y, x), lambda ex, ey: (-ey, ex)),
            ("transpose, flip y", lambda a: a.T[::-1, :], lambda x, y, w, h: (y, w - 1 - x), lambda ex, ey: (ey, -ex)),
            ("anti-transpose", lambda a: a.T[::-1, ::-1], lambda x, y, w, h: (h - 1 - y, w - 1 - x), lambda ex, ey: (-ey, -ex))]


def test_gain_is_invariant_under_the_symmetries_the_ray_table_has(maps):
    """K a multiple of 8.  cos and sin are rounded separately, so the table need not be closed under every symmetry of the square
    (R cos 60 deg = 30.000000000000004 but R sin 30 deg = 29.999999999999996 at R = 60 -- both round to 30 there, but nothing
    promises that at every R): each symmetry is first verified on the table and only then on the gains.  The walk itself is
    symmetric: it is built from |ex|, |ey| and the signs, and swapping the axes swaps its two conditions."""
    p = vm.Params(40, 360)
    ends = set(map(tuple, vm.ray_ends(p.radius_cells, p.n_rays).tolist()))
    cells, _ = vm.partially_explored(maps["obstacle_slam_10mx10m_5cm"]["cells"])
    h, w = cells.shape
    cands = vm.near_frontier_candidates(cells, 3)[::9]
    base = vm.gains(cells, p, cands)
    assert base.any()
    held = []
    for name, tmap, tcell, tend in _symmetries():
        if set(tend(ex, ey) for ex, ey in ends) != ends:
            continue
        held.append(name)
        tc = np.ascontiguousarray(tmap(cells))
        tq = [tcell(int(x), int(y), w, h) for x, y in cands]
        assert np.array_equal(vm.gains(tc, p, tq), base), name
    print("symmetries of the table:", held)
    assert "identity" in held and len(held) >= 2             # something beside the identity was put to the test


def test_edges_and_off_grid_candidates():
    cells = np.zeros((20, 30), np.int8)
    p = vm.Params(5, 64)
    off = [(-1, 0), (0, -1), (30, 5), (5, 20), (-100, -100)]
    assert not vm.gains(cells, p, off).any()
    ends = vm.ray_ends(5, 64)
    for c in [(0, 0), (29, 19), (0, 19), (29, 0), (15, 0), (0, 10)]:
        want = _loop_seen(cells, p, ends, *c)
        assert vm.gains(cells, p, [c])[0] == len(want) > 0
        assert all(0 <= x < 30 and 0 <= y < 20 for x, y in want) and c not in want
    # the candidate's own cell is never examined: a candidate on a blocking cell sees what a free one would
    cells2 = cells.copy()
    cells2[10, 15] = 100
    assert vm.gains(cells2, p, [(15, 10)])[0] == vm.gains(cells, p, [(15, 10)])[0]
    # class thresholds
    cells3 = np.full((20, 30), -3, np.int8)
    cells3[:, 20:] = 5
    assert vm.gains(cells3, p, [(15, 10)])[0] == 0
    q = vm.Params(5, 64, occupied_above=5, unknown_lo=-3, unknown_hi=-3)
    assert vm.gains(cells3, q, [(15, 10)])[0] == len(_loop_seen(cells3, q, ends, 15, 10)) > 0


def _constructed():
    cells, origin, mpc, robot = vm.two_frontier_map()
    h, w = cells.shape
    l1 = nm.l1_distances(cells)
    trav, pen = nm.tables(nm.dist_table(w, h), nm.Params(0.1, 1.0, 1.0))
    reach = next(n for n in range(w + h + 1) if trav[n])
    fr = vm.frontier_cells(cells)
    owner = [0 if x < 100 else 1 for x, y in fr]             # the niche, the hall
    return cells, l1, trav, pen, robot, fr, owner, reach


def test_zero_weight_picks_the_cheapest_candidate():
    cells, l1, trav, pen, robot, fr, owner, reach = _constructed()
    p = vm.Params(30, 120)
    c = vm.choose(cells, l1, trav, pen, robot, fr, owner, reach, p, gain_weight=0)
    tcell, _ = nm.cell_tables(l1, trav, pen)
    mask, _ = nm.goal_set(tcell, fr, reach)
    ok = mask & (c["field"] != nm.UNREACHED)
    ys, xs = np.nonzero(ok)
    g = vm.gains(cells, p, np.stack([xs, ys], axis=1))
    assert c["cost"] == int(c["field"][ys[g >= 1], xs[g >= 1]].min())
    assert c["gain"] >= 1


def test_gain_choice_differs_from_cost_choice_on_the_constructed_map():
    cells, l1, trav, pen, robot, fr, owner, reach = _constructed()
    assert set(owner) == {0, 1}
    # the cost rule: one field over every frontier cell, the descent from the robot ends on the nearest goal
    field = nm.dijkstra(l1, trav, pen, fr, reach)
    cache = nm.descend_cache(l1, trav, pen, fr, reach)
    steps = nm.descend_cells(field, cache[0], cache[1], cache[2], robot)
    end = (steps[-1][0], steps[-1][1]) if steps else robot
    by_cost = owner[int(cache[3][end[1], end[0]])]
    c = vm.choose(cells, l1, trav, pen, robot, fr, owner, reach, vm.Params(60, 360))
    print("cost rule -> frontier", by_cost, "; gain rule ->", {k: v for k, v in c.items() if k != "field"})
    assert by_cost == 0 and c["frontier"] == 1
    assert c["gain"] > 120                                   # more than the whole niche holds
    # thinning, a floor on the gain and no robot cell
    c4 = vm.choose(cells, l1, trav, pen, robot, fr, owner, reach, vm.Params(60, 360), stride=2)
    assert c4 is not None and c4["cell"][0] % 2 == 0 and c4["cell"][1] % 2 == 0 and c4["candidates"] < c["candidates"]
    assert vm.choose(cells, l1, trav, pen, robot, fr, owner, reach, vm.Params(60, 360), min_gain=10 ** 6) is None
    assert vm.choose(cells, l1, trav, pen, None, fr, owner, reach, vm.Params(60, 360)) is None
