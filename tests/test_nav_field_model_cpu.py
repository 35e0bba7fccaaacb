"""The navigation field's model (tests/nav_field_model.py) checked against itself on the CPU: the heap Dijkstra against an
independent tile-sweep implementation in several tile orders, a Bellman certificate checker that accepts the model and rejects
corrupted fields, the properties of the descent, and the reference search's own paths priced in this metric."""
import functools

import numpy as np
import pytest

import helpers
import nav_field_model as nm

ASTAR = ["empty", "filled", "narrow", "wide", "convex", "maze"]
SLAM = helpers.SLAM_MAPS
CPM = helpers.CPM_DEFAULT


def _astar_params(**kw):
    return nm.Params(0.1, 1.0, 1.0, **kw)               # MotionPlannerParams(0.1): astar_test.cpp:227-228


def _slam_params(**kw):
    return nm.Params(0.2, 2.0, 1.0, **kw)


@functools.lru_cache(maxsize=None)
def _maps():
    return helpers.load_reference_maps()


@functools.lru_cache(maxsize=None)
def _l1(name):
    if name == "ragged":
        return nm.l1_distances(ragged_cells())
    return nm.l1_distances(_maps()[name]["cells"])


def ragged_cells(w=173, h=211, seed=5):
    """A 173 x 211 world: walls with gaps and scattered blocks, free elsewhere; neither side a multiple of the tile."""
    rng = np.random.default_rng(seed)
    c = np.full((h, w), -100, np.int8)
    c[0, :] = c[-1, :] = 100
    c[:, 0] = c[:, -1] = 100
    for x in range(30, w - 20, 35):
        c[:, x] = 100
        for g in rng.integers(10, h - 25, 2):
            c[g:g + 14, x] = -100
    for _ in range(25):
        x, y = int(rng.integers(5, w - 8)), int(rng.integers(5, h - 8))
        c[y:y + 3, x:x + 3] = 100
    return c


def _far_cell(l1, trav):
    """A deterministic traversable cell: the first one with the largest finite L1 distance."""
    t, _ = nm.cell_tables(l1, trav, np.zeros(len(trav), np.int32))
    v = np.where(t, l1.astype(np.int64), -1)
    y, x = np.unravel_index(int(np.argmax(v)), v.shape)
    return (int(x), int(y)) if v[y, x] >= 0 else (0, 0)


def _spread_cells(l1, trav, n, seed):
    t, _ = nm.cell_tables(l1, trav, np.zeros(len(trav), np.int32))
    ys, xs = np.nonzero(t)
    if len(xs) == 0:
        return [(1, 1)] * n
    idx = np.random.default_rng(seed).choice(len(xs), size=n, replace=len(xs) < n)
    return [(int(xs[i]), int(ys[i])) for i in idx]


def cases():
    """name -> (map name, params, goals).  The six A* maps with the goals of their golden cases, the SLAM maps with the smoke goal and
    the deepest free cell, a ragged grid, multi-goal and reach > 0 cases."""
    out = {}
    rows = helpers.load_astar_cases()
    for name in ASTAR:
        m = _maps()["astar_" + name]
        h, w = m["cells"].shape
        goals = []
        for r in rows[name]:
            c = nm.pose_cell(r["goal"], m["origin"], CPM, w, h)
            goals.append(c if c is not None else (-1, -1))
        out["astar_" + name] = ("astar_" + name, _astar_params(), goals[:1])
        out["astar_" + name + "_all_goals"] = ("astar_" + name, _astar_params(), goals)
    for name in SLAM:
        m = _maps()[name]
        h, w = m["cells"].shape
        p = _slam_params()
        trav, _ = nm.tables(nm.dist_table(w, h), p)
        out[name] = (name, p, [nm.pose_cell((-0.35, 0.2), m["origin"], CPM, w, h)])
        out[name + "_far"] = (name, p, [_far_cell(_l1(name), trav)])
    p = _astar_params()
    trav, _ = nm.tables(nm.dist_table(173, 211), p)
    out["ragged"] = ("ragged", p, [_far_cell(_l1("ragged"), trav)])
    out["ragged_multi"] = ("ragged", p, _spread_cells(_l1("ragged"), trav, 7, 1) + [(-3, 5), (500, 2)])
    out["ragged_reach"] = ("ragged", _astar_params(reach_cells=4), _spread_cells(_l1("ragged"), trav, 3, 2) + [(15, 0), (172, 210)])
    m = "obstacle_slam_10mx10m_5cm"
    ps = _slam_params(reach_cells=3)
    trav, _ = nm.tables(nm.dist_table(200, 200), ps)
    out["slam_reach_multi"] = (m, ps, _spread_cells(_l1(m), trav, 5, 3) + [(0, 0)])
    out["maze_steep"] = ("astar_maze", nm.Params(0.1, 1.0, 2.5, obstacle_gain=4095), [out["astar_maze"][2][0]])
    out["convex_flat"] = ("astar_convex", nm.Params(0.1, 0.05, 1.0, obstacle_gain=50), [out["astar_convex"][2][0]])     # maxD <= minD: no penalty
    return out


@functools.lru_cache(maxsize=None)
def solved(case):
    name, p, goals = cases()[case]
    l1 = _l1(name)
    h, w = l1.shape
    trav, pen = nm.tables(nm.dist_table(w, h), p)
    return l1, trav, pen, goals, p, nm.dijkstra(l1, trav, pen, goals, p.reach_cells)


CASES = sorted(cases())


def test_l1_and_table_are_the_distance_grid(oracle):
    for name in ("obstacle_slam_10mx10m_5cm", "astar_maze", "astar_empty"):
        m = _maps()[name]
        l1 = _l1(name)
        h, w = l1.shape
        f = nm.dist_table(w, h)
        mine = np.where(l1 == nm.NONE16, np.float32(-1.0), f[np.minimum(l1, len(f) - 1)])
        ref = oracle.set_distances(m["cells"], m["mpc"], CPM, m["origin"])
        assert np.array_equal(mine.view(np.uint32), ref.view(np.uint32)), name


@pytest.mark.parametrize("case", CASES)
def test_tile_sweeps_equal_dijkstra_in_every_order(case):
    l1, trav, pen, goals, p, field = solved(case)
    rounds = []
    for order, seed in (("forward", 0), ("reverse", 0), ("random", 11)):
        got, r = nm.tile_fixed_point(l1, trav, pen, goals, p.reach_cells, order=order, seed=seed)
        assert np.array_equal(got, field), (case, order)
        rounds.append(r)
    tcell, _ = nm.cell_tables(l1, trav, pen)
    assert max(rounds) <= int(tcell.sum()) + 1                 # the bound the library caps its rounds at


@pytest.mark.parametrize("case", CASES)
def test_certificate_accepts_the_model(case):
    l1, trav, pen, goals, p, field = solved(case)
    assert nm.certificate(field, l1, trav, pen, goals, p.reach_cells) is None


@pytest.mark.parametrize("case", ["astar_maze", "obstacle_slam_10mx10m_5cm", "ragged_reach"])
def test_certificate_rejects_corruptions(case):
    l1, trav, pen, goals, p, field = solved(case)
    tcell, _ = nm.cell_tables(l1, trav, pen)
    mask, _ = nm.goal_set(tcell, goals, p.reach_cells)
    reached = np.argwhere((field != nm.UNREACHED) & ~mask)
    assert len(reached) > 100
    y, x = reached[len(reached) // 2]
    for delta in (1, -1):
        bad = field.copy()
        bad[y, x] = int(bad[y, x]) + delta
        assert nm.certificate(bad, l1, trav, pen, goals, p.reach_cells) is not None, delta
    # a reachable pocket set to UNREACHED: the 5 x 5 block around the cell (its non-traversable cells already are)
    bad = field.copy()
    bad[max(y - 2, 0):y + 3, max(x - 2, 0):x + 3] = nm.UNREACHED
    bad[mask] = 0
    assert not np.array_equal(bad, field)
    assert nm.certificate(bad, l1, trav, pen, goals, p.reach_cells) is not None
    # and a goal cell that is not 0, a wall cell that is reached
    gy, gx = np.argwhere(mask)[0]
    bad = field.copy()
    bad[gy, gx] = 10
    assert nm.certificate(bad, l1, trav, pen, goals, p.reach_cells) is not None
    wy, wx = np.argwhere(~tcell)[0]
    bad = field.copy()
    bad[wy, wx] = 0
    assert nm.certificate(bad, l1, trav, pen, goals, p.reach_cells) is not None


def check_path_properties(poses, label, cost, field, l1, trav, pen, goals, reach, origin, mpc, cache=None, pcell=None):
    """The properties every path must have; poses is a nm.POSE array (also used by the GPU tests on large maps)."""
    tcell, allowed, mask, lab = cache or nm.descend_cache(l1, trav, pen, goals, reach)
    if pcell is None:
        pcell = nm.cell_tables(l1, trav, pen)[1]
    h, w = field.shape
    start = nm.pose_cell((poses[0]["x"], poses[0]["y"]), origin, CPM, w, h)
    if len(poses) == 1:
        assert start is None or not tcell[start[1], start[0]] or field[start[1], start[0]] == nm.UNREACHED or mask[start[1], start[0]]
        return
    cells = [start]
    for p in poses[1:]:
        cells.append((int(round((float(p["x"]) - float(origin[0])) / float(mpc))), int(round((float(p["y"]) - float(origin[1])) / float(mpc)))))
        assert p["utime"] == poses[0]["utime"]
    vals = [int(field[y, x]) for x, y in cells]
    assert all(tcell[y, x] for x, y in cells)                                  # every cell traversable
    assert all(b < a for a, b in zip(vals[:-1], vals[1:]))                     # strictly decreasing field
    assert mask[cells[-1][1], cells[-1][0]] and not any(mask[y, x] for x, y in cells[:-1])   # ends on the goal set, at its first cell
    total = nm.path_cost(cells, allowed, pcell, mask)                          # None: a move that is not allowed (a cut corner)
    assert total is not None and total == vals[0] == cost                      # the summed cost is field(start)
    assert label == lab[cells[-1][1], cells[-1][0]]
    for k in range(1, len(cells)):
        m = nm.MOVES.index((cells[k][0] - cells[k - 1][0], cells[k][1] - cells[k - 1][1]))
        assert poses[k]["theta"].tobytes() == nm.THETA[m].tobytes()


@pytest.mark.parametrize("case", CASES)
def test_paths_descend_to_the_goal_set(case):
    l1, trav, pen, goals, p, field = solved(case)
    name = cases()[case][0]
    origin, mpc = ((-4.0, -5.0), np.float32(0.05)) if name == "ragged" else (_maps()[name]["origin"], _maps()[name]["mpc"])
    h, w = l1.shape
    cache = nm.descend_cache(l1, trav, pen, goals, p.reach_cells)
    rng = np.random.default_rng(17)
    found = 0
    for i in range(60):
        x, y = rng.uniform(-0.5, w + 0.5), rng.uniform(-0.5, h + 0.5)
        start = (1000 + i, np.float32(float(origin[0]) + x * float(mpc)), np.float32(float(origin[1]) + y * float(mpc)), np.float32(rng.uniform(-3, 3)))
        poses, label, cost = nm.descend(field, l1, trav, pen, goals, p.reach_cells, start, origin, mpc, CPM, _cache=cache)
        assert poses[0]["x"] == start[1] and poses[0]["theta"] == start[3] and poses[0]["utime"] == start[0]
        check_path_properties(poses, label, cost, field, l1, trav, pen, goals, p.reach_cells, origin, mpc, cache=cache)
        found += len(poses) > 1
    if (field != nm.UNREACHED).sum() > 2000:
        assert found > 0


@pytest.mark.parametrize("name", ASTAR)
def test_field_is_no_dearer_than_the_reference_search(oracle, name):
    """For every golden pair the reference's search solves: field(start) is finite and at most the reference's own path priced in
    this metric (its 4-connected moves between valid cells are moves of this graph)."""
    m = _maps()["astar_" + name]
    p = _astar_params()
    l1 = _l1("astar_" + name)
    h, w = l1.shape
    trav, pen = nm.tables(nm.dist_table(w, h), p)
    dist = oracle.set_distances(m["cells"], m["mpc"], CPM, m["origin"])
    checked = 0
    for i, row in enumerate(helpers.load_astar_cases()[name]):
        if (name, i) == ("narrow", 2):                 # 2.6e8 pops of the reference's algorithm to answer "no path" (test_gpu_parity.py)
            continue
        path, _ = oracle.search(oracle.pose(*row["start"], 0.0), oracle.pose(*row["goal"], 0.0), dist, m["mpc"], CPM, m["origin"], 0.1, 1.0)
        if len(path) <= 1:
            continue
        goal = nm.pose_cell(row["goal"], m["origin"], CPM, w, h)
        start = nm.pose_cell(row["start"], m["origin"], CPM, w, h)
        field = nm.dijkstra(l1, trav, pen, [goal], 0)
        tcell, _ = nm.cell_tables(l1, trav, pen)
        mask, _ = nm.goal_set(tcell, [goal], 0)
        cells = [start] + [(int(round((float(q["x"]) - float(m["origin"][0])) / float(m["mpc"]))),
                            int(round((float(q["y"]) - float(m["origin"][1])) / float(m["mpc"])))) for q in path[1:]]
        if cells[1] == cells[0]:
            cells = cells[1:]
        assert cells[-1] == goal, (name, i)
        ref_cost = nm.path_cost(cells, nm.allowed_moves(tcell), nm.cell_tables(l1, trav, pen)[1], mask)
        assert ref_cost is not None, (name, i)
        mine = int(field[start[1], start[0]])
        assert mine != nm.UNREACHED and mine <= ref_cost, (name, i, mine, ref_cost)
        checked += 1
    print(name, "pairs checked:", checked)
    if name in ("narrow", "wide", "convex", "maze"):
        assert checked > 0


@pytest.mark.parametrize("name", ["filled", "astar_filled", "astar_empty", "empty"])
def test_filled_and_all_free_maps_reach_nothing(name):
    """`filled`: every cell is a source, nothing is traversable.  An all-free map has no source at all: the distance grid shows -1
    everywhere, the search calls every cell invalid, and so does the field."""
    l1 = _l1(name)
    h, w = l1.shape
    p = _astar_params(reach_cells=2)
    trav, pen = nm.tables(nm.dist_table(w, h), p)
    goals = [(w // 2, h // 2), (3, 4)]
    field = nm.dijkstra(l1, trav, pen, goals, p.reach_cells)
    assert (field == nm.UNREACHED).all()
    assert nm.certificate(field, l1, trav, pen, goals, p.reach_cells) is None
    m = _maps()[name]
    for xy in ((0.0, 0.0), (1.0, -2.0), (100.0, 0.0)):
        poses, label, cost = nm.descend(field, l1, trav, pen, goals, p.reach_cells, (5, xy[0], xy[1], 0.5), m["origin"], m["mpc"], CPM)
        assert len(poses) == 1 and label == -1 and cost == nm.UNREACHED
