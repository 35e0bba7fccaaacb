"""tests/nav_field_cases.py checked on the CPU, with the model alone: every case is what it claims to be -- the corner variants differ
in the model, round 1 of the big grid lists more tiles than a round has workgroups, the strips' far tile is 130 tile steps from the
goal's, the edge starts land in the cells they are meant for.  tests/test_gpu_nav_field_edges.py runs the same cases on the device."""
import math

import numpy as np
import pytest

import nav_field_cases as nc
import nav_field_model as nm


@pytest.mark.parametrize("shape", nc.SMALL_SHAPES)
def test_small_grids(shape):
    h, w = shape
    name = nc.small_name(h, w)
    l1, trav, pen, goals, p, field = nc.solved(name)
    assert l1.shape == (h, w) and l1[0, 0] == 0 and l1[h - 1, w - 1] == h + w - 2
    tcell, _ = nm.cell_tables(l1, trav, pen)
    assert int(tcell.sum()) == h * w - 1 and not tcell[0, 0]                 # exactly the source cell is not traversable
    assert nm.certificate(field, l1, trav, pen, goals, 0) is None
    for order in ("forward", "reverse"):
        assert np.array_equal(nm.tile_fixed_point(l1, trav, pen, goals, 0, order=order)[0], field), order
    if shape == (1, 1):
        assert field[0, 0] == nm.UNREACHED                                   # the far corner is the source: nothing is reached
    else:
        assert (field != nm.UNREACHED).sum() == h * w - 1 and field[h - 1, w - 1] == 0
    allowed = nm.allowed_moves(tcell)
    if min(h, w) == 1:                                                       # a side of 1: no diagonal move anywhere
        assert not any(a.any() for a in allowed[4:])
    paths = nc.model_paths(name)
    assert len(paths) == h * w - 1 and all(label == 0 and len(poses) >= 1 for poses, label, _ in paths)
    assert max([len(poses) for poses, _, _ in paths], default=0) <= 128     # the cap_each of the GPU test


@pytest.mark.parametrize("d", range(4))
@pytest.mark.parametrize("size,cx,cy", [(s, cx, cy) for s in sorted(nc.CORNERS) for cx, cy in nc.CORNERS[s]])
def test_corner_variants_differ(size, cx, cy, d):
    k = nc.corner_cells(cx, cy, d)
    tiles = {(c[0] // nc.TILE, c[1] // nc.TILE) for c in (k["A"], k["B"], k["X"], k["Y"])}
    assert len(tiles) == 4                                                   # the move, its target and both side cells: four tiles
    at = {}
    for pattern in nc.PATTERNS:
        name = nc.corner_name(size, cx, cy, d, pattern)
        l1, trav, pen, goals, p, field = nc.solved(name)
        assert nm.certificate(field, l1, trav, pen, goals, 0) is None
        at[pattern] = int(field[k["A"][1], k["A"][0]])
        assert at[pattern] != nm.UNREACHED
        (poses, label, cost), = nc.model_paths(name)
        first = nc.path_moves(poses)[0]
        if pattern == "open":
            assert first == k["d"], (name, first)                            # the cheapest way from A is the diagonal through the corner
            assert at[pattern] == int(field[k["B"][1], k["B"][0]]) + 14 + int(nm.cell_tables(l1, trav, pen)[1][k["A"][1], k["A"][0]])
        else:
            assert first != k["d"], (name, first)
        assert label == 0 and cost == at[pattern]
    for pattern in nc.PATTERNS[1:]:
        assert at[pattern] > at["open"], (pattern, at)


def test_big_grid_lists_more_tiles_than_a_round_has_workgroups():
    c = nc.case("big")
    h, w = nc.world("big").cells.shape
    tx_n, ty_n = math.ceil(w / nc.TILE), math.ceil(h / nc.TILE)
    assert (h, w) == (1024, 1056) and tx_n * ty_n == 1056 == len(c.goals)
    tcell = nc.traversable("big", c.params)
    mask, label = nm.goal_set(tcell, c.goals, 0)
    assert int(mask.sum()) == 1056
    per_tile = mask.reshape(ty_n, nc.TILE, tx_n, nc.TILE).sum(axis=(1, 3))
    assert (per_tile == 1).all()                                             # a goal cell in every tile: round 1 lists all 1056
    relax_grid = nc.relax_grid_of_the_source()
    assert relax_grid == 1024, "NAV_RELAX_GRID changed: choose a grid of more tiles than that, or the second-tile loop goes untested"
    assert tx_n * ty_n > relax_grid
    share = 1.0 - tcell.mean()
    assert 0.025 < share < 0.035
    # the same grid carries the edge of the 32-bit guard
    n = h * w
    assert n * (14 + nc.GAIN_LAST_OK) <= 4294967294 < n * (14 + nc.GAIN_LAST_OK + 1)
    e = nc.case("big_gain_edge")
    trav, pen = nc.tables("big", e.params)
    assert list(pen[:6]) == [0, nc.GAIN_LAST_OK, nc.GAIN_LAST_OK, nc.GAIN_LAST_OK, nc.GAIN_LAST_OK, 0]     # exponent 0: the whole gain up to L1 distance 4


def test_strip_far_tile_is_130_tile_steps_from_the_goal():
    for name, far in (("strip", (15, nc.STRIP_ROWS - 1)), ("strip_t", (0, 15))):
        c = nc.case(name)
        cells = nc.world(name).cells
        assert sorted(cells.shape) == [32, 4192]
        assert nc.tile_steps(c.goals[0], far) == 130
        assert nc.traversable(name, c.params)[c.goals[0][1], c.goals[0][0]]
    c = nc.case("strip")
    cells = nc.world("strip").cells
    assert (cells[:, 0] == nc.SOURCE).all() and (cells[:, 31] == nc.SOURCE).all() and (cells[5, 10:20] == nc.FREE).all()
    l1, trav, pen, goals, p, field = nc.solved("strip")
    assert nm.certificate(field, l1, trav, pen, goals, 0) is None
    assert (field[-nc.TILE:] != nm.UNREACHED).any()                          # the wave does arrive in the far tile: 130 rounds at least
    assert 4 + 8 + 16 + 32 + 64 < 130                                        # ... which is beyond the groups that grow


def test_short_strip_tile_sweeps_equal_dijkstra():
    l1, trav, pen, goals, p, field = nc.solved("strip_short")
    assert l1.shape == (1056, 32) and np.array_equal(nc.world("strip_short").cells, nc.world("strip").cells[:1056])
    assert (field[-nc.TILE:] != nm.UNREACHED).any()
    for order in ("forward", "reverse"):
        got, rounds = nm.tile_fixed_point(l1, trav, pen, goals, 0, order=order)
        assert np.array_equal(got, field), order
        assert rounds >= 32, (order, rounds)


def test_serpentine_is_one_corridor():
    cells = nc.world("serpentine").cells
    free = cells == nc.FREE
    assert free[0::2, 1:63].all() and free[1::2].sum(axis=1).tolist() == [1] * 32
    # the corridor crosses the border between the tile columns in every even row: 16 times per tile row
    assert free[0::2, 31].all() and free[0::2, 32].all()
    l1, trav, pen, goals, p, field = nc.solved("serpentine")
    assert nm.certificate(field, l1, trav, pen, goals, 0) is None
    assert (field[free] != nm.UNREACHED).all()
    poses, label, cost = nc.model_paths("serpentine")[nc.FAR_START]
    moves = nc.path_moves(poses)
    assert all(dx == 0 or dy == 0 for dx, dy in moves)                       # no diagonal move fits the corridor
    assert len(poses) == 1 + 32 * 61 + 31 * 2 and label == 0                 # 32 runs of 61 steps along a row, 31 times 2 steps through a gap
    assert cost == int(field[:63][free[:63]].max())                          # the far end (below it there is only a dead-end cell in the last wall)


@pytest.mark.parametrize("name", ["strip", "serpentine"])
def test_path_batches_mix_long_and_short(name):
    c = nc.case(name)
    assert len(c.starts) == 70 > 64
    paths = nc.model_paths(name)
    lens = [len(poses) for poses, _, _ in paths]
    L = lens[nc.FAR_START]
    assert L == max(lens) and L > 1000 and sorted(lens)[-2] < L - 1          # at cap L - 1 exactly one path is cut off
    assert lens[0] == 1 and paths[0][2] == 0                                 # a start on the goal cell
    assert sum(1 for v in lens if v > 2) >= 60 and sum(1 for v in lens if v <= 2) >= 1     # at cap 2: cut-off and whole paths side by side
    assert all(label == 0 for _, label, _ in paths)


def test_edge_starts_land_where_they_are_meant_to():
    c = nc.case("edge_starts")
    w = nc.world("open40")
    l1, trav, pen, goals, p, field = nc.solved("edge_starts")
    tcell, _ = nm.cell_tables(l1, trav, pen)
    assert tcell[0, 0] and tcell[0, :].all() and tcell[:, 0].all() and int(tcell.sum()) == 1599
    paths = nc.model_paths("edge_starts")
    for ((cx, cy), want), start, (poses, label, cost) in zip(nc.EDGE_STARTS, c.starts, paths):
        vx, vy = nc.cell_coordinate(w.origin, start[1], 0), nc.cell_coordinate(w.origin, start[2], 1)
        got = nm.pose_cell((start[1], start[2]), w.origin, nc.CPM, 40, 40)
        assert got == want, ((cx, cy), got)
        for v, want_c, asked in ((vx, want and want[0], cx), (vy, want and want[1], cy)):
            if asked < 0 and asked > -1:
                assert -1.0 < v < 0.0 and want_c == 0, (asked, v)            # after the float32 rounding still inside (-1, 0): truncates to 0
            elif asked == -1.0:
                assert v <= -1.0, (asked, v)
            elif asked == 40.0:
                assert v >= 40.0, (asked, v)
            elif not math.isfinite(asked):
                assert not math.isfinite(v)
        if want is None or want == (20, 20):
            assert len(poses) == 1 and label == -1 and cost == nm.UNREACHED
        else:
            assert len(poses) > 1 and label == 0 and cost == int(field[want[1], want[0]])
    assert sum(1 for _, want in nc.EDGE_STARTS if want is None) == 10


def test_reach_cases():
    l1, trav, pen, goals, p, field = nc.solved("reach_all")
    tcell, _ = nm.cell_tables(l1, trav, pen)
    mask, label = nm.goal_set(tcell, goals, p.reach_cells)
    assert p.reach_cells == 1024 and np.array_equal(mask, tcell) and (field[tcell] == 0).all() and (label[tcell] == 1).all()
    assert all(len(poses) == 1 for poses, _, _ in nc.model_paths("reach_all"))
    assert sorted({lab for _, lab, _ in nc.model_paths("reach_all")}) == [-1, 1]           # -1: the start on the source cell
    l1, trav, pen, goals, p, field = nc.solved("reach_clipped")
    mask, label = nm.goal_set(nm.cell_tables(l1, trav, pen)[0], goals, p.reach_cells)
    assert int(mask.sum()) == 2 * 16 and mask[:4, :4].all() and mask[36:, 36:].all()      # 7 x 7 windows clipped to 4 x 4
    assert nm.certificate(field, l1, trav, pen, goals, p.reach_cells) is None
