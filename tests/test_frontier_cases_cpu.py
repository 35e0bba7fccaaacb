"""tests/frontier_cases.py without a GPU: every case reaches the kernel path it is built for (each condition printed as a count; a
count of 0 fails), the model that says so returns the oracle's frontier lists, and the corridor trees have the level widths the
cases rely on."""
import numpy as np
import pytest

import frontier_cases as fc
import helpers


def _same(got, exp):
    assert len(got) == len(exp), (len(got), len(exp))
    for k, (a, b) in enumerate(zip(got, exp)):
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), f"frontier {k} differs"


@pytest.mark.parametrize("case", fc.CASES, ids=repr)
def test_case_reaches_its_path_and_the_model_equals_the_oracle(oracle, case):
    cells = case.cells()
    origin, mpc = fc.frame(cells.shape)
    px, py = case.pose(cells.shape)
    assert fc.cell_of_pose(cells.shape, (px, py)) == tuple(case.robot)
    m = case.model()
    for min_len in (0.1, 0.35):
        exp = oracle.find_frontiers(cells, mpc, helpers.CPM_DEFAULT, origin, oracle.pose(px, py, 0.0), min_len)
        _same(m.lists(min_len), exp)
    print(f"{case.name}: {m.W} x {m.H}, reached {m.reached}, levels {m.levels}, widest level {max(m.flood_widths)}, frontiers {len(m.frontiers)}, "
          f"largest {m.largest_frontier()}, touched {m.n_touched}, frontier-class {m.n_frontier_class}, widest growth level "
          f"{m.widest_growth_level()}, largest backlog {m.largest_backlog()}")
    counts = case.reaches(m)
    for what, count in counts.items():
        print(f"    {what}: {count}")
    assert counts and all(v > 0 for v in counts.values()), counts
    assert m.sweep_kernel() == case.sweep
    assert (m.W * m.H <= fc.FR_CLS_LDS) == (case.sweep == 0)


def _tree_model(S, L, value, field):
    cells, (cx, cy), _ = fc.corridor_tree(S, S, L, value, field)
    if value == -3:
        cells[cy - 1, cx] = -50
        return fc.Model(cells, (cx, cy - 1))
    return fc.Model(cells, (cx, cy))


def test_flood_widths_of_the_corridor_trees():
    """4-connected, robot on the root, tree of -50 in a field of 60"""
    w = _tree_model(260, fc.L260, -50, 60).flood_widths
    assert max(w) == 4096 and sum(1 for v in w if v > 1024) == 4
    w = _tree_model(300, fc.L300, -50, 60).flood_widths
    assert max(w) == 5120 and sum(1 for v in w if v > 4096) == 1 and sum(1 for v in w if v > 1024) == 16
    w = _tree_model(520, fc.L520, -50, 60).flood_widths
    assert (sum(1 for v in w if 1024 < v <= 4096), sum(1 for v in w if 4096 < v <= 8192), sum(1 for v in w if v > 8192)) == (8, 2, 2)
    assert max(w) == 16384 and len(w) == 509


def test_growth_widths_of_the_corridor_trees():
    """8-connected, tree of -3 in a field of 60 and one free robot cell beside the root: one frontier each"""
    for S, L, cells, backlog, widest in ((160, fc.L_A, 6673, 1534, 1536), (160, fc.L_B, 5953, 1534, 1536),
                                         (260, fc.L260, 24193, None, 6144), (300, fc.L300, 49489, None, 5888)):
        m = _tree_model(S, L, -3, 60)
        assert len(m.frontiers) == 1 and len(m.frontiers[0]) == cells
        assert m.widest_growth_level() == widest
        assert backlog is None or m.largest_backlog() == backlog


@pytest.mark.parametrize("shape", fc.LATTICES + [(3, 33), (315, 313)])
def test_lattice_has_a_frontier_per_2x2_block(oracle, shape):
    H, W = shape
    cells = fc.lattice(W, H)
    origin, mpc = fc.frame(shape)
    px, py = fc.pose_of_cell(shape, (1, 1))
    exp = oracle.find_frontiers(cells, mpc, helpers.CPM_DEFAULT, origin, oracle.pose(px, py, 0.0), 0.0)
    blocks = ((W + 1) // 2) * ((H + 1) // 2)
    assert len(exp) == blocks and all(len(f) == 1 for f in exp)
    print(f"{W} x {H}: {blocks} frontiers, {W * H // 4 + 4} entries before, {W * H // 2 + 1} now")
    assert blocks <= W * H // 2 + 1                            # frontier_table_entries (bl_frontiers.hip)
    m = fc.Model(cells, (1, 1))
    _same(m.lists(0.0), exp)
    assert m.reached == W * H - blocks


def test_the_table_bound_holds_for_every_shape():
    """ceil(W/2) * ceil(H/2) <= cells / 2 + 1 for every W x H <= cells: the table follows from the allocation alone"""
    for cells in list(range(1, 400)) + [98304, 98306]:
        worst = max(((w + 1) // 2) * ((cells // w + 1) // 2) for w in range(1, cells + 1))
        assert worst <= cells // 2 + 1, (cells, worst)


def test_grow_set_model_agrees_with_the_set_model_test():
    """fg_home restated twice (here for arrays): the same homes"""
    import test_frontier_set_model_cpu as sm
    c = np.array([0, 1, 17, 98305, 5 * 10946 + 17, (1 << 28) - 1], np.int64)
    assert fc.fg_home(c).tolist() == [sm.fg_home(int(v)) for v in c]
    assert (fc.FG_SLOTS, fc.FG_PAD, fc.FG_DMAX, fc.FG_CELL_MAX) == (sm.FG_SLOTS, sm.FG_PAD, sm.FG_DMAX, sm.FG_CELL_MAX)
