"""The model of the Euclidean distance grid (tests/edt_model.py) against the definition and against the L1 grid, on the CPU; and the
diagonal-gap case, where the two grids disagree about a passage, through the navigation field's model."""
import math

import numpy as np
import pytest

import edt_model as em
import helpers
import nav_field_model as nm

RS = (1, 2, 3, 7, 64, 255)
GAP_PARAMS = nm.Params(0.2, 1.0, 1.0, obstacle_gain=50, reach_cells=0)
GAP_GOAL, GAP_START = (20, 35), (20, 5)
GAP_R = 64
GAP_L1_FIELD_AT_START = 646


def random_grids(n=300, seed=11):
    """n grids from 1 x 1 to 39 x 39, densities from no source to all sources, each with an R of RS."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        w, h = (1, 1) if i == 0 else (39, 39) if i == 1 else (int(rng.integers(1, 40)), int(rng.integers(1, 40)))
        density = (0.0, 1.0, 0.002, 0.02, 0.2, 0.7)[i % 6] if i >= 12 else (0.0 if i % 2 == 0 else 1.0)
        cells = np.where(rng.random((h, w)) < density, 100, -50).astype(np.int8)
        if density > 0 and density < 1 and i % 5 == 0:
            cells[rng.integers(0, h), rng.integers(0, w)] = 0          # log-odds 0 is a source
        out.append((cells, RS[i % len(RS)]))
    return out


def gap_cells(offset=5):
    """40 x 40 free cells and two walls whose ends stand `offset` cells apart in x and in y: a gap the L1 grid calls 2 * offset cells
    wide and that is offset * sqrt(2) cells wide."""
    cells = np.full((40, 40), -50, np.int8)
    cells[18, 0:18] = 100
    cells[18 + offset, 17 + offset:40] = 100
    return cells


def gap_fields(offset):
    """(L1 field, Euclidean field) of the gap case by the model."""
    cells = gap_cells(offset)
    l1 = nm.l1_distances(cells)
    trav, pen = nm.tables(nm.dist_table(40, 40), GAP_PARAMS)
    f_l1 = nm.dijkstra(l1, trav, pen, [GAP_GOAL], 0)
    code = em.codes(cells, GAP_R)
    et, ep = nm.tables(em.table(GAP_R, 0.05), GAP_PARAMS)
    f_eu = nm.dijkstra(code, et, ep, [GAP_GOAL], 0)
    return f_l1, f_eu


def test_model_equals_brute_force_on_random_grids():
    seen = set()
    for cells, R in random_grids():
        a, b = em.codes(cells, R), em.brute_force(cells, R)
        assert a.dtype == np.uint16 and np.array_equal(a, b), (cells.shape, R)
        seen.add(R)
        src = cells >= 0
        if not src.any():
            assert (a == em.NONE16).all()
        else:
            assert np.array_equal(a == 0, src) and int(a.max()) <= em.far(R)
    assert seen == set(RS)


def test_sandwich_between_l1_and_l1_squared_on_the_golden_maps():
    """L2 <= L1 <= sqrt(2) L2 cell by cell: code <= L1^2 <= 2 code wherever both are finite and the code is not FAR."""
    maps = helpers.load_reference_maps()
    R = 64
    checked = 0
    for name in helpers.ALL_MAPS:
        cells = maps[name]["cells"]
        l1 = nm.l1_distances(cells).astype(np.int64)
        code = em.codes(cells, R).astype(np.int64)
        assert np.array_equal(l1 == nm.NONE16, code == em.NONE16), name
        ok = (l1 != nm.NONE16) & (code <= R * R)
        assert (code[ok] <= l1[ok] ** 2).all() and (l1[ok] ** 2 <= 2 * code[ok]).all(), name
        assert np.array_equal(code == 0, l1 == 0), name
        checked += int(ok.sum())
    assert checked > 100000


@pytest.mark.parametrize("R,mpc", [(1, 0.05), (3, 0.05), (64, 0.05), (254, 0.05), (64, 0.1), (20, 0.025), (7, 1.0 / 3.0)])
def test_table_equals_a_math_sqrt_loop(R, mpc):
    f = em.table(R, mpc)
    assert f.dtype == np.float32 and len(f) == R * R + 2
    m = float(np.float32(mpc))
    exp = np.array([np.float32(math.sqrt(float(k)) * m) for k in range(R * R + 2)], np.float32)
    assert f.tobytes() == exp.tobytes()
    assert f[0] == 0 and (np.diff(f) > 0).all()                   # strictly increasing: f[FAR] bounds a far cell from below
    code = np.array([[0, 1, R * R, R * R + 1, em.NONE16]], np.uint16)
    assert em.floats(code, f).tobytes() == np.array([[f[0], f[1], f[R * R], f[R * R + 1], -1.0]], np.float32).tobytes()


def test_nearest_traversable_cell_is_metric():
    """At 5 cm and 0.2 m the L1 rule admits a cell 0.1118 m from an obstacle; the Euclidean table admits none nearer than 0.2 m."""
    maps = helpers.load_reference_maps()
    p = nm.Params(0.2, 2.0, 1.0)
    f = em.table(64, 0.05)
    trav, _ = nm.tables(f, p)
    first = int(np.flatnonzero(trav)[0])
    assert first == 17 and float(f[first]) > 0.2 and not trav[16]                # 16 = 4^2 is 0.2 m exactly: not farther than 0.2
    cells = maps["obstacle_slam_10mx10m_5cm"]["cells"]
    code = em.codes(cells, 64)
    tcell, _ = nm.cell_tables(code, trav, np.zeros(len(trav), np.int32))
    l1 = nm.l1_distances(cells)
    lt, _ = nm.tables(nm.dist_table(200, 200), p)
    l1cell, _ = nm.cell_tables(l1, lt, np.zeros(len(lt), np.int32))
    assert int(l1cell.sum()) == 2134 and int(tcell.sum()) == 1438 and not (tcell & ~l1cell).any()
    assert int(code[l1cell].min()) == 5                                         # offset (1, 2): 0.1118 m


def test_diagonal_gap_through_the_field_model():
    f_l1, f_eu = gap_fields(5)
    sx, sy = GAP_START
    assert int(f_l1[sy, sx]) == GAP_L1_FIELD_AT_START
    assert int(f_eu[sy, sx]) == nm.UNREACHED
    assert int(f_eu[GAP_GOAL[1], GAP_GOAL[0]]) == 0
    f_l1, f_eu = gap_fields(7)
    assert int(f_l1[sy, sx]) != nm.UNREACHED and int(f_eu[sy, sx]) != nm.UNREACHED
    assert int(f_eu[sy, sx]) >= int(f_l1[sy, sx])
