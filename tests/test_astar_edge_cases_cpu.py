"""The inputs of tests/astar_edge_cases.py on the CPU: the oracle and the model agree on every one, and every one reaches the edge it
is named for -- a refused push, an fCost within a few of INT16_MAX, an open list that drains, a border or corner pop.  What the GPU
test (tests/test_gpu_astar_edges.py) compares the kernels with is therefore known to be there.  No GPU."""
import json

import numpy as np
import pytest

import astar_edge_cases as ec


_models = {}


def _model(oracle, case, **kw):
    r = ec.reference(oracle, case)
    if not kw:
        if case.name not in _models:
            _models[case.name] = _model(oracle, case, cap=None)
        return _models[case.name]
    return ec.model(r["dist"], ec.world(case.world).origin, case.start, case.goal, case.params, **kw)


@pytest.mark.parametrize("case", ec.CORRIDOR_CASES + ec.EARLY_EXIT_CASES + [ec.RING_CHECKED], ids=lambda c: c.name)
def test_oracle_equals_model_and_the_case_reaches_its_edge(oracle, case):
    r = ec.reference(oracle, case)
    m = _model(oracle, case)
    assert (m["pops"], m["pushes"], m["poses"]) == (*r["stats"], len(r["path"])) == tuple(case.expect)
    assert m["found"] == (len(r["path"]) > 1)
    assert m["pops"] <= ec.MAX_POPS                       # a condition: the GPU test runs every case in six forms
    ec.check_want(case, m)
    if case.want and case.want["found"] is False:
        assert m["pops"] == m["pushes"] + 1               # drained: every entry that went in came out
    if case in ec.EARLY_EXIT_CASES:
        assert r["stats"] == (0, 0) and len(r["path"]) == 1


def test_the_cut_is_the_int16_rule_and_nothing_else(oracle):
    """Over the corridor cases: a push was refused in most, the largest fCost pushed is 32 760 .. 32 766 (keys 65 528 .. 65 534 beside the
    0xFFFF sentinel of k_astar2), both parameter sets have a goal one cell too far, and the control case refuses nothing although its
    list is the longest."""
    ms = {c.name: _model(oracle, c) for c in ec.CORRIDOR_CASES}
    assert sum(m["refused"] > 0 for m in ms.values()) >= 9
    assert max(m["f_max"] for m in ms.values() if m["f_max"] is not None) == 32764
    assert sum(32760 <= m["f_max"] < 32767 for m in ms.values() if m["f_max"] is not None) >= 7
    assert ms["h15_centre_d3262"]["refused"] == 0 and ms["h15_centre_d3262"]["longest"] == max(m["longest"] for m in ms.values())
    assert ms["h9_d3277"]["pops"] == ms["h9_ref_d3357"]["pops"] == 1
    # the drained lists fall from the deep regime (> 16 383 entries), from the LDS regime and from below 256 entries
    assert ms["h15_wall10_bx3200"]["longest"] > 16383 > ms["h15_wall10_bx1700"]["longest"] > 4095 > 255 >= ms["h15_wall10_bx40"]["longest"]
    # ... and the searches that hold ONE entry for thousands of iterations
    assert ms["h9_d3276"]["short_iterations"] == 3276 and ms["h9_ref_d3356"]["short_iterations"] == 3356


@pytest.mark.parametrize("case", ec.TWIN_CASES, ids=lambda c: c.name)
def test_the_160_row_twin_equals_its_plain_corridor(oracle, case):
    """rows of occupied cells below the corridor change no distance inside it: same poses, pops and pushes, on a grid of more than
    524 288 cells"""
    plain = next(c for c in ec.CORRIDOR_CASES if c.name == case.twin_of)
    a, b = ec.reference(oracle, case), ec.reference(oracle, plain)
    assert a["dist"].size == 544000 > 524288
    assert a["stats"] == b["stats"] == tuple(plain.expect[:2])
    assert a["path"].tobytes() == b["path"].tobytes()
    H = ec.world(plain.world).cells.shape[0]
    assert np.array_equal(a["dist"][:H - 1].view(np.uint32), b["dist"][:H - 1].view(np.uint32))


def test_capacity_count_of_the_model(oracle):
    """where a 16 384-entry list ends the h15_centre_d3270 search: the pop of the refusing iteration counted, the refused push not, so
    the list holds pushes + 1 - pops = capacity entries; and without a capacity the search goes on to 19 740 entries"""
    case = next(c for c in ec.CORRIDOR_CASES if c.name == "h15_centre_d3270")
    m = _model(oracle, case, cap=16384)
    pops, pushes = m["capacity_at"]
    assert (pops, pushes) == (11235, 27618) and pushes + 1 - pops == 16384 and not m["found"]
    assert _model(oracle, case, cap=19740)["capacity_at"] is None


def test_ring_pairs_are_what_the_oracle_says_today(oracle):
    rows = json.load(open(ec.RING_JSON))
    cases = ec.ring_cases()
    assert len(cases) == len(rows) >= 16
    for ring in (ec.RING_SMALL, ec.RING_LARGE):
        mine = [c for c in cases if c.world == ring]
        assert len(mine) >= 8
        cells = ec.world(ring).cells
        H, W = cells.shape
        assert (cells[0] < 0).all() and (cells[-1] < 0).all() and (cells[:, 0] < 0).all() and (cells[:, -1] < 0).all()     # the border is free
        corners, moves = set(), set()
        for c in mine:
            r = ec.reference(oracle, c)
            m = _model(oracle, c)
            assert (*r["stats"], len(r["path"])) == tuple(c.expect) == (m["pops"], m["pushes"], m["poses"]), c.name
            assert m["found"] and 0 < m["pops"] <= ec.MAX_POPS and m["border_pops"] > 0, c.name
            corners |= set(m["corner_pops"]); moves.add(m["last_move"])
        assert corners == {(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)}                      # a pop of each corner cell
        assert moves == {(1, 0), (-1, 0), (0, 1), (0, -1)}                                      # goals entered from all four sides
    assert ec.world(ec.RING_LARGE).cells.size > 524288
    # a goal pose less than a cell outside the grid is a goal in column 0 / row 0 (the truncating cast), and found
    beside = [c for c in cases if c.goal[0] < c.world[4] or c.goal[1] < c.world[5]]
    assert len(beside) == 6 and all(c.expect[2] > 1 for c in beside)
