"""Hand-built inputs of the range table's tests (tests/test_range_table_model_cpu.py, tests/test_gpu_range_table*.py).  A build case
is a dict: cells (int8 [H][W]), origin, mpc, cpm, hn, reach, params (beam_model.params(...)), D (the model's directions) and table (the
model's table on them, computed once per case and shared: nothing may change it).  Each builder asserts from the model alone that the
case reaches what it is built for.  The scoring cases are beam_cases' with a table beside them."""
import functools

import numpy as np

import beam_cases as bc
import beam_model as bm
import range_table_model as rm

F32 = np.float32
MPC, CPM = bc.MPC, bc.CPM


def cpm_for(reach):
    """The beam model takes no max_range <= 0.15 m: a reach below 4 cells needs cells larger than MPC."""
    return CPM if reach >= 4 else 2.0


def range_for(reach, cpm=CPM):
    """A max_range whose reach at cpm is `reach` cells exactly."""
    mr = (reach - 0.5) / cpm
    assert bm.params_ok(bm.params(max_range=mr)) and bm.reach_cells(bm.params(max_range=mr), cpm) == reach
    return mr


def build_case(cells, hn, reach, **prm):
    cpm = cpm_for(reach)
    p = bm.params(**dict(dict(max_range=range_for(reach, cpm)), **prm))
    cells = np.ascontiguousarray(cells, dtype=np.int8)
    D = rm.directions(reach, hn)
    c = dict(cells=cells, origin=(F32(0), F32(0)), mpc=1.0 / cpm, cpm=cpm, hn=hn, reach=reach, params=p, D=D, table=rm.build(cells, D, p["occ_min"]))
    c["table"].setflags(write=False)
    return c


def _blobs(w, h, seed, n=6, level=100):
    rng = np.random.default_rng(seed)
    cells = np.full((h, w), -20, np.int8)
    for _ in range(n):
        x, y = int(rng.integers(0, w)), int(rng.integers(0, h))
        cells[y:y + 2, x:x + 3] = level
    return cells


@functools.lru_cache(maxsize=None)
def single_cell(occupied, reach):
    c = build_case(np.full((1, 1), 100 if occupied else -20, np.int8), 64, reach)
    assert (c["table"] == (0 if occupied else rm.NONE)).all()
    return c


@functools.lru_cache(maxsize=None)
def strip(w, h, hn, reach):
    """One row or one column with two obstacles: only the two headings along it see anything but the start cell."""
    n = max(w, h)
    cells = np.full((h, w), -20, np.int8)
    cells.reshape(-1)[[n // 3, n - 2]] = 100
    c = build_case(cells, hn, reach)
    t = c["table"].reshape(n, hn)
    along = (0, hn // 2) if h == 1 else (hn // 4, 3 * hn // 4)
    assert t[0, along[0]] == (4 * (n // 3) if reach > n // 3 else rm.NONE) and t[0, along[1]] == rm.NONE
    assert t[n - 1, along[1]] == (4 if reach > 1 else rm.NONE) and (t[n // 3] == 0).all()
    return c


@functools.lru_cache(maxsize=None)
def room(w, h, hn, reach, occ_min=1):
    """A walled room with blobs; at occ_min 2 some blobs hold occ_min - 1 and are not seen."""
    cells = bc.room(w, h)
    blobs = _blobs(w, h, seed=w + hn)
    cells[blobs > 0] = 100
    weak = _blobs(w, h, seed=w + hn + 1, n=4, level=occ_min - 1 if occ_min > 1 else 1)
    cells[(weak > -20) & (cells < 0)] = occ_min - 1 if occ_min > 1 else 1
    c = build_case(cells, hn, reach, occ_min=occ_min)
    t = c["table"]
    assert (t[cells >= occ_min] == 0).all() and ((t != rm.NONE) & (t > 0)).any()
    if occ_min > 1:
        assert (cells == occ_min - 1).any() and (t[cells == occ_min - 1] != 0).any()
    if (reach - 1) * (reach - 1) > w * w + h * h:                           # longer than the diagonal: every ray ends on a wall
        assert (t != rm.NONE).all()
    else:
        assert (t == rm.NONE).any()
    return c


@functools.lru_cache(maxsize=None)
def long_reach():
    """8 x 8, a reach of 4096 cells, 1024 headings: directions with members of +-4096, walks that leave the grid after a few cells."""
    cells = np.full((8, 8), -20, np.int8)
    cells[6, 1] = cells[2, 5] = 100
    c = build_case(cells, 1024, 4096)
    assert np.abs(c["D"]).max() == 4096 and (c["table"] == rm.NONE).any() and ((c["table"] > 0) & (c["table"] != rm.NONE)).any()
    return c


@functools.lru_cache(maxsize=None)
def uniform(occupied):
    c = build_case(np.full((9, 20), 100 if occupied else -20, np.int8), 64, 5)
    assert (c["table"] == (0 if occupied else rm.NONE)).all()
    return c


@functools.lru_cache(maxsize=None)
def far_cell(hn=64, reach=9):
    """Obstacles exactly at the far cell of the axis and diagonal headings from (15, 15) (k = K: not seen) and, from (45, 15), one cell
    short of it (k = K - 1: seen)."""
    cells = np.full((31, 61), -20, np.int8)
    c0 = build_case(cells, hn, reach)
    for h in range(0, hn, hn // 8):
        dx, dy = (int(v) for v in c0["D"][h])
        cells[15 + dy, 15 + dx] = 100
        cells[15 + dy - np.sign(dy), 45 + dx - np.sign(dx)] = 100
    c = build_case(cells, hn, reach)
    for h in range(0, hn, hn // 8):
        dx, dy = (int(v) for v in c["D"][h])
        assert c["table"][15, 15, h] == rm.NONE, h
        assert c["table"][15, 45, h] == int(bm.quarter(dx - np.sign(dx), dy - np.sign(dy), 0, 0)), h
    return c


def changed(c, edits):
    """A copy of the case's cells with `edits` = [(x, y, value), ...] applied (value None: occupied turns free and free occupied), and
    the bounding box of the edits."""
    cells = c["cells"].copy()
    for x, y, v in edits:
        cells[y, x] = v if v is not None else (-20 if cells[y, x] >= c["params"]["occ_min"] else 100)
    xs, ys = [e[0] for e in edits], [e[1] for e in edits]
    return cells, (min(xs), min(ys), max(xs), max(ys))


def score_case(c, hn):
    """A beam case with the model's directions and table for `hn` headings beside it."""
    reach = bm.reach_cells(c["params"], c["cpm"])
    D = rm.directions(reach, hn)
    return dict(c, hn=hn, reach=reach, D=D, table=rm.build(c["cells"], D, c["params"]["occ_min"]))
