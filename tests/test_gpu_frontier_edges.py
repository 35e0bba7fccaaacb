"""find_map_frontiers on the hand-built maps of tests/frontier_cases.py: the level paths, growth paths and tables no random blob map
reaches (tests/test_frontier_cases_cpu.py shows that each case reaches its path).  The bar is the suite's: the oracle's lists byte for
byte, in order.  Beside the lists: Frontiers.stats() against the model's cells reached and levels, and which kernels swept."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import botlab_amd as bl
import frontier_cases as fc
import helpers

pytestmark = pytest.mark.gpu


def _same_frontiers(got, exp):
    assert len(got) == len(exp), (len(got), len(exp))
    for k, (a, b) in enumerate(zip(got, exp)):
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), f"frontier {k} differs"


def _sweep_kernel_is(fr, case, m):
    """which kernels grew the frontiers: the value the case names -- under BOTLAB_FRONTIER_GROW_V1 the one the model gives for that form"""
    form = os.environ.get("BOTLAB_FRONTIER_GROW_V1")
    want = case.sweep if form is None else m.sweep_kernel(int(form))
    assert fr.sweep_kernel() == want, (fr.sweep_kernel(), want)


@pytest.mark.parametrize("case", fc.CASES, ids=repr)
def test_find_map_frontiers_hand_built_case(oracle, gpu_ctx, case):
    cells = case.cells()
    origin, mpc = fc.frame(cells.shape)
    px, py = case.pose(cells.shape)
    m = case.model()
    grid = bl.OccupancyGrid.from_cells(cells, origin, mpc, cellsPerMeter=helpers.CPM_DEFAULT, ctx=gpu_ctx)
    try:
        for min_len in (0.1, 0.35):
            exp = oracle.find_frontiers(cells, mpc, helpers.CPM_DEFAULT, origin, oracle.pose(px, py, 0.0), min_len)
            fr = bl.find_map_frontiers(grid, bl.make_pose(px, py, 0.0), min_len)
            print(f"{case.name} at {min_len}: {len(fr)} frontiers ({len(exp)}), stats {fr.stats()} ({m.stats()}), sweep kernel {fr.sweep_kernel()}")
            _same_frontiers(fr.cells(), exp)
            assert fr.stats() == m.stats()
            _sweep_kernel_is(fr, case, m)
            fr.close()
    finally:
        grid.close()


def test_find_map_frontiers_tree_and_block_cases_through_the_grow_kernel_without_the_cell_set():
    """BOTLAB_FRONTIER_GROW_V1 = 1, 2: the sweeps of the multi-launch form through k_frontier_grow, whose ring the frontier-valued
    trees overtake too and whose visited set the largest of them overflows (the one-workgroup sweep then grows a wide level) -- a
    fresh child process per value, the tree and block cases of the multi-launch form only (no other case has a growth kernel to choose)."""
    for form in ("1", "2"):
        e = dict(os.environ)
        e["BOTLAB_FRONTIER_GROW_V1"] = form
        subprocess.check_call([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                               "-k", "hand_built_case and (big or block_large or tree520)"], env=e)


# ---- the table of frontier offsets: a context of its own per test (the session's has seen large grids: its table holds millions)
def _find_on(ctx, cells, robot_cell, min_len):
    """(status, lists, sweep kernel) of bl_frontiers_find on `ctx`"""
    origin, mpc = fc.frame(cells.shape)
    px, py = fc.pose_of_cell(cells.shape, robot_cell)
    grid = bl.OccupancyGrid.from_cells(cells, origin, mpc, cellsPerMeter=helpers.CPM_DEFAULT, ctx=ctx)
    try:
        h = C.c_void_p()
        pose = bl.make_pose(px, py, 0.0)
        rc = ctx.lib.bl_frontiers_find(ctx.h, grid.h, C.byref(pose), float(min_len), C.byref(h))
        if rc != 0:
            msg = ctx.lib.bl_last_error()
            return rc, (msg.decode() if msg else ""), -1
        fr = bl.host.Frontiers(ctx, h)
        out = rc, fr.cells(), fr.sweep_kernel()
        fr.close()
        return out
    finally:
        grid.close()


def _oracle_lattice(oracle, shape):
    cells = fc.lattice(shape[1], shape[0])
    origin, mpc = fc.frame(shape)
    px, py = fc.pose_of_cell(shape, (1, 1))
    return cells, oracle.find_frontiers(cells, mpc, helpers.CPM_DEFAULT, origin, oracle.pose(px, py, 0.0), 0.0)


@pytest.mark.parametrize("shape,count", list(zip(fc.LATTICES, (25, 20, 16, 16, 18, 16))), ids=lambda v: str(v).replace(" ", ""))
def test_lattice_of_one_cell_frontiers_on_a_fresh_context(oracle, gpu_ctx, shape, count):
    """a frontier per 2 x 2 block, odd sides: more than cells / 4 + 4 (7 x 7: exactly as many)"""
    cells, exp = _oracle_lattice(oracle, shape)
    assert len(exp) == count
    ctx = bl.Context(0)
    try:
        rc, got, _ = _find_on(ctx, cells, (1, 1), 0.0)
        print(f"lattice {shape[1]} x {shape[0]}: status {rc}, {got if rc else len(got)}")
        assert rc == 0, (rc, got)
        _same_frontiers(got, exp)
    finally:
        ctx.close()


def test_lattice_on_a_scratch_sized_for_another_shape(oracle, gpu_ctx):
    """10 x 10 first, then a 3 x 33 lattice (99 cells: no reallocation) with 34 frontiers"""
    cells, exp = _oracle_lattice(oracle, (3, 33))
    assert len(exp) == 34
    first = np.full((10, 10), -50, np.int8)
    first[4, 4] = 0
    ctx = bl.Context(0)
    try:
        rc, got, _ = _find_on(ctx, first, (1, 1), 0.0)
        assert rc == 0 and len(got) == 1
        rc, got, _ = _find_on(ctx, cells, (1, 1), 0.0)
        print(f"lattice 33 x 3 behind 10 x 10: status {rc}, {got if rc else len(got)}")
        assert rc == 0, (rc, got)
        _same_frontiers(got, exp)
    finally:
        ctx.close()


def test_large_lattice_with_odd_sides(oracle, gpu_ctx):
    """313 x 315 (98 595 cells: the multi-launch form), 24 806 frontiers: more touches than the grow kernels keep, so the one-workgroup
    sweep fills the table"""
    cells, exp = _oracle_lattice(oracle, (315, 313))
    assert len(exp) == 24806
    ctx = bl.Context(0)
    try:
        rc, got, sweep = _find_on(ctx, cells, (1, 1), 0.0)
        print(f"lattice 313 x 315: status {rc}, {got if rc else len(got)}, sweep kernel {sweep}")
        assert rc == 0, (rc, got)
        _same_frontiers(got, exp)
        assert sweep == 1
    finally:
        ctx.close()
