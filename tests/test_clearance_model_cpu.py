"""The clearance grid's model and the leap walk (tests/clearance_model.py), and bl_beam_dev.h's beam_first_hit_leap compiled for the
host (tests/cpp/clearance_dev_ref.cpp), without a GPU.  Every comparison is for equality but the last, a floor.

  * the grid's separable model against the definition word for word (the minimum over all occupied cells): random grids up to 24 x 24,
    caps 1, 2, 7 and 255, all free, all occupied, one cell;
  * the leap walk against the plain Bresenham loop in (first, K, hit cell): every (dx, dy) in -12 .. 12 from every start of a 25 x 25
    grid at three densities, which takes the walks over all four borders; cap 1, where a walk inside the grid makes first + 1 rounds;
    the rounds never exceed the loop's reads;
  * the host-compiled beam_first_hit_leap against beam_first_hit on the same walks, and both against the model;
  * on convex_10mx10m_5cm, cap 255, a reach of 100 cells, 300 random free start cells x 58 headings: the mean rounds are at most a
    quarter of the loop's mean reads (measured: about one sixteenth).  The quarter is a floor under the reason for the walk, not a
    tuning target."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import clearance_model as cm
import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_cells(rng, h, w, density):
    return np.where(rng.random((h, w)) < density, rng.integers(1, 128, (h, w)), rng.integers(-128, 1, (h, w))).astype(np.int8)


# ---------------------------------------------------------------------------------------------------------------- the grid
@pytest.mark.parametrize("cap", [1, 2, 7, 255])
def test_grid_equals_the_definition(cap):
    rng = np.random.default_rng(cap)
    shapes = [(1, 1), (1, 9), (9, 1), (5, 7), (24, 24), (13, 24), (24, 11)]
    seen = set()
    for h, w in shapes:
        for density in (0.02, 0.15, 0.6):
            cells = random_cells(rng, h, w, density)
            for occ_min in (1, 40):
                got = cm.grid(cells, occ_min, cap)
                assert got.dtype == np.uint8 and np.array_equal(got, cm.brute(cells, occ_min, cap)), (h, w, density, occ_min)
                assert np.array_equal(got == 0, cells >= occ_min)
                seen |= set(got.ravel().tolist())
    assert cap in seen and 0 in seen


@pytest.mark.parametrize("cap", [1, 2, 7, 255])
def test_grid_all_free_all_occupied_one_cell(cap):
    free = np.full((24, 17), -5, np.int8)
    assert (cm.grid(free, 1, cap) == cap).all() and np.array_equal(cm.grid(free, 1, cap), cm.brute(free, 1, cap))
    assert (cm.grid(np.full((24, 17), 9, np.int8), 1, cap) == 0).all()
    assert (cm.grid(np.full((24, 17), 9, np.int8), 10, cap) == cap).all()   # all at occ_min - 1
    one = free.copy()
    one[20, 3] = 1
    yy, xx = np.mgrid[0:24, 0:17]
    want = np.minimum(cap, np.maximum(np.abs(xx - 3), np.abs(yy - 20)))
    assert np.array_equal(cm.grid(one, 1, cap), want) and np.array_equal(cm.brute(one, 1, cap), want)
    for v, n in ((-7, 1), (7, 0)):
        assert cm.grid(np.full((1, 1), v, np.int8), 1, cap).tolist() == [[cap if n else 0]]


# ---------------------------------------------------------------------------------------------------------------- the walks
@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("clearance_dev") / "clearance_dev_ref.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-shared", "-fPIC", "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "clearance_dev_ref.cpp")])
    return C.CDLL(so)


def all_walks(n=25, reach=12):
    """Every (dx, dy) in -reach .. reach from every start cell of an n x n grid: sx, sy, tx, ty."""
    sy, sx, dy, dx = np.meshgrid(np.arange(n), np.arange(n), np.arange(-reach, reach + 1), np.arange(-reach, reach + 1), indexing="ij")
    sx, sy, dx, dy = (v.ravel().astype(np.int64) for v in (sx, sy, dx, dy))
    return sx, sy, sx + dx, sy + dy


GRIDS = {}


def walks_case(density):
    """The 25 x 25 grid of a density, its walks and the loop's answers, computed once and left unchanged."""
    if density not in GRIDS:
        rng = np.random.default_rng(int(density * 1000))
        cells = random_cells(rng, 25, 25, density)
        w = all_walks()
        loop = cm.loop_walks(cells, 1, *w)
        for a in (cells,) + w + loop:
            a.setflags(write=False)
        GRIDS[density] = (cells, w, loop)
    return GRIDS[density]


def same_hits(a, b):
    """(first, K) of every walk and the hit cell of every walk that has one."""
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    hit = a[0] < a[1]
    assert np.array_equal(a[2][hit], b[2][hit]) and np.array_equal(a[3][hit], b[3][hit])
    return hit


@pytest.mark.parametrize("density", [0.03, 0.15, 0.5])
@pytest.mark.parametrize("cap", [1, 7, 255])
def test_leap_walk_equals_the_loop_walk(density, cap):
    cells, w, loop = walks_case(density)
    D = cm.grid(cells, 1, cap)
    leap = cm.leap_walks(D, *w)
    hit = same_hits(loop, leap)
    assert hit.any() and (~hit).any() and (loop[0][hit] == 0).any() and (loop[0][hit] == loop[1][hit] - 1).any()
    assert (leap[4] <= loop[4]).all()                                         # rounds never exceed the loop's reads
    sx, sy, tx, ty = w
    left = (np.minimum(tx, ty) < 0) | (np.maximum(tx, ty) > 24)
    for side in (tx < 0, tx > 24, ty < 0, ty > 24):                           # walks leaving over each border, with and without a hit
        assert (side & hit).any() and (side & ~hit).any()
    if cap == 1:                                                              # a walk that stays inside reads every cell up to its hit
        inside_hit = hit & ~left
        assert inside_hit.any() and np.array_equal(leap[4][inside_hit], leap[0][inside_hit] + 1)
        assert np.array_equal(leap[4], loop[4])
    elif density < 0.5:                                                       # some walk leaps (at 0.5 this grid holds no clearance above 1)
        assert (leap[4] < loop[4]).any()


@pytest.mark.parametrize("density", [0.03, 0.15, 0.5])
@pytest.mark.parametrize("cap", [1, 7, 255])
def test_host_compiled_leap_equals_first_hit(ref, density, cap):
    cells, w, loop = walks_case(density)
    D = np.ascontiguousarray(cm.grid(cells, 1, cap))
    walks = np.ascontiguousarray(np.stack(w, axis=1).astype(np.int32))
    n = len(walks)
    a, b = np.zeros((n, 5), np.int32), np.zeros((n, 5), np.int32)
    ref.cd_walks(np.ascontiguousarray(cells).ctypes.data_as(C.c_void_p), D.ctypes.data_as(C.c_void_p), 25, 25, 1, n,
                 walks.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p))
    same_hits(a.T, b.T)                                                       # beam_first_hit_leap against beam_first_hit
    same_hits(a.T, loop)                                                      # ... and both against the model's loop
    assert np.array_equal(a[:, 4], loop[4])
    assert np.array_equal(b[:, 4], cm.leap_walks(D, *w)[4]) and (b[:, 4] <= a[:, 4]).all()


def test_rounds_on_a_real_map_are_a_fraction_of_the_loops_reads():
    cells = helpers.load_reference_maps()["convex_10mx10m_5cm"]["cells"]
    h, w = cells.shape
    rng = np.random.default_rng(300)
    fy, fx = np.nonzero(cells < 1)
    pick = rng.choice(len(fx), 300, replace=False)
    th = 2.0 * math.pi * np.arange(58) / 58.0
    sx, sy = np.repeat(fx[pick], 58).astype(np.int64), np.repeat(fy[pick], 58).astype(np.int64)
    tx = sx + np.tile(np.rint(100 * np.cos(th)).astype(np.int64), 300)
    ty = sy + np.tile(np.rint(100 * np.sin(th)).astype(np.int64), 300)
    loop = cm.loop_walks(cells, 1, sx, sy, tx, ty)
    leap = cm.leap_walks(cm.grid(cells, 1, 255), sx, sy, tx, ty)
    same_hits(loop, leap)
    assert (leap[4] <= loop[4]).all()
    print("cell reads per ray: loop %.2f, leaps %.2f" % (loop[4].mean(), leap[4].mean()))
    assert leap[4].mean() * 4 <= loop[4].mean()
