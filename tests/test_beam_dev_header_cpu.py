"""bl_beam_dev.h compiled for the host (tests/cpp/beam_dev_ref.cpp), without a GPU: the one copy of the rules that k_beam_cast,
k_beam_lookup (bl_beam.hip) and k_rt_build (bl_rangetable.hip) share, against the models (tests/beam_model.py,
tests/range_table_model.py).  Every comparison is for equality.

  * beam_first_hit in both grid-leaving forms (walking on outside the grid as beam_ray does, ending there as k_rt_build does)
    against the closed-form walk the models use: the eight octants and both axes, K = 0, a hit in the start cell and at k = K - 1, an
    occupied end cell, walks that leave over each border and through a corner with occupied cells where an index that wrapped
    round would land, a 1 x 1 grid;
  * beam_quarter at distance 0, (1, 0), (3, 4), the largest legal span and every dx^2 + dy^2 <= 4096 against the integer root;
  * beam_return_p against the model's look-up of a one-cell table: with and without an expected hit, z below, at and above z*,
    |z - z*| at hit_cut and one past it, z >> 2 at 1023 and 1024;
  * beam_lg at 1, 2, 3, 2^30, 2^31 - 1 and both sides of a mantissa step;
  * beam_heading_index at Hn = 64 and 1024: 0, -0.0, +-pi, and the floats round the half-way points between two headings;
  * beam_start: non-finite pose words, a grid position at +-2^30, start cells on each border and one cell outside."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import beam_model as bm
import range_table_model as rm
from obstacle_layer_model import walk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
PI_F = F32(math.pi)                                                       # the float just above pi: what wrap_to_pi lets through


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("beam_dev") / "beam_dev_ref.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-shared", "-fPIC", "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "beam_dev_ref.cpp")])
    lib = C.CDLL(so)
    lib.bd_return_p.restype = C.c_uint32
    lib.bd_return_p.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.bd_lg.argtypes = [C.c_void_p, C.c_uint32, C.c_int]
    lib.bd_heading_index.argtypes = [C.c_int, C.c_void_p, C.c_float, C.c_int, C.c_void_p]
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _tab(ref, t):
    """The block of table words as the kernels hold it, from the model's tables."""
    tab = np.zeros(ref.bd_table_words(), np.uint32)
    for which, name in enumerate(("hit", "short", "lt")):
        at = ref.bd_table_place(which)
        tab[at:at + len(t[name])] = t[name]
    return tab


# ---------------------------------------------------------------------------------------------------------------- the walk
def model_first_hit(cells, occ_min, sx, sy, tx, ty):
    """first, K and the hit cell (None without a hit) by the models' closed-form walk: no cell outside the grid is occupied."""
    H, W = cells.shape
    xs, ys = walk(sx, sy, tx, ty)
    K = max(abs(tx - sx), abs(ty - sy))
    assert len(xs) == K
    for k in range(K):
        x, y = int(xs[k]), int(ys[k])
        if 0 <= x < W and 0 <= y < H and cells[y, x] >= occ_min:
            return k, K, (x, y)
    return K, K, None


def check_walk(ref, cells, sx, sy, tx, ty, occ_min=1):
    cells = np.ascontiguousarray(cells, np.int8)
    H, W = cells.shape
    assert 0 <= sx < W and 0 <= sy < H                                    # the two forms agree for a start cell inside the grid
    first, K, cell = model_first_hit(cells, occ_min, sx, sy, tx, ty)
    for stop in (0, 1):
        out = np.zeros(4, np.int32)
        ref.bd_first_hit(_p(cells), W, H, occ_min, sx, sy, tx, ty, stop, _p(out))
        assert (int(out[0]), int(out[1])) == (first, K), (stop, sx, sy, tx, ty, out.tolist(), first, K)
        if cell is not None:
            assert (int(out[2]), int(out[3])) == cell, (stop, sx, sy, tx, ty, out.tolist(), cell)
    return first, K, cell


def test_first_hit_in_every_octant_and_along_both_axes(ref):
    cells = np.full((21, 21), -20, np.int8)
    ring = np.maximum(np.abs(np.arange(21)[None, :] - 10), np.abs(np.arange(21)[:, None] - 10)) == 7
    cells[ring] = 50
    ends = [(10, 0), (-10, 0), (0, 10), (0, -10),                         # the axes
            (10, 4), (4, 10), (-4, 10), (-10, 4), (-10, -4), (-4, -10), (4, -10), (10, -4),     # one ray inside each octant
            (10, 10), (-10, 10), (-10, -10), (10, -10)]                   # and the diagonals between them
    for dx, dy in ends:
        first, K, cell = check_walk(ref, cells, 10, 10, 10 + dx, 10 + dy)
        assert (first, K) == (7, 10) and max(abs(cell[0] - 10), abs(cell[1] - 10)) == 7
    assert check_walk(ref, cells, 10, 10, 16, 13)[0] == 6                 # ends inside the ring: no hit
    assert check_walk(ref, cells, 10, 10, 20, 14, occ_min=51)[0] == 10    # nothing reaches occ_min


def test_first_hit_towards_every_cell_round_the_start(ref):
    """Every end cell within 8 of the start of a 13 x 13 grid occupied at random: the ties of the loop's two comparisons (2 err = -dy,
    2 err = dx) decide which cell a walk visits, and with it the hit."""
    rng = np.random.default_rng(3)
    cells = np.where(rng.random((13, 13)) < 0.3, 60, -20).astype(np.int8)
    cells[6, 6] = -20
    seen = set()
    for ty in range(-2, 15):
        for tx in range(-2, 15):
            first, K, cell = check_walk(ref, cells, 6, 6, tx, ty)
            seen.add(first < K)
    assert seen == {True, False}


def test_first_hit_at_the_ends_of_the_walk(ref):
    cells = np.full((9, 12), -20, np.int8)
    assert check_walk(ref, cells, 3, 4, 3, 4) == (0, 0, None)             # K = 0: no cell is visited
    occupied_start = cells.copy()
    occupied_start[4, 3] = 1
    assert check_walk(ref, occupied_start, 3, 4, 3, 4) == (0, 0, None)    # ... not even an occupied start cell
    assert check_walk(ref, occupied_start, 3, 4, 9, 6) == (0, 6, (3, 4))  # a hit in the start cell
    xs, ys = walk(3, 4, 9, 6)
    last = cells.copy()
    last[int(ys[5]), int(xs[5])] = 1
    assert check_walk(ref, last, 3, 4, 9, 6) == (5, 6, (int(xs[5]), int(ys[5])))      # a hit at k = K - 1
    end = cells.copy()
    end[6, 9] = 127
    assert check_walk(ref, end, 3, 4, 9, 6) == (6, 6, None)               # the end cell is excluded
    both = end.copy()
    both[int(ys[2]), int(xs[2])] = 1
    both[int(ys[4]), int(xs[4])] = 1
    assert check_walk(ref, both, 3, 4, 9, 6)[0] == 2                      # the first of two


@pytest.mark.parametrize("start,end", [((13, 5), (22, 8)), ((2, 6), (-7, 3)), ((7, 1), (10, -8)), ((8, 10), (5, 19)),
                                       ((14, 10), (23, 19)), ((1, 1), (-8, -8)), ((14, 1), (23, -9)), ((1, 10), (-9, 14))],
                         ids=["right", "left", "top", "bottom", "corner-far", "corner-near", "corner-top-right", "corner-bottom-left"])
def test_a_walk_that_leaves_the_grid_finds_nothing_behind_the_border(ref, start, end):
    """16 x 12, free where the walk runs, occupied wherever an index that wrapped round the row or the grid would land: the whole
    rim but for the cells the walk itself crosses on its way out."""
    W, H = 16, 12
    cells = np.full((H, W), -20, np.int8)
    cells[0, :] = cells[H - 1, :] = 100
    cells[:, 0] = cells[:, W - 1] = 100
    xs, ys = walk(start[0], start[1], end[0], end[1])
    for x, y in zip(xs.tolist(), ys.tolist()):
        if 0 <= x < W and 0 <= y < H:
            cells[y, x] = -20
    first, K, cell = check_walk(ref, cells, start[0], start[1], end[0], end[1])
    assert (first, cell) == (K, None) and K >= 9
    inside = [(0 <= x < W and 0 <= y < H) for x, y in zip(xs.tolist(), ys.tolist())]
    assert inside[0] and not inside[-1] and inside == sorted(inside, reverse=True)          # it leaves, once, for good
    blocked = cells.copy()                                                # the same walk with its last cell inside occupied: found
    k_last = inside.index(False) - 1
    blocked[int(ys[k_last]), int(xs[k_last])] = 100
    assert check_walk(ref, blocked, start[0], start[1], end[0], end[1]) == (k_last, K, (int(xs[k_last]), int(ys[k_last])))


def test_first_hit_on_a_one_cell_grid(ref):
    for v, want in ((-20, (5, 5, None)), (100, (0, 5, (0, 0)))):
        cells = np.full((1, 1), v, np.int8)
        assert check_walk(ref, cells, 0, 0, 5, 3) == want
        assert check_walk(ref, cells, 0, 0, -3, -5) == want
        assert check_walk(ref, cells, 0, 0, 0, 0) == (0, 0, None)


# ---------------------------------------------------------------------------------------------------------------- quarter cells
def test_quarter(ref):
    pairs = [(0, 0), (1, 0), (3, 4), (4098, 4098)] + [(dx, dy) for dx in range(65) for dy in range(65) if dx * dx + dy * dy <= 4096]
    a = np.array([(7 + dx, -3 - dy, 7, -3) for dx, dy in pairs], np.int32)
    out = np.zeros(len(a), np.int32)
    ref.bd_quarter(len(a), _p(a), _p(out))
    d2 = np.array([dx * dx + dy * dy for dx, dy in pairs], np.int64)
    assert out[:4].tolist() == [0, 4, 20, math.isqrt(16 * 2 * 4098 * 4098)]
    assert out.tolist() == [math.isqrt(16 * int(v)) for v in d2]
    assert np.array_equal(out, bm.quarter(a[:, 0].astype(np.int64), a[:, 1].astype(np.int64), 7, -3))
    assert set(range(65)) <= {int(math.isqrt(int(v))) for v in d2} and 16 * int(d2.max()) < 2 ** 31 and (d2 == 4096).any()


# ---------------------------------------------------------------------------------------------------------------- p and lg
CPM = F32(20.0)
P = bm.params(max_range=60.0, hit_cut=64, lam=0.001, sigma_cells=8.0)     # a reach of 1200 cells: z >> 2 passes 1023
T = bm.make_tables(P, CPM)


def model_return_p(expect, z, zstar):
    """p of one return of z quarter cells by the model's look-up on a one-cell table holding zstar (or NONE)."""
    table = np.full((1, 1, 64), zstar if expect else rm.NONE, np.uint16)
    r = np.array([(z + 0.5) / (4.0 * float(CPM))], np.float32)
    rays = (r, np.zeros(1, np.float32), r >= F32(P["max_range"]))
    c = rm.lookup(table, (F32(0), F32(0)), CPM, rays, (0.025, 0.025, 0.0), P, T)
    assert c["z"].tolist() == [z] and c["zstar"].tolist() == [zstar if expect else -1]
    return int(c["p"][0])


def test_return_p(ref):
    tab = _tab(ref, T)
    cut = P["hit_cut"]
    cases = [(1, 300, 400), (1, 400, 400), (1, 500, 400),                  # z below, at and above z*
             (1, 400 - cut, 400), (1, 400 - cut - 1, 400), (1, 400 + cut, 400), (1, 400 + cut + 1, 400),
             (0, 300, -1), (0, 4091, -1), (0, 4092, -1), (0, 4095, -1), (0, 4096, -1), (0, 4700, -1),    # z >> 2 at 1022, 1023, 1024, beyond
             (1, 4095, 4600), (1, 4096, 4600), (1, 4400, 4600), (1, 12, 12), (1, 13, 12)]
    got = [ref.bd_return_p(_p(tab), int(T["rand"]), cut, e, z, zs) for e, z, zs in cases]
    assert got == [model_return_p(e, z, zs) for e, z, zs in cases]
    hit, short, rnd = T["hit"].astype(np.int64), T["short"].astype(np.int64), int(T["rand"])
    assert got[0] == rnd + hit[cut] + short[75] and got[1] == rnd + hit[0] and got[2] == rnd + hit[cut]
    assert got[3] - short[84] == got[4] - short[83] == got[5] == got[6] == rnd + hit[cut]            # the cut holds on both sides
    assert got[9] == got[10] == got[11] == got[12] == rnd + short[1023] != got[8]                   # the clamp at 1023
    assert hit[cut - 1] > hit[cut] and short[1022] > short[1023] > 0


def test_lg(ref):
    tab = _tab(ref, T)
    ps = [1, 2, 3, 2 ** 30, 2 ** 31 - 1,
          (1 << 30) + (1 << 22) - 1, (1 << 30) + (1 << 22),                # both sides of the first mantissa step at e = 30
          (1 << 20) + 77 * (1 << 12) - 1, (1 << 20) + 77 * (1 << 12),      # ... of step 77 at e = 20
          511, 512, 0x7f800000 - 1, 0x7f800000]
    got = [ref.bd_lg(_p(tab), p, int(T["ln2"])) for p in ps]
    assert got == bm.lg(np.array(ps, np.int64), T).tolist()
    assert got[0] == -30 * int(T["ln2"]) and got[3] == 0 and got[5] == 0 and got[6] == int(T["lt"][1]) and got[8] - got[7] > 0


# ---------------------------------------------------------------------------------------------------------------- heading index
@pytest.mark.parametrize("hn", [64, 1024])
def test_heading_index(ref, hn):
    kf = rm.heading_scale(hn)
    angles = [F32(0.0), F32(-0.0), PI_F, -PI_F, np.nextafter(PI_F, F32(0)), np.nextafter(-PI_F, F32(0))]
    straddled = 0
    for h in (0, 1, hn // 4, hn // 2 - 1, -1, -(hn // 4), -(hn // 2)):      # the half-way point above heading h, and the floats round it
        a = F32((h + 0.5) / float(kf))
        near = [a]
        for _ in range(3):
            near = [np.nextafter(near[0], F32(-10))] + near + [np.nextafter(near[-1], F32(10))]
        idx = rm.h_index(np.array(near, np.float32), hn)
        straddled += set(idx.tolist()) == {h & (hn - 1), (h + 1) & (hn - 1)}
        angles += near
    assert straddled == 7                                                 # every group holds floats on either side of its step
    a = np.array(angles, np.float32)
    out = np.zeros(len(a), np.int32)
    ref.bd_heading_index(len(a), _p(a), C.c_float(float(kf)), hn, _p(out))
    assert np.array_equal(out, rm.h_index(a, hn))
    assert out[:4].tolist() == [0, 0, hn // 2, hn // 2] and out.min() >= 0 and out.max() < hn


# ---------------------------------------------------------------------------------------------------------------- start cell
def test_start_cell(ref):
    W, H = 16, 12
    origin, cpm = (F32(-0.3), F32(0.7)), F32(20.0)
    off = lambda c: c + 0.5 if c >= 0 else c - 0.5                        # (a negative position truncates towards zero: cell -1 is (-2, -1])
    mid = lambda cx, cy: (float(origin[0]) + off(cx) / 20.0, float(origin[1]) + off(cy) / 20.0, 0.3)
    poses = [mid(0, 0), mid(W - 1, 0), mid(0, H - 1), mid(W - 1, H - 1), mid(7, 0), mid(7, H - 1), mid(0, 5), mid(W - 1, 5), mid(7, 5),
             mid(-1, 5), mid(W, 5), mid(7, -1), mid(7, H), mid(-1, -1), mid(W, H),              # one cell outside
             (float(origin[0]) - 0.01, 1.0, 0.0),                                               # (-1, 0) truncates to cell 0, as in the reference
             (float("nan"), 1.0, 0.0), (0.0, float("inf"), 0.0), (0.0, 1.0, float("-inf")), (0.0, 1.0, float("nan"))]
    assert [bm.pose_start(p, origin, cpm, W, H) is not None for p in poses] == [True] * 9 + [False] * 6 + [True] + [False] * 4
    _check_start(ref, poses, W, H, origin, cpm)
    # a grid position at +-2^30 (refused) and the float below it (converted, and outside): origin 0, one cell per metre
    edge, below = float(2 ** 30), float(np.nextafter(F32(2 ** 30), F32(0)))
    far = [(edge, 1.0, 0.0), (-edge, 1.0, 0.0), (1.0, edge, 0.0), (1.0, -edge, 0.0), (below, 1.0, 0.0), (-below, 1.0, 0.0), (1.0, below, 0.0),
           (1.0, -below, 0.0), (1.5, 1.5, 0.0)]
    out = _check_start(ref, far, 4, 4, (F32(0), F32(0)), F32(1.0))
    assert out[:, 0].tolist() == [0] * 8 + [1]
    assert out[:4, 1:].tolist() == [[0, 0]] * 4                           # at 2^30 nothing is converted
    assert out[4:8, 1:].tolist() == [[int(below), 1], [-int(below), 1], [1, int(below)], [1, -int(below)]]


def _check_start(ref, poses, W, H, origin, cpm):
    q = np.array(poses, np.float32).reshape(-1, 3)
    frame = np.array([origin[0], origin[1], F32(1.0) / cpm, cpm], np.float32)
    out, pos = np.zeros((len(q), 3), np.int32), np.zeros((len(q), 2), np.float32)
    ref.bd_start(len(q), _p(q), W, H, _p(frame), _p(out), _p(pos))
    for i, p in enumerate(q):
        s = bm.pose_start(p, origin, cpm, W, H)
        assert bool(out[i, 0]) == (s is not None), (i, p.tolist(), out[i].tolist())
        if s is not None:
            assert tuple(out[i, 1:].tolist()) == s
            px, py = bm.grid_position(p[0], p[1], origin, cpm)
            assert pos[i].tobytes() == np.array([px, py], np.float32).tobytes()
    return out
