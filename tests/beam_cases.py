"""Hand-built inputs of the beam model's tests (tests/test_beam_model_cpu.py, tests/test_gpu_beam*.py): small grids, scans and poses
that reach the rules of the definition one by one.  A case is a dict: cells (int8 [H][W]), origin, mpc, cpm, ranges, thetas (float32),
poses (float32 [n][3]) and params (beam_model.params(...))."""
import math

import numpy as np

import beam_model as bm

F32 = np.float32
MPC, CPM = 0.05, 20.0


def centre(cx, cy, theta=0.0, origin=(0.0, 0.0)):
    """The pose at the centre of cell (cx, cy)."""
    return (F32(origin[0] + (cx + 0.5) * MPC), F32(origin[1] + (cy + 0.5) * MPC), F32(theta))


def case(cells, ranges, thetas, poses, origin=(0.0, 0.0), **prm):
    return dict(cells=np.ascontiguousarray(cells, dtype=np.int8), origin=(F32(origin[0]), F32(origin[1])), mpc=MPC, cpm=CPM,
                ranges=np.asarray(ranges, dtype=np.float32), thetas=np.asarray(thetas, dtype=np.float32),
                poses=np.asarray(poses, dtype=np.float32).reshape(-1, 3), params=bm.params(**prm))


def room(w, h, fill=-20):
    """Free space inside a one-cell wall."""
    cells = np.full((h, w), fill, np.int8)
    cells[0, :] = cells[-1, :] = 100
    cells[:, 0] = cells[:, -1] = 100
    return cells


def two_walls():
    """96 x 48, one-cell walls at x = 40 and x = 60; a single fan of returns at 30 cells; pose A at x = 10 facing +x, B at x = 30.
    Every end cell of A lies in the first wall and of B in the second: an endpoint score cannot tell them apart."""
    cells = np.full((48, 96), -20, np.int8)
    cells[:, 40] = 100
    cells[:, 60] = 100
    phis = np.radians(np.arange(-8, 9, dtype=np.float64))
    return case(cells, np.full(len(phis), 30 * MPC, np.float32), -phis, [centre(10, 24), centre(30, 24)], max_range=3.0)


def octant_scan(n=32, r0=0.4, dr=0.13, extra=()):
    """n rays all round (exact diagonals and axes among them when n is a multiple of 8), ranges climbing, then `extra` (range, theta)."""
    th = [2.0 * math.pi * k / n for k in range(n)] + [e[1] for e in extra]
    rg = [r0 + dr * (k % 11) for k in range(n)] + [e[0] for e in extra]
    return np.array(rg, np.float32), np.array(th, np.float32)


def conditions(w, h, **prm):
    """A walled room with a pillar and a blob that is occupied where a pose stands: returns short of, at and behind the expected hit,
    rays with first == K, walks that leave the grid, max readings with and without an expected hit, the range limits and a NaN;
    poses in free space, on an occupied cell, next to the border, off the grid and with a NaN member."""
    cells = room(w, h)
    cells[h // 2 - 2:h // 2 + 1, w // 2 + 6:w // 2 + 8] = 90
    cells[5:7, 5:7] = 1                                     # occupied at occ_min = 1, not at 2
    cells[3, 3] = -128
    mr = prm.get("max_range", 1.5)
    extra = [(0.15, 0.1), (np.nextafter(F32(0.15), F32(1)), 0.2), (mr, 0.3), (np.nextafter(F32(mr), F32(0)), 0.3), (float("nan"), 0.4),
             (float("inf"), 0.5), (mr * 2, 3.0), (mr * 2, 0.0), (-1.0, 1.0), (0.0, 2.0)]
    rg, th = octant_scan(32, extra=extra)
    poses = [centre(w // 2, h // 2), centre(5, 5, 0.7), centre(1, 1, -2.0), centre(w - 2, h - 2, 3.1), centre(0, h // 2, 1.0),
             centre(-3, 4), centre(w + 2, 2), (F32("nan"), F32(0.5), F32(0)), (F32(0.5), F32(0.5), F32("inf")),
             centre(w // 2, h // 2), centre(w // 3, h // 3, 5.0)]
    return case(cells, rg, th, poses, **dict(dict(max_range=mr), **prm))


def open_field(w, h, reach, wall_x=None, **prm):
    """No border: a pose at the left edge looking along +x and along the diagonals with max_range = reach cells exactly, so that K is
    `reach`; with wall_x a wall column stands in the way, without it every walk ends with first == K or leaves the grid."""
    cells = np.full((h, w), -20, np.int8)
    if wall_x is not None:
        cells[:, wall_x] = 100
    th = np.array([0.0, math.pi / 4, -math.pi / 4, math.pi / 2, -math.pi / 2, math.pi, 0.05, -0.05], np.float32)
    rg = np.array([reach * MPC * f for f in (0.5, 0.9, 2.0, 0.25, 2.0, 0.5, 0.98, 0.3)], np.float32)
    poses = [centre(0, h // 2), centre(1, 1), centre(w - 1, h - 1, math.pi), centre(w // 2, 0, math.pi / 2)]
    return case(cells, rg, th, poses, **dict(dict(max_range=reach * MPC), **prm))


def ray_count(rays, stride=1, dropped_every=0, w=64, h=48):
    """`rays` non-dropped rays (one in dropped_every + 1 scan entries is a dropped one between them) all round a walled room."""
    cells = room(w, h)
    cells[10:14, 30:33] = 100
    rg, th = [], []
    for k in range(rays):
        if dropped_every and k % dropped_every == 0:
            rg.append(0.1)
            th.append(0.0)
        rg.append(0.3 + 0.01 * (k % 97))
        th.append(2.0 * math.pi * k / max(rays, 1))
    poses = [centre(20, 20, 0.3), centre(40, 30, -1.0), centre(31, 11)]
    return case(cells, rg, th, poses, max_range=1.2, ray_stride=stride)


def many_poses(n, w=64, h=48, seed=5):
    """n poses scattered over (and a few beyond) a walled room with pillars; 65 rays."""
    rng = np.random.default_rng(seed)
    cells = room(w, h)
    for _ in range(6):
        x, y = int(rng.integers(2, w - 4)), int(rng.integers(2, h - 4))
        cells[y:y + 2, x:x + 2] = 100
    rg, th = octant_scan(65, r0=0.3, dr=0.17)
    poses = np.stack([rng.uniform(-0.1, w * MPC + 0.1, n), rng.uniform(-0.1, h * MPC + 0.1, n), rng.uniform(-3.1, 3.1, n)], axis=1)
    return case(cells, rg, th, poses.astype(np.float32), max_range=2.0)


def mirror_case():
    """A room with an L-shaped wall and poses at cell centres with headings that are multiples of pi / 2: the cases on which the
    symmetries of the test are asked (after the end cells have been found mirror-exact).  The reach is 7 cells and no pose stands
    closer than 8 to the border: a far cell with a negative coordinate is truncated towards zero, which no mirror image shares."""
    cells = room(41, 41)
    cells[10:30, 25] = 100
    cells[16, 8:20] = 100
    th = np.array([0.0, math.pi / 2, math.pi, -math.pi / 2], np.float32)
    rg = np.array([0.2, 0.3, 0.1, 1.9], np.float32)
    poses = [centre(20, 20), centre(12, 14), centre(30, 9)]
    return case(cells, rg, th, poses, max_range=0.35)
