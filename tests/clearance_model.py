"""The model of the clearance grid and of the leap walk: a numpy restatement of the definition in include/botlab_hip.h ("clearance
grid"), which botlab_amd/csrc/bl_clearance.hip and k_beam_leap (bl_beam.hip) must reproduce value for value.  Everything else of the
beam model -- rays, geometry, lengths, p, lg, scores, units -- is tests/beam_model.py's, and beam_model.cast is the yardstick for
first, K, z, zstar and p of the leap form too; this file adds the grid, the walk in leaps and its rounds.
"""
import numpy as np

import beam_model as bm
from scan_match_model import endpoints


class StateError(Exception):
    """What the library answers with BL_ERR_STATE."""


def _line(occ, cap):
    """Along the last axis: min(cap, distance to the nearest True), cap where there is none."""
    n = occ.shape[-1]
    idx = np.arange(n, dtype=np.int64)
    big = np.int64(4 * (n + cap + 1))
    last = np.maximum.accumulate(np.where(occ, idx, -big), axis=-1)          # the nearest True at or before
    nxt = np.minimum.accumulate(np.where(occ, idx, big)[..., ::-1], axis=-1)[..., ::-1]   # at or after
    return np.minimum(np.minimum(idx - last, nxt - idx), cap)


def grid(cells, occ_min, cap):
    """uint8 [H][W]: D of the definition, separably: the distance along the row to the row's nearest occupied cell, then
    D = min over dy of max(|dy|, row[y + dy]), each capped."""
    cells = np.asarray(cells)
    assert 1 <= cap <= 255 and 1 <= occ_min <= 127
    h, w = cells.shape
    rows = _line(cells >= occ_min, cap)                                       # [H][W]
    out = rows.copy()
    for dy in range(1, min(cap, h)):                                          # |dy| >= cap adds nothing below the cap
        up = np.full((h, w), cap, np.int64)
        up[dy:] = rows[:-dy]
        dn = np.full((h, w), cap, np.int64)
        dn[:-dy] = rows[dy:]
        out = np.minimum(out, np.maximum(dy, np.minimum(up, dn)))
    return out.astype(np.uint8)


def brute(cells, occ_min, cap):
    """The definition word for word: the minimum over all occupied cells."""
    cells = np.asarray(cells)
    h, w = cells.shape
    oy, ox = np.nonzero(cells >= occ_min)
    out = np.full((h, w), cap, np.int64)
    for y in range(h):
        for x in range(w):
            if len(ox):
                out[y, x] = min(cap, int(np.maximum(np.abs(ox - x), np.abs(oy - y)).min()))
    return out.astype(np.uint8)


def widened(box, cap, w, h):
    """The cells bl_clearance_update computes again for the inclusive box (x0, y0, x1, y1), or None when it changes nothing."""
    x0, y0, x1, y1 = box
    if x1 < x0 or y1 < y0 or x1 < 0 or y1 < 0 or x0 >= w or y0 >= h:
        return None
    return max(x0 - cap, 0), max(y0 - cap, 0), min(x1 + cap, w - 1), min(y1 + cap, h - 1)


def loop_walks(cells, occ_min, sx, sy, tx, ty):
    """For arrays of walks: first, K, the hit cell (x, y; -1 without one) and the cells read, by the plain Bresenham loop of the
    reference (mapping.cpp:101-127), one cell a step with the error term carried along, ended where it leaves the grid."""
    cells = np.asarray(cells)
    h, w = cells.shape
    sx, sy, tx, ty = (np.atleast_1d(np.asarray(v, dtype=np.int64)) for v in (sx, sy, tx, ty))
    dx, dy = np.abs(tx - sx), np.abs(ty - sy)
    stx, sty = np.where(sx < tx, 1, -1), np.where(sy < ty, 1, -1)
    K = np.maximum(dx, dy)
    err, x, y = dx - dy, sx.copy(), sy.copy()
    first, hx, hy, reads = K.copy(), np.full(len(K), -1, np.int64), np.full(len(K), -1, np.int64), np.zeros(len(K), np.int64)
    live = np.ones(len(K), bool)
    for k in range(int(K.max(initial=0))):
        live &= k < K
        inside = (x >= 0) & (x < w) & (y >= 0) & (y < h)
        live &= inside                                                        # a walk that left is over: first stays K
        reads[live] += 1
        occ = np.zeros(len(K), bool)
        occ[live] = cells[y[live], x[live]] >= occ_min
        first[occ], hx[occ], hy[occ] = k, x[occ], y[occ]
        live &= ~occ
        e2 = 2 * err
        mx, my = e2 >= -dy, e2 <= dx
        err = err - np.where(mx, dy, 0) + np.where(my, dx, 0)
        x, y = x + np.where(mx, stx, 0), y + np.where(my, sty, 0)
    return first, K, hx, hy, reads


def leap_walks(D, sx, sy, tx, ty):
    """For arrays of walks: first, K, the hit cell (x, y; -1 without one) and the rounds of the walk in leaps over the clearance grid
    D, each cell placed by the walk's closed form."""
    D = np.asarray(D)
    h, w = D.shape
    sx, sy, tx, ty = (np.atleast_1d(np.asarray(v, dtype=np.int64)) for v in (sx, sy, tx, ty))
    dx, dy = np.abs(tx - sx), np.abs(ty - sy)
    stx, sty = np.where(sx < tx, 1, -1), np.where(sy < ty, 1, -1)
    K = np.maximum(dx, dy)
    xmaj, dmaj, dmin = dx >= dy, np.maximum(K, 1), np.minimum(dx, dy)
    k = np.zeros(len(K), np.int64)
    first, hx, hy, rounds = K.copy(), np.full(len(K), -1, np.int64), np.full(len(K), -1, np.int64), np.zeros(len(K), np.int64)
    live = k < K
    while live.any():
        minor = (2 * k * dmin + dmaj) // (2 * dmaj)
        x = sx + stx * np.where(xmaj, k, minor)
        y = sy + sty * np.where(xmaj, minor, k)
        live &= (x >= 0) & (x < w) & (y >= 0) & (y < h)                       # a walk that left is over: first stays K
        rounds[live] += 1
        d = np.zeros(len(K), np.int64)
        d[live] = D[y[live], x[live]]
        hit = live & (d == 0)
        first[hit], hx[hit], hy[hit] = k[hit], x[hit], y[hit]
        live &= ~hit
        k = k + d
        live &= k < K
    return first, K, hx, hy, rounds


def loop_walk(cells, occ_min, sx, sy, tx, ty):
    """One walk: first, K, the hit cell (None without one), the cells read."""
    f, K, hx, hy, n = loop_walks(cells, occ_min, [sx], [sy], [tx], [ty])
    return int(f[0]), int(K[0]), ((int(hx[0]), int(hy[0])) if f[0] < K[0] else None), int(n[0])


def leap_walk(D, sx, sy, tx, ty):
    """One walk: first, K, the hit cell (None without one), the rounds."""
    f, K, hx, hy, n = leap_walks(D, [sx], [sy], [tx], [ty])
    return int(f[0]), int(K[0]), ((int(hx[0]), int(hy[0])) if f[0] < K[0] else None), int(n[0])


def far_cells(origin, cpm, rays, pose, p):
    """(mx, my, ok) per used ray of one pose: the far cell and whether `has` keeps the ray, as beam_model.cast forms them."""
    r, th, is_max = rays
    pose = tuple(np.float32(v) for v in pose)
    _, _, has_e = endpoints(r, th, pose, 0, np.float32(0), origin, cpm)
    mx, my, has_m = endpoints(np.full(len(r), np.float32(p["max_range"]), np.float32), th, pose, 0, np.float32(0), origin, cpm)
    return mx, my, has_m & (has_e | is_max)


def cast(cells, D, origin, cpm, rays, pose, p, t):
    """beam_model.cast's columns plus `rounds` (-1 for a dropped ray), or None for an off-grid pose.  first and K are asserted to be
    the cast's own: the leap walk may not change them."""
    c = bm.cast(cells, origin, cpm, rays, pose, p, t)
    if c is None:
        return None
    h, w = np.asarray(cells).shape
    s = bm.pose_start(pose, origin, cpm, w, h)
    mx, my, ok = far_cells(origin, cpm, rays, pose, p)
    rounds = np.full(len(rays[0]), -1, np.int64)
    i = np.flatnonzero(ok)
    first, K, _, _, rounds[i] = leap_walks(D, np.full(len(i), s[0]), np.full(len(i), s[1]), mx[i], my[i])
    assert np.array_equal(first, c["first"][i]) and np.array_equal(K, c["K"][i])
    return dict(c, rounds=rounds)


def check_state(built, built_occ_min, p):
    """bl_clearance_scores' state rule."""
    if not built or built_occ_min != p["occ_min"]:
        raise StateError()
