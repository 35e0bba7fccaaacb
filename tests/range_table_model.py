"""The model of the range table: a numpy restatement of the definition in include/botlab_hip.h ("range table"), which k_rt_build
(botlab_amd/csrc/bl_rangetable.hip) and k_beam_lookup (bl_beam.hip) must reproduce value for value: every entry of the table after a
build and after an update, and h, z, z*, p of every used ray, the score of every pose and the units of the scoring by table.

Behind the directions -- made on the host in double, directions(), compared on their own against bl_rangetable_directions -- everything
is an exact integer; build(), update() and lookup() take whichever directions and tables they are given.  The used rays, the start
cell, the tables, lg and the units are the beam model's (tests/beam_model.py, imported, not restated).
"""
import math

import numpy as np

import beam_model as bm
from beam_model import ArgError, OFF_GRID
from obstacle_layer_model import walk
from scan_match_model import wrap_to_pi

F32 = np.float32
NONE = 0xFFFF
MIN_HEADINGS, MAX_HEADINGS = 64, 1024
MAX_ENTRIES = 2 ** 31


class StateError(Exception):
    """What the library answers with BL_ERR_STATE."""


def headings_ok(hn):
    return MIN_HEADINGS <= hn <= MAX_HEADINGS and hn & (hn - 1) == 0


def directions(reach, hn):
    """int64 [hn][2]: D[h] = (lround(reach cos(2 pi h / hn)), lround(reach sin(2 pi h / hn))) in double."""
    if not headings_ok(hn):
        raise ArgError("headings")
    return np.array([(bm._lround(reach * math.cos(2.0 * math.pi * h / hn)), bm._lround(reach * math.sin(2.0 * math.pi * h / hn)))
                     for h in range(hn)], np.int64).reshape(hn, 2)


def _fill(table, cells, D, occ_min, x0, y0, x1, y1):
    """The entries of the cells x0 .. x1, y0 .. y1 (inclusive, inside the grid) computed from `cells`, heading by heading: cell k of the
    walk lies at the same offset from every start cell, so step k looks the whole box up in a shifted copy of the grid."""
    H, W = cells.shape
    occ = np.asarray(cells) >= occ_min
    bw, bh = x1 - x0 + 1, y1 - y0 + 1
    ys, xs = np.mgrid[y0:y1 + 1, x0:x1 + 1]
    for h in range(len(D)):
        dx, dy = int(D[h][0]), int(D[h][1])
        wx, wy = walk(0, 0, dx, dy)                                         # offsets of cells k = 0 .. K - 1
        val = np.full((bh, bw), NONE, np.int64)
        open_ = np.ones((bh, bw), bool)
        for k in range(min(len(wx), max(W, H))):                            # beyond that every walk has left the grid
            cx, cy = xs + int(wx[k]), ys + int(wy[k])
            inside = (cx >= 0) & (cx < W) & (cy >= 0) & (cy < H)
            hit = open_ & inside
            hit[hit] = occ[cy[hit], cx[hit]]
            val[hit] = int(bm.quarter(int(wx[k]), int(wy[k]), 0, 0))
            open_ &= ~hit
            if not open_.any():
                break
        table[y0:y1 + 1, x0:x1 + 1, h] = val
    return table


def check_entries(W, H, hn):
    if W * H * hn > MAX_ENTRIES:
        raise ArgError("entries")


def build(cells, D, occ_min):
    """uint16 [H][W][Hn]: T of the whole grid."""
    cells = np.asarray(cells)
    H, W = cells.shape
    check_entries(W, H, len(D))
    return _fill(np.zeros((H, W, len(D)), np.uint16), cells, D, occ_min, 0, 0, W - 1, H - 1)


def widened(box, reach, W, H):
    """The box x0, y0, x1, y1 (inclusive) widened by reach and clipped to the grid, or None for one that is empty or lies outside."""
    x0, y0, x1, y1 = box
    if x1 < x0 or y1 < y0 or x1 < 0 or y1 < 0 or x0 >= W or y0 >= H:
        return None
    return max(x0 - reach, 0), max(y0 - reach, 0), min(x1 + reach, W - 1), min(y1 + reach, H - 1)


def update(table, cells, D, occ_min, reach, box):
    """bl_rangetable_update: `table` (changed in place and returned) after the cells of `box` changed to what `cells` now holds."""
    cells = np.asarray(cells)
    H, W = cells.shape
    if table.shape[:2] != (H, W):
        raise ArgError("shape")
    b = widened(box, reach, W, H)
    return table if b is None else _fill(table, cells, D, occ_min, *b)


def heading_scale(hn):
    return F32(hn / (2.0 * math.pi))


def h_index(a, hn):
    """h of float32 angles a: (int)floorf(a * kf + 0.5f) & (hn - 1), one multiply and one add, each rounded to float."""
    a = np.asarray(a, dtype=np.float32)
    v = (a * heading_scale(hn)).astype(np.float32) + F32(0.5)
    return np.floor(v.astype(np.float32)).astype(np.int64) & (hn - 1)


def ray_angles(thetas, pose_theta):
    """a = wrap_to_pi(theta - theta_r) in float32, the angle scan_match_model.endpoints forms at heading step 0."""
    theta_k = F32(F32(pose_theta) + F32(F32(0) * F32(0)))
    return np.array([wrap_to_pi(F32(theta_k - t)) for t in np.asarray(thetas, dtype=np.float32)], np.float32).reshape(-1)


def lookup(table, origin, cpm, rays, pose, p, t):
    """Per used ray of one pose: h, z, zstar, p (int64 each; -1, -1, -1, 0 for a ray whose angle is not finite; z = -1 for a max
    reading, zstar = -1 without an expected hit), or None for a pose that takes no part.  rays = beam_model.used_rays(...)."""
    H, W, hn = table.shape
    s = bm.pose_start(pose, origin, cpm, W, H)
    if s is None:
        return None
    r, th, is_max = rays
    a = ray_angles(th, pose[2])
    ok = np.isfinite(a)
    h = h_index(np.where(ok, a, F32(0)), hn)
    tz = table[s[1], s[0]].astype(np.int64)[h]
    expect = tz != NONE
    zstar = np.where(expect, tz, -1)
    q = F32(F32(4.0) * F32(cpm))
    with np.errstate(all="ignore"):
        z = np.where(is_max, -1, np.trunc(np.where(is_max, F32(0), r * q).astype(np.float32)).astype(np.int64))
    hit = t["hit"].astype(np.int64)[np.minimum(np.abs(z - zstar), p["hit_cut"])]
    short = t["short"].astype(np.int64)[np.minimum(np.maximum(z, 0) >> 2, 1023)]
    p_ret = np.where(expect, hit, 0) + np.where(~expect | (z < zstar), short, 0) + int(t["rand"])
    pv = np.where(is_max, np.where(expect, int(t["max_blocked"]), int(t["max_free"])), p_ret)
    out = dict(h=h, z=z, zstar=zstar, p=pv)
    for name, dropped in (("h", -1), ("z", -1), ("zstar", -1), ("p", 0)):
        out[name] = np.where(ok, out[name], dropped).astype(np.int64)
    return out


def scores(table, origin, cpm, ranges, thetas, poses, p, t):
    """int64 [n]: S of every pose by table (OFF_GRID for the poses that take no part)."""
    rays = bm.used_rays(ranges, thetas, p)
    out = np.empty(len(poses), np.int64)
    for i, pose in enumerate(poses):
        c = lookup(table, origin, cpm, rays, pose, p, t)
        out[i] = OFF_GRID if c is None else int(bm.lg(c["p"][c["p"] > 0], t).sum())
    return out


def check_state(built, table_occ_min, table_reach, table_cpm, p):
    """The three refusals of the scoring by table."""
    if not built:
        raise StateError("not built")
    if p["occ_min"] != table_occ_min:
        raise StateError("occ_min")
    if bm.reach_cells(p, table_cpm) != table_reach:
        raise StateError("reach")
