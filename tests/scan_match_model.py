"""The model of the correlative scan matcher: a numpy restatement of the definition in include/botlab_hip.h
("correlative scan matching"), which the HIP kernels of botlab_amd/csrc/bl_scanmatch.hip must reproduce bit for bit.

Float arithmetic is numpy float32 / float64 operation by operation (no fused operations); sinf / cosf come from the C library
through ctypes -- glibc's, which bl_math.h reproduces bit for bit -- not from numpy.  Every score is an exact integer.
"""
import ctypes
import ctypes.util
import math

import numpy as np

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.sinf.restype = ctypes.c_float
_libm.sinf.argtypes = [ctypes.c_float]
_libm.cosf.restype = ctypes.c_float
_libm.cosf.argtypes = [ctypes.c_float]

MIN_RANGE = np.float32(0.15)          # moving_laser_scan.cpp:24
MAX_N, MAX_NTHETA, MAX_RAYS = 64, 180, 4096
F32 = np.float32
PI_F = np.float32(3.14159274101257324)


def wrap_to_pi(a):
    """angle_functions.hpp:12-24: a float angle compared against double pi, stepped by a double 2 pi, narrowed on every step."""
    a = F32(a)
    if not math.isfinite(float(a)):
        return a
    while float(a) < -math.pi:
        a = F32(float(a) + 2.0 * math.pi)
    while float(a) > math.pi:
        a = F32(float(a) - 2.0 * math.pi)
    return a


def valid_rays(ranges, thetas, max_range):
    ranges = np.asarray(ranges, dtype=np.float32)
    thetas = np.asarray(thetas, dtype=np.float32)
    keep = (ranges > MIN_RANGE) & (ranges < F32(max_range))
    return ranges[keep], thetas[keep]


def grid_position(cx, cy, origin, cpm):
    """global_position_to_grid_position (grid_utils.hpp:49-55) narrowed to Point<float>."""
    sx = F32((float(F32(cx)) - float(F32(origin[0]))) * float(F32(cpm)))
    sy = F32((float(F32(cy)) - float(F32(origin[1]))) * float(F32(cpm)))
    return sx, sy


def endpoints(ranges, thetas, centre, dk, dtheta, origin, cpm):
    """(ex, ey, has_cell) of the valid rays at heading step dk: scoreRay's float arithmetic and truncating conversion."""
    cpm = F32(cpm)
    theta_k = F32(F32(centre[2]) + F32(F32(dk) * F32(dtheta)))
    sx, sy = grid_position(centre[0], centre[1], origin, cpm)
    n = len(ranges)
    cs = np.empty(n, dtype=np.float32)
    sn = np.empty(n, dtype=np.float32)
    for r in range(n):
        a = wrap_to_pi(F32(theta_k - thetas[r]))
        cs[r] = _libm.cosf(float(a))
        sn[r] = _libm.sinf(float(a))
    with np.errstate(all="ignore"):
        fx = (ranges * cs) * cpm + sx
        fy = (ranges * sn) * cpm + sy
        has = (np.abs(fx) < F32(2.0 ** 30)) & (np.abs(fy) < F32(2.0 ** 30))
    ex = np.zeros(n, dtype=np.int64)
    ey = np.zeros(n, dtype=np.int64)
    ex[has] = np.trunc(fx[has]).astype(np.int64)
    ey[has] = np.trunc(fy[has]).astype(np.int64)
    return ex, ey, has


def score_volume(cells, origin, cpm, ranges, thetas, centre, nx, ny, ntheta, dtheta):
    """int32 [2 ntheta + 1][2 ny + 1][2 nx + 1] of the valid rays (ranges, thetas already filtered)."""
    cells = np.asarray(cells)
    H, W = cells.shape
    P = np.zeros((H + 4 * ny + 2, W + 4 * nx + 2), dtype=np.int32)           # positive part, zero frame of 2 n + 1
    px, py = 2 * nx + 1, 2 * ny + 1
    P[py:py + H, px:px + W] = np.maximum(cells.astype(np.int32), 0)
    cw, ch = 2 * nx + 1, 2 * ny + 1
    vol = np.zeros((2 * ntheta + 1, ch, cw), dtype=np.int64)
    small = cw * ch <= 1024
    view = np.lib.stride_tricks.sliding_window_view(P, (ch, cw)) if small else None
    for k in range(2 * ntheta + 1):
        ex, ey, has = endpoints(ranges, thetas, centre, k - ntheta, dtheta, origin, cpm)
        on = has & (ex >= -nx) & (ex < W + nx) & (ey >= -ny) & (ey < H + ny)  # the others meet the grid under no shift
        ex, ey = ex[on], ey[on]
        if small:
            vol[k] = view[ey + py - ny, ex + px - nx].sum(axis=0, dtype=np.int64)
        else:
            acc = vol[k]
            for x, y in zip(ex.tolist(), ey.tolist()):
                acc += P[y + py - ny:y + py + ny + 1, x + px - nx:x + px + nx + 1]
    assert vol.max(initial=0) < 2 ** 31
    return vol.astype(np.int32)


def best_candidate(vol, nx, ny, ntheta):
    """Highest score; ties: smallest di*di + dj*dj, then smallest |dk|, then smallest dk, dj, di.  Returns (di, dj, dk, score, ties)."""
    top = int(vol.max())
    ks, js, is_ = np.nonzero(vol == top)
    cands = [((i - nx) ** 2 + (j - ny) ** 2, abs(k - ntheta), k - ntheta, j - ny, i - nx) for k, j, i in zip(ks.tolist(), js.tolist(), is_.tolist())]
    _, _, dk, dj, di = min(cands)
    return di, dj, dk, top, len(cands)


def check_params(nx, ny, ntheta, dtheta):
    return 0 <= nx <= MAX_N and 0 <= ny <= MAX_N and 0 <= ntheta <= MAX_NTHETA and F32(dtheta) > 0


def match(cells, origin, mpc, cpm, scan_ranges, scan_thetas, centre, nx, ny, ntheta, dtheta, max_range, min_score=0, utime=0):
    """The whole definition.  centre = (x, y, theta).  Returns a dict with the fields of bl_scan_match_result_t (pose as float32
    x, y, theta) and "volume"."""
    assert check_params(nx, ny, ntheta, dtheta)
    dtheta = F32(dtheta)
    centre = (F32(centre[0]), F32(centre[1]), F32(centre[2]))
    ranges, thetas = valid_rays(scan_ranges, scan_thetas, max_range)
    assert len(ranges) <= MAX_RAYS
    vol = score_volume(cells, origin, cpm, ranges, thetas, centre, nx, ny, ntheta, dtheta)
    di, dj, dk, top, ties = best_candidate(vol, nx, ny, ntheta)
    accepted = int(top >= min_score)
    if accepted:
        x = F32(float(centre[0]) + di * float(F32(mpc)))
        y = F32(float(centre[1]) + dj * float(F32(mpc)))
        theta = wrap_to_pi(F32(centre[2] + F32(F32(dk) * dtheta)))
    else:
        x, y, theta = centre
    return dict(x=F32(x), y=F32(y), theta=F32(theta), utime=int(utime), di=di, dj=dj, dk=dk, score=top,
                score_centre=int(vol[ntheta, ny, nx]), ties=ties, rays_used=int(len(ranges)), accepted=accepted, volume=vol)


def brute_force_volume(cells, origin, cpm, scan_ranges, scan_thetas, centre, nx, ny, ntheta, dtheta, max_range):
    """The definition as a plain triple loop over candidates and a loop over rays (small windows only)."""
    cells = np.asarray(cells)
    H, W = cells.shape
    ranges, thetas = valid_rays(scan_ranges, scan_thetas, max_range)
    centre = (F32(centre[0]), F32(centre[1]), F32(centre[2]))
    vol = np.zeros((2 * ntheta + 1, 2 * ny + 1, 2 * nx + 1), dtype=np.int32)
    for dk in range(-ntheta, ntheta + 1):
        ex, ey, has = endpoints(ranges, thetas, centre, dk, F32(dtheta), origin, cpm)
        for dj in range(-ny, ny + 1):
            for di in range(-nx, nx + 1):
                s = 0
                for r in range(len(ranges)):
                    if not has[r]:
                        continue
                    x, y = int(ex[r]) + di, int(ey[r]) + dj
                    if 0 <= x < W and 0 <= y < H and cells[y, x] > 0:
                        s += int(cells[y, x])
                vol[dk + ntheta, dj + ny, di + nx] = s
    return vol


def compose_delta(last, odo_prev, odo_now):
    """The driver's centre: `last` (x, y, theta as float32) composed with the odometry delta odo_prev -> odo_now, the delta
    expressed in the odometry frame of odo_prev and replayed from `last` (float32 inputs, double arithmetic, narrowed once)."""
    dx = float(F32(odo_now[0])) - float(F32(odo_prev[0]))
    dy = float(F32(odo_now[1])) - float(F32(odo_prev[1]))
    dth = float(F32(odo_now[2])) - float(F32(odo_prev[2]))
    rot = float(F32(last[2])) - float(F32(odo_prev[2]))
    c, s = math.cos(rot), math.sin(rot)
    x = F32(float(F32(last[0])) + (c * dx - s * dy))
    y = F32(float(F32(last[1])) + (s * dx + c * dy))
    th = wrap_to_pi(F32(float(F32(last[2])) + dth))
    return x, y, th
