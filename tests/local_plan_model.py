"""The model of the local planner (include/botlab_hip.h, "local planner"), restated in Python: the definition the HIP kernels of
botlab_amd/csrc/bl_localplan.hip are checked against, byte for byte.  Built over tests/nav_field_model.py's field, tables and
path-step rule.  Float arithmetic is numpy float32 / Python double operation by operation (nothing fused); sinf / cosf come from the
C library through ctypes, as in tests/scan_match_model.py.  Costs are exact Python integers.
"""
import ctypes
import ctypes.util
import math

import numpy as np

import nav_field_model as nm
from scan_match_model import wrap_to_pi

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.sinf.restype = ctypes.c_float
_libm.sinf.argtypes = [ctypes.c_float]
_libm.cosf.restype = ctypes.c_float
_libm.cosf.argtypes = [ctypes.c_float]

F32 = np.float32
REACHED, OFF_FIELD, BLOCKED = 1, 2, 4
COST_NONE = 2 ** 63 - 1
MAX_NV, MAX_NW, MAX_STEPS, MAX_WEIGHT = 64, 1025, 255, 65535
MAX_THETA = F32(65536.0)                                     # BL_LOCALPLAN_MAX_THETA: 10 432 wrap steps, below bl_wrap_to_pi's cut at 2^16
WINDOW_BYTES = 48 * 1024
# the angle of each move of nm.MOVES, a double narrowed to float
MOVE_ANGLE = [F32(a) for a in (0.0, math.pi, math.pi / 2, -math.pi / 2, math.pi / 4, 3 * math.pi / 4, -math.pi / 4, -3 * math.pi / 4)]
K_HEADING = F32(1024.0 / math.pi)
RESULT = np.dtype([("trans_v", "<f4"), ("angular_v", "<f4"), ("index", "<i4"), ("n_admissible", "<i4"), ("cost", "<i8"), ("flags", "<i4"),
                   ("pad", "<i4")])
assert RESULT.itemsize == 32


class Params:
    def __init__(self, v_min=0.0, v_max=0.5, w_max=2.0, acc_v=1.0, acc_w=6.0, dt_control=0.1, dt_sim=0.05, n_v=8, n_w=33, n_steps=30,
                 w_field=1, w_heading=0, w_clear=0, w_speed=0):
        self.v_min, self.v_max, self.w_max = F32(v_min), F32(v_max), F32(w_max)
        self.acc_v, self.acc_w = F32(acc_v), F32(acc_w)
        self.dt_control, self.dt_sim = F32(dt_control), F32(dt_sim)
        self.n_v, self.n_w, self.n_steps = int(n_v), int(n_w), int(n_steps)
        self.w_field, self.w_heading, self.w_clear, self.w_speed = int(w_field), int(w_heading), int(w_clear), int(w_speed)

    def floats(self):
        return [self.v_min, self.v_max, self.w_max, self.acc_v, self.acc_w, self.dt_control, self.dt_sim]

    def ok(self):
        """bl_localplan_set_params' rule."""
        if not all(math.isfinite(float(f)) for f in self.floats()):
            return False
        if self.v_min > self.v_max or self.w_max < 0 or not self.dt_control > 0 or not self.dt_sim > 0:
            return False
        if not (1 <= self.n_v <= MAX_NV and 1 <= self.n_w <= MAX_NW and 1 <= self.n_steps <= MAX_STEPS):
            return False
        return all(0 <= w <= MAX_WEIGHT for w in (self.w_field, self.w_heading, self.w_clear, self.w_speed))

    def v_abs(self):
        return max(abs(float(self.v_min)), abs(float(self.v_max)))

    def can_skip_a_cell(self, mpc):
        return self.v_abs() * float(self.dt_sim) > float(F32(mpc))

    def staged(self, cpm):
        """The header's rule: True when the window of the rollouts' reach is staged in LDS."""
        r = int(math.ceil(self.v_abs() * float(self.dt_sim) * self.n_steps * float(F32(cpm)))) + 2
        return (2 * r + 1) * (2 * r + 1) * 2 <= WINDOW_BYTES


def _table(cur, lim_lo, lim_hi, acc, dt, n):
    cur, lim_lo, lim_hi, acc, dt = float(cur), float(lim_lo), float(lim_hi), float(acc), float(dt)
    lo, hi = max(lim_lo, cur - acc * dt), min(lim_hi, cur + acc * dt)
    if lo > hi:
        lo = hi = min(max(cur, lim_lo), lim_hi)
    if n == 1:
        return np.array([hi], dtype=np.float32)
    return np.array([lo + (hi - lo) * i / (n - 1) for i in range(n)], dtype=np.float32)


def tables(p, v, w):
    """(v_i, w_j) of a state with velocities v, w (float32)."""
    return (_table(F32(v), p.v_min, p.v_max, p.acc_v, p.dt_control, p.n_v),
            _table(F32(w), -float(p.w_max), p.w_max, p.acc_w, p.dt_control, p.n_w))


class World:
    """What a computed field hands the planner: the field, per-cell traversability and penalty, the allowed moves, the frame."""

    def __init__(self, field, l1, trav, pen, origin, mpc, cpm):
        self.field = field
        self.tcell, self.pcell = nm.cell_tables(l1, trav, pen)
        self.allowed = nm.allowed_moves(self.tcell)
        self.origin, self.mpc, self.cpm = origin, F32(mpc), F32(cpm)
        self.h, self.w = field.shape

    def cell(self, x, y):
        return nm.pose_cell((x, y), self.origin, self.cpm, self.w, self.h)

    def descent_move(self, x, y):
        """nm.descend_cells' choice from (x, y): the move index, or -1."""
        best, bm = None, -1
        for m, (dx, dy) in enumerate(nm.MOVES):
            if not self.allowed[m][y, x]:
                continue
            v = int(self.field[y + dy, x + dx])
            if v == nm.UNREACHED:
                continue
            if best is None or v + nm.STEP[m] < best:
                best, bm = v + nm.STEP[m], m
        return bm

    def start_flags(self, x, y):
        c = self.cell(x, y)
        if c is None or not self.tcell[c[1], c[0]] or int(self.field[c[1], c[0]]) == nm.UNREACHED:
            return OFF_FIELD
        return REACHED if int(self.field[c[1], c[0]]) == 0 else 0


def state_ok(pose, v, w):
    """lp_state_ok's rule: every member finite, and |theta| <= MAX_THETA (in float)."""
    if not all(math.isfinite(float(F32(f))) for f in (pose[0], pose[1], pose[2], v, w)):
        return False
    return not abs(F32(pose[2])) > MAX_THETA


def headings(theta, w_j, dt_sim, n_steps):
    """theta_0 .. theta_n: the heading each step integrates with, and the one the rollout ends on."""
    th = wrap_to_pi(F32(theta))
    dth = F32(F32(w_j) * F32(dt_sim))
    out = [th]
    for _ in range(n_steps):
        th = wrap_to_pi(F32(th + dth))
        out.append(th)
    return out


def trig(ths):
    return [(F32(_libm.cosf(float(t))), F32(_libm.sinf(float(t)))) for t in ths]


def rollout(pose, v_i, w_j, p):
    """The n_steps poses (x, y, theta) of a candidate."""
    ths = headings(pose[2], w_j, p.dt_sim, p.n_steps)
    cs_sn = trig(ths[:-1])
    s = F32(F32(v_i) * p.dt_sim)
    x, y = F32(pose[0]), F32(pose[1])
    out = []
    for k in range(p.n_steps):
        x = F32(x + F32(s * cs_sn[k][0]))
        y = F32(y + F32(s * cs_sn[k][1]))
        out.append((x, y, ths[k + 1]))
    return out


def heading_term(world, e, theta_end):
    if int(world.field[e[1], e[0]]) == 0:
        return 0
    bm = world.descent_move(e[0], e[1])
    if bm < 0:
        return 1024
    l, r = float(F32(theta_end)), float(MOVE_ANGLE[bm])
    diff = l - r                                             # angle_diff (angle_functions.hpp:78-87), in double
    if abs(diff) > math.pi:
        diff -= math.pi * 2 if diff > 0 else math.pi * -2
    return int(math.floor(float(F32(abs(F32(diff)) * K_HEADING))))


def costs(world, p, pose, v, w, stats=None):
    """int64 [n_w * n_v] costs of a state's candidates, COST_NONE for an inadmissible one (whatever the state's flags would be).
    stats, a dict, counts what the rollouts met: 'left' / 'right' / 'bottom' / 'top' exits of the grid, 'blocked' cells, 'unreached'
    ends, 'wrapped' candidates whose heading stepped through +-pi, 'strip' steps on the grid at x < origin x or y < origin y (the
    (-1, 0) strip that the truncating cast gives to cell 0), 'strip_candidates' admissible candidates with such a step, and under
    'terms' {c: (field(e), h, sum of penalties)} of every admissible candidate."""
    assert state_ok(pose, v, w)
    vt, wt = tables(p, v, w)
    out = np.full(p.n_w * p.n_v, COST_NONE, dtype=np.int64)
    ox, oy, cpm = float(F32(world.origin[0])), float(F32(world.origin[1])), float(world.cpm)
    for j in range(p.n_w):
        ths = headings(pose[2], wt[j], p.dt_sim, p.n_steps)
        cs_sn = trig(ths[:-1])
        if stats is not None and any(abs(float(b) - float(a)) > math.pi for a, b in zip(ths[:-1], ths[1:])):
            stats["wrapped"] = stats.get("wrapped", 0) + p.n_v
        for i in range(p.n_v):
            s = F32(vt[i] * p.dt_sim)
            x, y = F32(pose[0]), F32(pose[1])
            pen, e, ok, in_strip = 0, None, True, 0
            for k in range(p.n_steps):
                x = F32(x + F32(s * cs_sn[k][0]))
                y = F32(y + F32(s * cs_sn[k][1]))
                e = world.cell(x, y)
                if e is None:
                    ok = False
                    if stats is not None:
                        vx, vy = (float(x) - ox) * cpm, (float(y) - oy) * cpm
                        side = "left" if not vx > -1.0 else "right" if not vx < world.w else "bottom" if not vy > -1.0 else "top"
                        stats[side] = stats.get(side, 0) + 1
                    break
                if not world.tcell[e[1], e[0]]:
                    ok = False
                    if stats is not None:
                        stats["blocked"] = stats.get("blocked", 0) + 1
                    break
                pen += int(world.pcell[e[1], e[0]])
                if stats is not None and (float(x) < ox or float(y) < oy):
                    stats["strip"] = stats.get("strip", 0) + 1
                    in_strip += 1
            if not ok:
                continue
            fe = int(world.field[e[1], e[0]])
            if fe == nm.UNREACHED:
                if stats is not None:
                    stats["unreached"] = stats.get("unreached", 0) + 1
                continue
            if stats is not None and in_strip:
                stats["strip_candidates"] = stats.get("strip_candidates", 0) + 1
            h = heading_term(world, e, ths[-1])
            if stats is not None:
                stats.setdefault("terms", {})[j * p.n_v + i] = (fe, h, pen)
            out[j * p.n_v + i] = p.w_field * fe + p.w_heading * h + p.w_clear * pen + p.w_speed * (p.n_v - 1 - i)
    return out


def command(world, p, pose, v, w, stats=None):
    """The result of one state as a RESULT record, and the costs (None when nothing was rolled out)."""
    assert state_ok(pose, v, w)
    r = np.zeros((), RESULT)
    r["index"], r["cost"] = -1, COST_NONE
    flags = world.start_flags(pose[0], pose[1])
    if flags:
        r["flags"] = flags
        if flags == REACHED:
            r["cost"] = 0
        return r, None
    cs = costs(world, p, pose, v, w, stats)
    adm = cs != COST_NONE
    r["n_admissible"] = int(adm.sum())
    if not adm.any():
        r["flags"] = BLOCKED
        return r, cs
    c = int(np.argmin(cs))                                    # the first of the least: ties to the lowest c
    vt, wt = tables(p, v, w)
    r["index"], r["cost"] = c, int(cs[c])
    r["trans_v"], r["angular_v"] = vt[c % p.n_v], wt[c // p.n_v]
    return r, cs


def drive(pose, v, w, p):
    """The unicycle integrated over one control period by the rollout's own arithmetic: steps of dt_sim while a whole one fits into
    dt_control (at least one).  Returns the poses passed through, the last being where the robot is at the next tick."""
    n = max(1, int(math.floor(float(p.dt_control) / float(p.dt_sim) + 1e-6)))
    q = Params(dt_sim=p.dt_sim, n_steps=n)
    return rollout(pose, v, w, q)
