"""The model of the sampling local planner (include/botlab_hip.h, "sampling local planner"), restated in Python: what the kernels of
botlab_amd/csrc/bl_mppi.hip are checked against, byte for byte.  Built over tests/local_plan_model.py (the world, the heading term,
the flags of the pose's own cell) and tests/local_plan_moving_model.py (used slots and their boxes); Philox from
tests/global_init_model.py.  Controls, costs, weights and sums are exact Python or int64 integers; the rollout is numpy float32
operation by operation over all samples at once, with sinf / cosf from the C library through ctypes.
"""
import math

import numpy as np

import global_init_model as gm
import local_plan_model as lpm
import local_plan_moving_model as lmm
import nav_field_model as nm

F32 = np.float32
FELL_BACK = 8
REACHED, OFF_FIELD, BLOCKED = lpm.REACHED, lpm.OFF_FIELD, lpm.BLOCKED
COST_NONE = lpm.COST_NONE
MAX_SAMPLES, MAX_HORIZON, MAX_SUB, MAX_STEPS, MAX_LAMBDA, MAX_Q = 16384, 64, 16, 255, 1 << 30, 1 << 21
TABLE_MUL = 4034748382                                       # floor(2^32 e^(-1/16))
Q16_INV = F32(2.0 ** -16)
RESULT = np.dtype([("trans_v", "<f4"), ("angular_v", "<f4"), ("index_best", "<i4"), ("n_admissible", "<i4"), ("cost_best", "<i8"),
                   ("cost_out", "<i8"), ("weight_sum", "<u8"), ("weight_sq_sum", "<u8"), ("flags", "<i4"), ("pad", "<i4")])
assert RESULT.itemsize == 56
_PI_F = F32(math.pi)


def weight_table():
    """The 257 weights: the recurrence is the definition."""
    t = [1 << 24]
    for _ in range(255):
        t.append((t[-1] * TABLE_MUL) >> 32)
    t.append(0)
    return t


WEIGHTS = np.array(weight_table(), dtype=np.int64)


def q16(x):
    """(int32)lrint((double)x * 65536.0): Python's round is to nearest, ties to even."""
    return int(round(float(F32(x)) * 65536.0))


class Params:
    def __init__(self, v_min=0.0, v_max=0.5, w_max=2.5, acc_v=2.0, acc_w=12.0, dt_sim=0.05, noise_v=0.25, noise_w=1.5, n_samples=1024, horizon=10,
                 n_sub=2, lam=64, w_field=16, w_heading=0, w_clear=1, seed=1):
        self.v_min, self.v_max, self.w_max = F32(v_min), F32(v_max), F32(w_max)
        self.acc_v, self.acc_w, self.dt_sim = F32(acc_v), F32(acc_w), F32(dt_sim)
        self.noise_v, self.noise_w = F32(noise_v), F32(noise_w)
        self.K, self.T, self.n_sub, self.lam = int(n_samples), int(horizon), int(n_sub), int(lam)
        self.w_field, self.w_heading, self.w_clear = int(w_field), int(w_heading), int(w_clear)
        self.seed = int(seed)

    @property
    def n_steps(self):
        return self.T * self.n_sub

    def floats(self):
        return [self.v_min, self.v_max, self.w_max, self.acc_v, self.acc_w, self.dt_sim, self.noise_v, self.noise_w]

    def derived(self):
        """(vmin_q, vmax_q, wmax_q, nv_q, nw_q, av_q, aw_q)"""
        acc = [int(round(float(a) * float(self.dt_sim) * self.n_sub * 65536.0)) for a in (self.acc_v, self.acc_w)]
        return [q16(self.v_min), q16(self.v_max), q16(self.w_max), q16(self.noise_v), q16(self.noise_w)] + acc

    def ok(self):
        """bl_mppi_set_params' rule."""
        if not all(math.isfinite(float(f)) for f in self.floats()):
            return False
        if self.v_min > self.v_max or self.w_max < 0 or self.noise_v < 0 or self.noise_w < 0 or self.acc_v < 0 or self.acc_w < 0 or not self.dt_sim > 0:
            return False
        if not (1 <= self.K <= MAX_SAMPLES and 1 <= self.T <= MAX_HORIZON and 1 <= self.n_sub <= MAX_SUB and self.n_steps <= MAX_STEPS):
            return False
        if not 1 <= self.lam <= MAX_LAMBDA or not all(0 <= w <= lpm.MAX_WEIGHT for w in (self.w_field, self.w_heading, self.w_clear)):
            return False
        return all(abs(q) < MAX_Q for q in self.derived())

    def v_abs(self):
        return max(abs(float(self.v_min)), abs(float(self.v_max)))

    def can_skip_a_cell(self, mpc):
        return self.v_abs() * float(self.dt_sim) > float(F32(mpc))

    def staged(self, cpm):
        r = int(math.ceil(self.v_abs() * float(self.dt_sim) * self.n_steps * float(F32(cpm)))) + 2
        return (2 * r + 1) * (2 * r + 1) * 2 <= lpm.WINDOW_BYTES


def state_ok(pose, v, w):
    return lpm.state_ok(pose, v, w) and abs(q16(v)) < MAX_Q and abs(q16(w)) < MAX_Q


# ---------------------------------------------------------------------------------------------------------------- sequences
def draws(p, tick, stream):
    """(e_v, e_w) int64 [K, T]: the Irwin-Hall sums of every sample and period."""
    k = np.arange(p.K, dtype=np.uint64)[:, None]
    t = np.arange(p.T, dtype=np.uint64)[None, :]
    a = gm.philox4x32(k, t, int(stream), int(tick), p.seed & gm.MASK32, (p.seed >> 32) & gm.MASK32)
    lo, s16 = np.uint64(0xFFFF), np.uint64(16)

    def ih(x, y):
        return ((x & lo) + (x >> s16) + (y & lo) + (y >> s16)).astype(np.int64) - 131070

    return ih(a[0], a[1]), ih(a[2], a[3])


def clamp_chain(raw, prev, lim_lo, lim_hi, a_q):
    """raw int64 [..., T] through the chain, prev the control before t = 0 (an int).  Returns int64 of the same shape."""
    raw = np.asarray(raw, dtype=np.int64)
    out = np.empty_like(raw)
    pv = np.full(raw.shape[:-1], int(prev), dtype=np.int64)
    for t in range(raw.shape[-1]):
        lo, hi = np.maximum(lim_lo, pv - a_q), np.minimum(lim_hi, pv + a_q)
        both = np.minimum(np.maximum(pv, lim_lo), lim_hi)
        bad = lo > hi
        lo, hi = np.where(bad, both, lo), np.where(bad, both, hi)
        pv = np.minimum(np.maximum(raw[..., t], lo), hi)
        out[..., t] = pv
    return out


def clamp_seq(p, raw, v, w):
    """raw int64 [..., T, 2] through both channels' chains from the state's (v, w)."""
    vmin, vmax, wmax, _, _, av, aw = p.derived()
    raw = np.asarray(raw, dtype=np.int64)
    return np.stack([clamp_chain(raw[..., 0], q16(v), vmin, vmax, av), clamp_chain(raw[..., 1], q16(w), -wmax, wmax, aw)], axis=-1)


def sample_seqs(p, v, w, tick, stream, u_in=None):
    """int64 [K, T, 2]: the control sequence of every sample."""
    u = np.zeros((p.T, 2), np.int64) if u_in is None else np.asarray(u_in, dtype=np.int64).reshape(p.T, 2)
    ev, ew = draws(p, tick, stream)
    nv, nw = p.derived()[3:5]
    raw = np.stack([u[None, :, 0] + ((ev * nv) >> 17), u[None, :, 1] + ((ew * nw) >> 17)], axis=-1)    # >> of int64: floor
    raw[0] = u
    if p.K >= 2:
        raw[1] = 0
    return clamp_seq(p, raw, v, w)


# ---------------------------------------------------------------------------------------------------------------- rollout
def _wrap(th):
    """bl_wrap_to_pi over a float32 array."""
    th = th.copy()
    while True:
        lo = th <= -_PI_F
        if not lo.any():
            break
        th[lo] = (th[lo].astype(np.float64) + 2.0 * math.pi).astype(np.float32)
    while True:
        hi = th >= _PI_F
        if not hi.any():
            break
        th[hi] = (th[hi].astype(np.float64) - 2.0 * math.pi).astype(np.float32)
    return th


def _trig(th):
    cs = np.fromiter((lpm._libm.cosf(float(t)) for t in th), np.float32, len(th))
    sn = np.fromiter((lpm._libm.sinf(float(t)) for t in th), np.float32, len(th))
    return cs, sn


def poses(p, pose, seqs):
    """x, y, theta float32 [M, n_steps] of the sequences int [M, T, 2]."""
    seqs = np.asarray(seqs, dtype=np.int64)
    M, n = seqs.shape[0], p.n_steps
    x, y = np.full(M, F32(pose[0]), np.float32), np.full(M, F32(pose[1]), np.float32)
    th = _wrap(np.full(M, F32(pose[2]), np.float32))
    xs, ys, ths = (np.zeros((M, n), np.float32) for _ in range(3))
    step = 0
    for t in range(p.T):
        v = seqs[:, t, 0].astype(np.float32) * Q16_INV
        w = seqs[:, t, 1].astype(np.float32) * Q16_INV
        s, dth = v * p.dt_sim, w * p.dt_sim
        for _ in range(p.n_sub):
            cs, sn = _trig(th)
            x = x + s * cs
            y = y + s * sn
            th = _wrap(th + dth)
            assert x.dtype == np.float32 and th.dtype == np.float32
            xs[:, step], ys[:, step], ths[:, step] = x, y, th
            step += 1
    return xs, ys, ths


def rollouts(world, p, pose, seqs):
    """poses(), and the visited cells: cx, cy int64 [M, n_steps] with inside bool [M, n_steps] (a cell is meaningful where inside)."""
    xs, ys, ths = poses(p, pose, seqs)
    ox, oy, cpm = float(F32(world.origin[0])), float(F32(world.origin[1])), float(world.cpm)
    vx, vy = (xs.astype(np.float64) - ox) * cpm, (ys.astype(np.float64) - oy) * cpm
    inside = (vx > -1.0) & (vx < world.w) & (vy > -1.0) & (vy < world.h)
    cx, cy = np.where(inside, np.trunc(vx), 0).astype(np.int64), np.where(inside, np.trunc(vy), 0).astype(np.int64)
    return xs, ys, ths, cx, cy, inside


def first_hits(p, slots, m, cx, cy, inside):
    """int32 [M]: the least step whose cell lies in a used slot's box at that step, 0 when there is none."""
    out = np.zeros(cx.shape[0], np.int32)
    us = lmm.used_slots(slots) if slots is not None else []
    if not us:
        return out
    for k in range(p.n_steps, 0, -1):
        hit = np.zeros(cx.shape[0], bool)
        for s in us:
            b = lmm.box_at(s, k, m)
            hit |= inside[:, k - 1] & (cx[:, k - 1] >= b[0]) & (cx[:, k - 1] <= b[2]) & (cy[:, k - 1] >= b[1]) & (cy[:, k - 1] <= b[3])
        out[hit] = k
    return out


def seq_costs(world, p, pose, seqs, slots=None, m=None):
    """(costs int64 [M], first_hit int32 [M]) of the sequences: COST_NONE for an inadmissible one."""
    xs, ys, ths, cx, cy, inside = rollouts(world, p, pose, seqs)
    M = cx.shape[0]
    trav = inside & world.tcell[cy, cx].astype(bool)
    ok = trav.all(axis=1)
    pen = np.where(trav, world.pcell[cy, cx].astype(np.int64), 0).sum(axis=1)
    fh = first_hits(p, slots, m, cx, cy, inside)
    ok &= fh == 0
    out = np.full(M, COST_NONE, dtype=np.int64)
    for i in np.flatnonzero(ok):
        e = (int(cx[i, -1]), int(cy[i, -1]))
        fe = int(world.field[e[1], e[0]])
        if fe == nm.UNREACHED:
            continue
        out[i] = p.w_field * fe + p.w_heading * lpm.heading_term(world, e, ths[i, -1]) + p.w_clear * int(pen[i])
    return out, fh


def weights(p, costs):
    """(W int64 [K], c_min, best): c_min None when no sample is admissible."""
    adm = costs != COST_NONE
    if not adm.any():
        return np.zeros(len(costs), np.int64), None, -1
    best = int(np.argmin(costs))                                # the first of the least: ties to the lowest k
    c_min = int(costs[best])
    idx = np.minimum((np.where(adm, costs - c_min, 0) * 16) // p.lam, 256)
    return np.where(adm, WEIGHTS[idx], 0).astype(np.int64), c_min, best


def average(W, seqs):
    """a [T, 2] as Python integers: floor((2 N + S) / (2 S)) with exact sums."""
    S = int(W.sum())
    out = []
    for t in range(seqs.shape[1]):
        row = []
        for c in range(2):
            N = sum(int(a) * int(b) for a, b in zip(W.tolist(), seqs[:, t, c].tolist()) if a)
            row.append((2 * N + S) // (2 * S))                  # Python's // is floor
        out.append(row)
    return out


def plan(world, p, pose, v, w, tick=0, stream=0, u_in=None, slots=None, m=None):
    """One state: (RESULT record, seq_out int32 [T, 2], dict(costs, seqs, first_hit, weights, candidate) or None when nothing was
    drawn)."""
    assert state_ok(pose, v, w) and p.ok()
    r = np.zeros((), RESULT)
    r["index_best"], r["cost_best"], r["cost_out"] = -1, COST_NONE, COST_NONE
    seq_out = np.zeros((p.T, 2), np.int32)
    flags = world.start_flags(pose[0], pose[1])
    if flags:
        r["flags"] = flags
        if flags == REACHED:
            r["cost_best"] = r["cost_out"] = 0
        return r, seq_out, None
    seqs = sample_seqs(p, v, w, tick, stream, u_in)
    costs, fh = seq_costs(world, p, pose, seqs, slots, m)
    W, c_min, best = weights(p, costs)
    info = dict(costs=costs, seqs=seqs, first_hit=fh, weights=W)
    if c_min is None:
        r["flags"] = BLOCKED
        return r, seq_out, info
    cand = clamp_seq(p, np.array(average(W, seqs), dtype=np.int64), v, w)
    info["candidate"] = cand
    cc, _ = seq_costs(world, p, pose, cand[None], slots, m)
    r["index_best"], r["n_admissible"], r["cost_best"] = best, int((costs != COST_NONE).sum()), c_min
    r["weight_sum"], r["weight_sq_sum"] = int(W.sum()), sum(int(a) * int(a) for a in W.tolist())
    if int(cc[0]) != COST_NONE:
        seq_out[:] = cand
        r["cost_out"] = int(cc[0])
    else:
        seq_out[:] = seqs[best]
        r["cost_out"], r["flags"] = c_min, FELL_BACK
    r["trans_v"], r["angular_v"] = F32(seq_out[0, 0]) * Q16_INV, F32(seq_out[0, 1]) * Q16_INV
    return r, seq_out, info


def debug_samples(world, p, pose, v, w, tick=0, stream=0, u_in=None, slots=None, m=None):
    """bl_mppi_debug_samples: (costs, first_hit, seqs), rolled out whatever the state's flags would be."""
    seqs = sample_seqs(p, v, w, tick, stream, u_in)
    costs, fh = seq_costs(world, p, pose, seqs, slots, m)
    return costs, fh, seqs.astype(np.int32)


def advance(seq, flags):
    """MppiPlanner.advance: the held sequence shifted by one period, the last control repeated; zeros after any flag but FELL_BACK."""
    if int(flags) & ~FELL_BACK:
        return np.zeros_like(seq)
    return np.concatenate([seq[1:], seq[-1:]], axis=0)


def drive(pose, seq0, p):
    """The unicycle over one control period (n_sub steps of dt_sim) under the control seq0 = (q_v, q_w), by the rollout's own
    arithmetic.  Returns the poses passed through."""
    q = Params(dt_sim=p.dt_sim, horizon=1, n_sub=p.n_sub)
    xs, ys, ths = poses(q, pose, np.array([[seq0]], dtype=np.int64))
    return [(xs[0, i], ys[0, i], ths[0, i]) for i in range(p.n_sub)]
