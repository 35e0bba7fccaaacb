"""Operation-for-operation model of the pose-graph solver (bl_posegraph.hip), and an independent dense solve.

solve() restates k_pg_solve: numpy float64 operation by operation (no fused operations), every sum in the kernel's order, sinf / cosf
of the heading narrowed to float from the C library through ctypes (glibc's, which bl_math.h reproduces bit for bit).  The device
result is compared with it bit for bit.  dense_solve() is the same step control around plain normal equations through
np.linalg.solve: it shares the residual's definition and nothing else, and agrees within a bound.
"""
import ctypes
import ctypes.util
import math
from collections import namedtuple

import numpy as np

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.sinf.restype = ctypes.c_float
_libm.sinf.argtypes = [ctypes.c_float]
_libm.cosf.restype = ctypes.c_float
_libm.cosf.argtypes = [ctypes.c_float]

PG_T = 512
PI = 3.141592653589793
TWO_PI = 6.283185307179586
CONVERGED_STEP, CONVERGED_DECREASE, OUT_OF_TRIES, CG_CAP = 1, 2, 3, 16

Params = namedtuple("Params", "fixed max_tries max_cg lambda0 lambda_up lambda_down step_tol rel_tol cg_tol")
DEFAULT = Params(fixed=0, max_tries=20, max_cg=500, lambda0=1e-6, lambda_up=10.0, lambda_down=0.1, step_tol=1e-6, rel_tol=1e-6, cg_tol=1e-8)
Result = namedtuple("Result", "cost_before cost_after tries accepted cg_iterations final_lambda status poses chi2_before chi2_after "
                              "poses32 cg_per_try wrapped trial_wrapped node_lists cg_ends")

_SYM = ((0, 0), (0, 1), (1, 1), (0, 2), (1, 2), (2, 2))        # xx, xy, yy, xt, yt, tt


def sincos32(theta):
    """sin, cos (float64 arrays) of float64 headings narrowed to float"""
    t32 = np.asarray(theta, np.float64).astype(np.float32)
    s = np.array([_libm.sinf(float(v)) for v in t32.ravel()], np.float32).astype(np.float64).reshape(t32.shape)
    c = np.array([_libm.cosf(float(v)) for v in t32.ravel()], np.float32).astype(np.float64).reshape(t32.shape)
    return s, c


def wrap(d):
    d = np.asarray(d, np.float64)
    return np.where(d > PI, d - TWO_PI, np.where(d < -PI, d + TWO_PI, d))


def full(s6):
    """(..., 6) symmetric -> (..., 3, 3)"""
    m = np.zeros(s6.shape[:-1] + (3, 3))
    for q, (r, c) in enumerate(_SYM):
        m[..., r, c] = s6[..., q]
        m[..., c, r] = s6[..., q]
    return m


def sym6(m):
    return np.stack([m[..., r, c] for r, c in _SYM], -1)


def tr(m):
    return np.swapaxes(m, -1, -2)


def mm(A, B):
    """every entry (a0 b0 + a1 b1) + a2 b2"""
    o = np.zeros(np.broadcast(A[..., 0, 0], B[..., 0, 0]).shape + (3, 3))
    for r in range(3):
        for c in range(3):
            o[..., r, c] = (A[..., r, 0] * B[..., 0, c] + A[..., r, 1] * B[..., 1, c]) + A[..., r, 2] * B[..., 2, c]
    return o


def mv(A, v):
    return np.stack([(A[..., r, 0] * v[..., 0] + A[..., r, 1] * v[..., 1]) + A[..., r, 2] * v[..., 2] for r in range(3)], -1)


def inv6(s):
    a, b, c, d, e, f = (s[..., q] for q in range(6))
    c00, c01, c02 = c * f - e * e, d * e - b * f, b * e - c * d
    c11, c12, c22 = a * f - d * d, b * d - a * e, a * c - b * b
    det = (a * c00 + b * c01) + d * c02
    return np.stack([c00 / det, c01 / det, c11 / det, c02 / det, c12 / det, c22 / det], -1)


def tree_sum(terms):
    """thread t of PG_T adds its terms t, t + PG_T, ... from 0; the partial sums fold in halves"""
    terms = np.asarray(terms, np.float64)
    rows = -(-max(len(terms), 1) // PG_T)
    pad = np.zeros(rows * PG_T)
    pad[:len(terms)] = terms
    acc = np.zeros(PG_T)
    for row in pad.reshape(rows, PG_T):
        acc = acc + row
    h = PG_T // 2
    while h >= 1:
        acc[:h] = acc[:h] + acc[h:2 * h]
        h //= 2
    return float(acc[0])


def dot(a, b):
    return tree_sum((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2])


def residual(xi, xj, z):
    """e, sin, cos, rx, ry and the heading difference before the wrap"""
    s, c = sincos32(xi[..., 2])
    dx, dy = xj[..., 0] - xi[..., 0], xj[..., 1] - xi[..., 1]
    rx = c * dx + s * dy
    ry = c * dy - s * dx
    raw = (xj[..., 2] - xi[..., 2]) - z[..., 2]
    e = np.stack([rx - z[..., 0], ry - z[..., 1], wrap(raw)], -1)
    return e, s, c, rx, ry, raw


def relative_pose(xi, xj):
    """pose j seen from pose i by the residual's statements (set_chain_from_nodes)"""
    xi, xj = np.asarray(xi, np.float64), np.asarray(xj, np.float64)
    return residual(xi, xj, np.zeros_like(xi))[0]


class Graph:
    """nodes (N, 3) float64 (the device takes them as floats: pass float32 values); edges: i, j int arrays, z (E, 3), info (E, 6);
    the first N - 1 are the chain."""

    def __init__(self, nodes, ei, ej, z, info):
        self.nodes = np.asarray(nodes, np.float64).copy()
        self.N = len(self.nodes)
        self.i, self.j = np.asarray(ei, np.int64), np.asarray(ej, np.int64)
        self.z, self.info = np.asarray(z, np.float64).reshape(-1, 3), np.asarray(info, np.float64).reshape(-1, 6)
        self.E = len(self.i)
        self.L = self.E - (self.N - 1)
        assert np.array_equal(self.i[:self.N - 1], np.arange(self.N - 1)) and np.array_equal(self.j[:self.N - 1], np.arange(1, self.N))


def in_force(g, mask):
    """bool (E): the chain, and the loop edges whose mask bit is set and whose information is not all zero"""
    on = np.ones(g.E, bool)
    for l in range(g.L):
        bit = True if mask is None else bool((int(mask[l >> 5]) >> (l & 31)) & 1)
        on[g.N - 1 + l] = bit and bool(np.any(g.info[g.N - 1 + l] != 0.0))
    return on


def _edges(g, x, on, fixed, want_full):
    e, s, c, rx, ry, raw = residual(x[g.i], x[g.j], g.z)
    Om = full(g.info)
    oe = mv(Om, e)
    chi = (e[:, 0] * oe[:, 0] + e[:, 1] * oe[:, 1]) + e[:, 2] * oe[:, 2]
    F = tree_sum(chi[on])                               # the edges in force are the terms, the others are left out
    if not want_full:
        return F, chi, None
    A = np.zeros((g.E, 3, 3))
    B = np.zeros((g.E, 3, 3))
    A[:, 0, 0], A[:, 0, 1], A[:, 0, 2] = -c, -s, ry
    A[:, 1, 0], A[:, 1, 1], A[:, 1, 2] = s, -c, -rx
    A[:, 2, 2] = -1.0
    B[:, 0, 0], B[:, 0, 1], B[:, 1, 0], B[:, 1, 1], B[:, 2, 2] = c, s, -s, c, 1.0
    A[g.i == fixed] = 0.0
    B[g.j == fixed] = 0.0
    OA, OB = mm(Om, A), mm(Om, B)
    blocks = dict(AA=sym6(mm(tr(A), OA)), BB=sym6(mm(tr(B), OB)), AB=mm(tr(A), OB), ga=mv(tr(A), oe), gb=mv(tr(B), oe),
                  wrapped=bool(np.any(np.abs(raw) > PI)))
    return F, chi, blocks


def _gather(g, b, loops_on):
    """D (N, 6) and g (N, 3): from 0, chain edge k - 1, chain edge k, then the node's loop edges ascending"""
    N = g.N
    D, gr = np.zeros((N, 6)), np.zeros((N, 3))
    D[1:] = D[1:] + b["BB"][:N - 1]
    gr[1:] = gr[1:] + b["gb"][:N - 1]
    D[:-1] = D[:-1] + b["AA"][:N - 1]
    gr[:-1] = gr[:-1] + b["ga"][:N - 1]
    for e in loops_on:
        i, j = g.i[e], g.j[e]
        D[i] = D[i] + b["AA"][e]
        gr[i] = gr[i] + b["ga"][e]
        D[j] = D[j] + b["BB"][e]
        gr[j] = gr[j] + b["gb"][e]
    return D, gr


class _Factor:
    """block cyclic reduction of the block-tridiagonal (Dl, chain A'Omega B): pg_factor and pg_tsolve"""

    def __init__(self, Dl, U0):
        N = len(Dl)
        self.N = N
        Dw = Dl.copy()
        Up = np.zeros((N, 3, 3))
        Up[:N - 1] = U0
        Lo = np.zeros((N, 3, 3))
        s = 1
        while s <= N:
            e = np.arange(s - 1, N, 2 * s)
            Dw[e] = inv6(Dw[e])
            el = e[e - s >= 0]
            Lo[el] = tr(Up[el - s])
            k = np.arange(2 * s - 1, N, 2 * s)
            if len(k):
                lo = k - s
                U = Up[lo]
                M = mm(tr(U), full(Dw[lo]))
                d = Dw[k] - sym6(mm(M, U))
                has = k + s < N
                kh = k[has]
                if len(kh):
                    hi = kh + s
                    Uk = Up[kh]
                    G = mm(Uk, full(Dw[hi]))
                    d[has] = d[has] - sym6(mm(G, tr(Uk)))
                    far = hi + s < N
                    if np.any(far):
                        Up[kh[far]] = -mm(G[far], Up[hi[far]])
                Dw[k] = d
            s *= 2
        self.Dw, self.Up, self.Lo = Dw, Up, Lo

    def solve(self, v):
        N = self.N
        v = v.copy()
        Dw, Up, Lo = self.Dw, self.Up, self.Lo
        s = 1
        top = 1
        while s <= N:
            top = s
            e = np.arange(s - 1, N, 2 * s)
            v[e] = mv(full(Dw[e]), v[e])
            k = np.arange(2 * s - 1, N, 2 * s)
            if len(k):
                lo = k - s
                vk = v[k] - mv(tr(Up[lo]), v[lo])
                has = k + s < N
                hi = k[has] + s
                vk[has] = vk[has] - mv(tr(Lo[hi]), v[hi])
                v[k] = vk
            s *= 2
        s = top
        while s >= 1:
            e = np.arange(s - 1, N, 2 * s)
            has_lo, has_hi = e - s >= 0, e + s < N
            t = np.zeros((len(e), 3))
            both, only_lo, only_hi = has_lo & has_hi, has_lo & ~has_hi, ~has_lo & has_hi
            if np.any(both):
                eb = e[both]
                t[both] = mv(Lo[eb], v[eb - s]) + mv(Up[eb], v[eb + s])
            if np.any(only_lo):
                eb = e[only_lo]
                t[only_lo] = mv(Lo[eb], v[eb - s])
            if np.any(only_hi):
                eb = e[only_hi]
                t[only_hi] = mv(Up[eb], v[eb + s])
            some = has_lo | has_hi
            es = e[some]
            v[es] = v[es] - mv(full(Dw[es]), t[some])
            s //= 2
        return v


def _hp(g, Dl, AB, loops_on, p):
    N = g.N
    o = mv(full(Dl), p)
    o[1:] = o[1:] + mv(tr(AB[:N - 1]), p[:-1])
    o[:-1] = o[:-1] + mv(AB[:N - 1], p[1:])
    if len(loops_on):
        # per node in ascending edge order: np.add.at applies its updates one after the other, in the order given
        e = np.asarray(loops_on)
        i, j = g.i[e], g.j[e]
        node = np.stack([i, j], 1).ravel()
        term = np.stack([mv(AB[e], p[j]), mv(tr(AB[e]), p[i])], 1).reshape(-1, 3)
        np.add.at(o, node, term)
    return o


def solve(g, prm=DEFAULT, mask=None):
    """k_pg_solve for one subset"""
    N = g.N
    on = in_force(g, mask)
    loops_on = [e for e in range(N - 1, g.E) if on[e]]
    x = g.nodes.copy()
    F, chi, b = _edges(g, x, on, prm.fixed, True)
    wrapped = b["wrapped"]
    chi0, F0 = chi.copy(), F
    D, gr = _gather(g, b, loops_on)
    lam = prm.lambda0
    tries = accepted = cg_total = 0
    status, cap = OUT_OF_TRIES, 0
    cg_per_try = []
    # what the cases' conditions read, beside the results: whether a trial heading left [-pi, pi] before its wrap, the length of every
    # node's list of loop entries, and how each try's iteration ended -- ("tol" | "cap" | "php" | "none", the last r' T^-1 r)
    trial_wrapped = False
    ends = np.concatenate([g.i[loops_on], g.j[loops_on]]) if loops_on else np.zeros(0, np.int64)
    node_lists = np.bincount(ends, minlength=N)
    cg_ends = []
    free = np.arange(N) != prm.fixed
    while tries < prm.max_tries:
        tries += 1
        Dl = D.copy()
        Dl[:, 0] = Dl[:, 0] + lam
        Dl[:, 2] = Dl[:, 2] + lam
        Dl[:, 5] = Dl[:, 5] + lam
        Dl[prm.fixed] = (1.0, 0.0, 1.0, 0.0, 0.0, 1.0)
        AB = b["AB"]
        fac = _Factor(Dl, AB[:N - 1])
        r = -gr
        z = fac.solve(r)
        p = z.copy()
        dx = np.zeros((N, 3))
        rz = dot(r, z)
        rz0 = rz
        tol = (prm.cg_tol * prm.cg_tol) * rz0
        it = 0
        done = not (rz0 > 0.0)
        end, last = "none" if done else "cap", rz0
        while not done and it < prm.max_cg:
            hp = _hp(g, Dl, AB, loops_on, p)
            php = dot(p, hp)
            if not (php > 0.0):
                end = "php"
                break
            al = rz / php
            dx = dx + al * p
            r = r - al * hp
            z = fac.solve(r)
            rz2 = dot(r, z)
            it += 1
            last = rz2
            if rz2 <= tol:
                done = True
                end = "tol"
                break
            beta = rz2 / rz
            p = z + beta * p
            rz = rz2
        cg_ends.append((end, last))
        cg_total += it
        cg_per_try.append(it)
        if not done:
            cap = 1
        if rz0 == 0.0:
            status = CONVERGED_STEP
            break
        xn = x.copy()
        xn[free, 0] = x[free, 0] + dx[free, 0]
        xn[free, 1] = x[free, 1] + dx[free, 1]
        trial = x[free, 2] + dx[free, 2]
        trial_wrapped = trial_wrapped or bool(np.any(np.abs(trial) > PI))
        xn[free, 2] = wrap(trial)
        md = float(np.max(np.abs(dx[free]))) if np.any(free) else 0.0
        F2, _, _ = _edges(g, xn, on, prm.fixed, False)
        if F2 < F:
            accepted += 1
            x = xn
            Fold = F
            F, chi, b = _edges(g, x, on, prm.fixed, True)
            wrapped = wrapped or b["wrapped"]
            D, gr = _gather(g, b, loops_on)
            if md <= prm.step_tol:
                status = CONVERGED_STEP
                break
            if Fold - F <= prm.rel_tol * Fold:
                status = CONVERGED_DECREASE
                break
            lam = lam * prm.lambda_down
        else:
            lam = lam * prm.lambda_up
    return Result(F0, F, tries, accepted, cg_total, lam, status | (CG_CAP if cap else 0), x, chi0, chi, x.astype(np.float32), cg_per_try, wrapped,
                  trial_wrapped, node_lists, cg_ends)


# ---------------------------------------------------------------- the independent dense solve
def _dense_build(g, x, on, fixed):
    N = g.N
    H, gv, F = np.zeros((3 * N, 3 * N)), np.zeros(3 * N), 0.0
    for e in range(g.E):
        if not on[e]:
            continue
        i, j = int(g.i[e]), int(g.j[e])
        c, s = math.cos(float(np.float32(x[i, 2]))), math.sin(float(np.float32(x[i, 2])))
        dx, dy = x[j, 0] - x[i, 0], x[j, 1] - x[i, 1]
        d = x[j, 2] - x[i, 2] - g.z[e, 2]
        d = (d + math.pi) % (2 * math.pi) - math.pi
        r = np.array([c * dx + s * dy - g.z[e, 0], -s * dx + c * dy - g.z[e, 1], d])
        Om = full(g.info[e])
        A = np.array([[-c, -s, -s * dx + c * dy], [s, -c, -c * dx - s * dy], [0, 0, -1.0]])
        B = np.array([[c, s, 0], [-s, c, 0], [0, 0, 1.0]])
        F += r @ Om @ r
        for p, P in ((i, A), (j, B)):
            gv[3 * p:3 * p + 3] += P.T @ Om @ r
            for q, Q in ((i, A), (j, B)):
                H[3 * p:3 * p + 3, 3 * q:3 * q + 3] += P.T @ Om @ Q
    return H, gv, F


def dense_solve(g, prm=DEFAULT, mask=None):
    """the same step control around np.linalg.solve of the normal equations: (poses, cost, tries, accepted)"""
    N = g.N
    on = in_force(g, mask)
    keep = np.ones(3 * N, bool)
    keep[3 * prm.fixed:3 * prm.fixed + 3] = False
    x = g.nodes.copy()
    H, gv, F = _dense_build(g, x, on, prm.fixed)
    lam, tries, accepted = prm.lambda0, 0, 0
    while tries < prm.max_tries:
        tries += 1
        Hk = H[np.ix_(keep, keep)] + lam * np.eye(3 * N - 3)
        d = np.zeros(3 * N)
        d[keep] = np.linalg.solve(Hk, -gv[keep])
        if not np.any(d):
            break
        xn = x + d.reshape(N, 3)
        xn[:, 2] = (xn[:, 2] + math.pi) % (2 * math.pi) - math.pi
        H2, g2, F2 = _dense_build(g, xn, on, prm.fixed)
        if F2 < F:
            accepted += 1
            Fold = F
            x, H, gv, F = xn, H2, g2, F2
            if np.abs(d).max() <= prm.step_tol or Fold - F <= prm.rel_tol * Fold:
                break
            lam *= prm.lambda_down
        else:
            lam *= prm.lambda_up
    return x, F, tries, accepted
