"""bl_pf_clusters (include/botlab_hip.h) in Python integers: a dict of bins, a union-find over them, exact sums; and
bl_pf_cluster_pose on top of it.  A second component finder -- breadth-first search that tests every pair of bins -- shares no
code with the first.  sinf / cosf come from the C library through ctypes (bl_sincosf reproduces glibc bit for bit)."""
import ctypes
import ctypes.util
import math

import numpy as np

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.sinf.restype = ctypes.c_float
_libm.sinf.argtypes = [ctypes.c_float]
_libm.cosf.restype = ctypes.c_float
_libm.cosf.argtypes = [ctypes.c_float]

SUMS = ("sx", "sy", "sxx", "syy", "sxy", "sc", "ss")
TWO_PI = 6.283185307179586


def _clamp_floor(v64, lim):
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.floor(v64)
        q = np.where(np.isnan(q), -lim, np.clip(q, -lim, lim - 1.0))
    return q.astype(np.int64)


def particle_terms(x, y, th, bin_xy, T):
    """(px, py, it, si, ci) as int64 arrays: the per-particle integers of the definition."""
    x, y, th = (np.asarray(a, np.float32) for a in (x, y, th))
    xy_scale = 1024.0 / float(bin_xy)
    th_scale = float(T) / TWO_PI
    with np.errstate(invalid="ignore", over="ignore"):
        px = _clamp_floor(x.astype(np.float64) * xy_scale, 2.0 ** 30)
        py = _clamp_floor(y.astype(np.float64) * xy_scale, 2.0 ** 30)
        q = _clamp_floor(th.astype(np.float64) * th_scale, 2.0 ** 40)
    it = q % np.int64(T)
    si = np.zeros(len(th), np.int64)
    ci = np.zeros(len(th), np.int64)
    for m, a in enumerate(th):
        if np.isfinite(a) and abs(float(a)) < 100.0:
            si[m] = int(np.rint(np.float64(_libm.sinf(float(a))) * 1048576.0))
            ci[m] = int(np.rint(np.float64(_libm.cosf(float(a))) * 1048576.0))
    return px, py, it, si, ci


def _adjacent_steps(T):
    """Heading steps that lead to different neighbours: T = 1 has none but 0, T = 2 one."""
    return sorted({d % T for d in (-1, 0, 1)})


def bins_of(x, y, th, units, bin_xy, T):
    """dict bin -> [count, U, sx, sy, sxx, syy, sxy, sc, ss] in absolute fine coordinates, and each particle's bin."""
    px, py, it, si, ci = particle_terms(x, y, th, bin_xy, T)
    bins, where = {}, []
    for m in range(len(px)):
        a, b, u = int(px[m]), int(py[m]), int(units[m])
        key = (a >> 10, b >> 10, int(it[m]))
        where.append(key)
        e = bins.setdefault(key, [0] * 9)
        e[0] += 1
        e[1] += u
        e[2] += u * a
        e[3] += u * b
        e[4] += u * a * a
        e[5] += u * b * b
        e[6] += u * a * b
        e[7] += u * int(ci[m])
        e[8] += u * int(si[m])
    return bins, where


def components_union_find(keys, T):
    """bin -> representative, by union-find over the 26 neighbours found in the dict."""
    parent = {k: k for k in keys}

    def find(k):
        while parent[k] != k:
            parent[k] = parent[parent[k]]
            k = parent[k]
        return k

    steps = _adjacent_steps(T)
    for (ix, iy, it) in keys:
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dt in steps:
                    nb = (ix + dx, iy + dy, (it + dt) % T)
                    if nb != (ix, iy, it) and nb in parent:
                        ra, rb = find((ix, iy, it)), find(nb)
                        if ra != rb:
                            parent[ra] = rb
    return {k: find(k) for k in keys}


def components_brute_force(keys, T):
    """bin -> component number, by breadth-first search testing every bin against every other (numpy rows)."""
    keys = list(keys)
    a = np.array(keys, np.int64).reshape(-1, 3)
    comp = -np.ones(len(keys), np.int64)
    n = 0
    for s in range(len(keys)):
        if comp[s] >= 0:
            continue
        comp[s] = n
        todo = [s]
        while todo:
            i = todo.pop()
            d = a - a[i]
            dt = np.abs(d[:, 2])
            dt = np.minimum(dt, T - dt)
            adj = (np.abs(d[:, 0]) <= 1) & (np.abs(d[:, 1]) <= 1) & (dt <= 1) & (comp < 0)
            for j in np.flatnonzero(adj):
                comp[j] = n
                todo.append(int(j))
        n += 1
    return {k: int(c) for k, c in zip(keys, comp)}


def clusters(x, y, th, units, bin_xy, T, K, finder=components_union_find):
    """The whole result: dict of num_clusters, units_sum, active, clusters (ALL of them, in order; the call reports the first K),
    labels (int32 per particle, -1 beyond rank K - 1)."""
    bins, where = bins_of(x, y, th, units, bin_xy, T)
    rep = finder(bins.keys(), T)
    groups = {}
    for k, r in rep.items():
        groups.setdefault(r, []).append(k)
    out = []
    for r, ks in groups.items():
        tot = [sum(bins[k][f] for k in ks) for f in range(9)]
        c = {"count": tot[0], "units": tot[1], "anchor": min(ks), "bins": ks}
        c.update({n: tot[2 + i] for i, n in enumerate(SUMS)})
        out.append(c)
    out.sort(key=lambda c: (-c["units"], c["anchor"]))
    rank_of = {}
    for rank, c in enumerate(out):
        for k in c["bins"]:
            rank_of[k] = rank
    labels = np.array([rank_of[k] if rank_of[k] < K else -1 for k in where], np.int32)
    return {"num_clusters": len(out), "units_sum": sum(int(u) for u in units), "active": len(where), "clusters": out, "labels": labels}


def cluster_pose(c, units_sum, bin_xy):
    """bl_pf_cluster_pose: the same expressions, Python integers for the 128-bit ones (int -> float rounds correctly, once)."""
    U = c["units"]
    if U == 0:
        return None
    xy_scale = 1024.0 / float(bin_xy)
    ax, ay = 1024 * c["anchor"][0], 1024 * c["anchor"][1]
    rx, ry = c["sx"] - ax * U, c["sy"] - ay * U
    rxx = c["sxx"] - 2 * ax * c["sx"] + ax * ax * U
    ryy = c["syy"] - 2 * ay * c["sy"] + ay * ay * U
    rxy = c["sxy"] - ax * c["sy"] - ay * c["sx"] + ax * ay * U
    dU = float(U)
    mx, my = float(rx) / dU, float(ry) / dU
    dss, dsc = float(c["ss"]), float(c["sc"])
    return {"share": dU / float(units_sum),
            "mean_x": (float(ax) + mx + 0.5) / xy_scale, "mean_y": (float(ay) + my + 0.5) / xy_scale,
            "var_x": (float(rxx) / dU - mx * mx) / (xy_scale * xy_scale), "var_y": (float(ryy) / dU - my * my) / (xy_scale * xy_scale),
            "cov_xy": (float(rxy) / dU - mx * my) / (xy_scale * xy_scale),
            "theta": math.atan2(dss, dsc), "theta_resultant": math.hypot(dss, dsc) / (dU * 1048576.0)}
