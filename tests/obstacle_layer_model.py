"""The model of the obstacle layer: a numpy restatement of the definition in include/botlab_hip.h ("obstacle layer"), which the HIP
kernels of botlab_amd/csrc/bl_obslayer.hip must reproduce value for value: the class of every ray, count, last and n of the state,
the stats, the list of live cells and the composed grid.

The geometry is the scan matcher's at heading step 0 (scan_match_model.endpoints with dk = 0, grid_position); the walk is the
reference's Bresenham variant in its closed form (tests/test_mapray_header_cpu.py), start cell included, end cell excluded.
"""
import math

import numpy as np

from scan_match_model import MIN_RANGE, MAX_RAYS, endpoints, grid_position

F32 = np.float32
OFF, EXPLAINED, NOVEL, THROUGH, OUTSIDE = 0, 1, 2, 3, 4
MAX_REACH_CELLS = 4096
N_END = 2 ** 32 - 1


class ArgError(Exception):
    """What the library answers with BL_ERR_ARG."""


class StateError(Exception):
    """What the library answers with BL_ERR_STATE."""


def params_ok(max_range, occ_min, tol_cells, ttl_scans, min_hits):
    """bl_obslayer_set_params' rule."""
    mr = float(F32(max_range))
    return (math.isfinite(mr) and F32(max_range) > MIN_RANGE and 1 <= occ_min <= 127 and 0 <= tol_cells <= 16 and
            1 <= ttl_scans <= 65535 and 1 <= min_hits <= 255)


def walk_loop(x0, y0, x1, y1):
    """The reference's loop itself (mapping.cpp:101-127), end cell excluded: what walk() is the closed form of."""
    dx, dy = abs(x1 - x0), abs(y1 - y0)
    sx, sy = (1 if x0 < x1 else -1), (1 if y0 < y1 else -1)
    err, x, y, out = dx - dy, x0, y0, []
    while x != x1 or y != y1:
        out.append((x, y))
        e2 = 2 * err
        if e2 >= -dy:
            err -= dy
            x += sx
        if e2 <= dx:
            err += dx
            y += sy
    return out


def walk(x0, y0, x1, y1):
    """(xs, ys) of cells k = 0 .. K - 1, K = max(|dx|, |dy|): the major axis advances k, the minor floor((2 k dmin + dmaj) / (2 dmaj))."""
    dx, dy = abs(x1 - x0), abs(y1 - y0)
    sx, sy = (1 if x0 < x1 else -1), (1 if y0 < y1 else -1)
    K = max(dx, dy)
    k = np.arange(K, dtype=np.int64)
    if K == 0:
        return k, k
    if dx >= dy:
        return x0 + sx * k, y0 + sy * ((2 * k * dy + dx) // (2 * dx))
    return x0 + sx * ((2 * k * dx + dy) // (2 * dy)), y0 + sy * k


class Layer:
    def __init__(self, width, height, max_range=5.0, occ_min=1, tol_cells=1, ttl_scans=50, min_hits=1):
        self.w, self.h = int(width), int(height)
        assert params_ok(max_range, occ_min, tol_cells, ttl_scans, min_hits)
        self.max_range, self.occ_min, self.tol, self.ttl, self.min_hits = F32(max_range), int(occ_min), int(tol_cells), int(ttl_scans), int(min_hits)
        self.reset()

    def set_params(self, max_range, occ_min, tol_cells, ttl_scans, min_hits):
        """False (and nothing changes) when refused."""
        if not params_ok(max_range, occ_min, tol_cells, ttl_scans, min_hits):
            return False
        self.max_range, self.occ_min, self.tol, self.ttl, self.min_hits = F32(max_range), int(occ_min), int(tol_cells), int(ttl_scans), int(min_hits)
        return True

    def reset(self):
        self.count = np.zeros((self.h, self.w), np.uint8)
        self.last = np.zeros((self.h, self.w), np.uint32)
        self.n = 0
        self.classes = np.zeros(0, np.uint8)
        self.valid = 0
        self.hs = 0
        self.clr = 0

    def upload(self, count, last, n):
        self.count = np.array(count, dtype=np.uint8).reshape(self.h, self.w)
        self.last = np.array(last, dtype=np.uint32).reshape(self.h, self.w)
        self.n = int(n)
        self.hs = self.clr = 0                                   # the sets belong to an update

    def update(self, cells, origin, cpm, ranges, thetas, pose, info=None):
        """One bl_obslayer_update.  Returns the classes (uint8, one per ray of the scan).  info, a dict, receives per ray 'first', 'K',
        's', 'e' and the sets 'C', 'Hs' (as sets of (x, y))."""
        cells = np.asarray(cells)
        if cells.shape != (self.h, self.w):
            raise ArgError("shape")
        ranges = np.asarray(ranges, dtype=np.float32)
        thetas = np.asarray(thetas, dtype=np.float32)
        if math.ceil(float(self.max_range) * float(F32(cpm))) > MAX_REACH_CELLS:
            raise ArgError("reach")
        with np.errstate(invalid="ignore"):
            keep = (ranges > MIN_RANGE) & (ranges < self.max_range)
        if int(keep.sum()) > MAX_RAYS:
            raise ArgError("rays")
        pose = (F32(pose[0]), F32(pose[1]), F32(pose[2]))
        if not all(math.isfinite(float(v)) for v in pose):
            raise ArgError("pose")
        if self.n == N_END:
            raise StateError("counter")
        self.n += 1
        n = self.n
        occ = cells >= self.occ_min
        ex, ey, has = endpoints(ranges[keep], thetas[keep], pose, 0, F32(0), origin, cpm)
        sxf, syf = grid_position(pose[0], pose[1], origin, F32(cpm))
        idx = np.nonzero(keep)[0]
        classes = np.zeros(len(ranges), np.uint8)
        C, Hs = set(), set()
        per_ray = []
        t = self.tol
        for j, r in enumerate(idx.tolist()):
            if not has[j]:
                continue
            s = (int(np.trunc(sxf)), int(np.trunc(syf)))
            e = (int(ex[j]), int(ey[j]))
            xs, ys = walk(s[0], s[1], e[0], e[1])
            K = len(xs)
            inside = (xs >= 0) & (xs < self.w) & (ys >= 0) & (ys < self.h)
            hit = np.zeros(K, bool)
            hit[inside] = occ[ys[inside], xs[inside]]
            first = int(np.argmax(hit)) if hit.any() else K
            x0, x1, y0, y1 = max(e[0] - t, 0), min(e[0] + t, self.w - 1), max(e[1] - t, 0), min(e[1] + t, self.h - 1)
            explained = x0 <= x1 and y0 <= y1 and bool(occ[y0:y1 + 1, x0:x1 + 1].any())
            e_in = 0 <= e[0] < self.w and 0 <= e[1] < self.h
            c = EXPLAINED if explained else THROUGH if first < K else NOVEL if e_in else OUTSIDE
            classes[r] = c
            if c != THROUGH:
                m = inside & (np.arange(K) < first)
                C.update(zip(xs[m].tolist(), ys[m].tolist()))
            if c == NOVEL:
                Hs.add(e)
            per_ray.append(dict(ray=r, s=s, e=e, K=K, first=first, cls=c))
        for (x, y) in Hs:
            l = int(self.last[y, x])
            fresh = l != 0 and ((n - l) & 0xFFFFFFFF) < self.ttl
            self.count[y, x] = min(int(self.count[y, x]) + 1, 255) if fresh else 1
            self.last[y, x] = n
        for (x, y) in C - Hs:
            self.count[y, x] = 0
            self.last[y, x] = 0
        self.classes, self.valid, self.hs, self.clr = classes, int(keep.sum()), len(Hs), len(C - Hs)
        if info is not None:
            info.update(rays=per_ray, C=C, Hs=Hs)
        return classes

    def live(self):
        last = self.last.astype(np.int64)
        return (self.count >= self.min_hits) & (last != 0) & (((self.n - last) & 0xFFFFFFFF) < self.ttl)    # uint32 arithmetic

    def live_cells(self):
        """int32 [m][2] of (x, y), row-major."""
        ys, xs = np.nonzero(self.live())
        return np.stack([xs, ys], axis=1).astype(np.int32)

    def compose(self, cells):
        out = np.array(cells, dtype=np.int8)
        out[self.live()] = 127
        return out

    def stats(self):
        return dict(n=self.n, valid=self.valid, classes=[int((self.classes == c).sum()) for c in range(5)], hs=self.hs, clr=self.clr,
                    live=int(self.live().sum()))
