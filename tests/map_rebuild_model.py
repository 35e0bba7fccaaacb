"""The model of the map rebuild (bl_scanlog_rebuild, include/botlab_hip.h).  TEST INFRASTRUCTURE, no GPU.

Two things live here:

  truth()   the definition: a fresh OracleMapping, primed with prev_pose by one throw-away update on a scratch grid (as
            tests/rb_slam_model.py does), then one OracleMapping.update per scan, in order, on a copy of the base.
  fold()    a restatement of what the kernels do: the rays' cells, each scan's box clipped to the grid, chunks of CHUNK consecutive
            scans, the (tile, chunk) pairs whose boxes meet, per pair the composed clamped add (a, lo, hi) of every cell with `a`
            saturated to +-255, and the pairs of a tile applied in chunk order to the base cell.  It must equal truth() byte for byte.

naive() is the rule the kernels must NOT implement: all the scans' adds summed, clamped once.  The tests count where it differs."""
import numpy as np

import oracle_lib

TILE = 64                 # RL_TILE
CHUNK = 16                # RL_CHUNK
MAX_CHUNKS = 4096         # RL_MAX_CHUNKS
CELL_LIMIT = 1 << 24      # RL_CELL_LIMIT
MIN_RANGE = np.float32(0.15)
IDENTITY = (0, -128, 127)


# ---------------------------------------------------------------- the clamped add and its composition (scalars or numpy arrays)
def f_apply(f, v):
    a, lo, hi = f
    return np.maximum(lo, np.minimum(hi, v + a))


def f_then(f1, f2):
    """f2 o f1 = (a1 + a2 saturated to +-255, f2(lo1), f2(hi1))."""
    a = np.clip(f1[0] + f2[0], -255, 255)
    return (a, f_apply(f2, f1[1]), f_apply(f2, f1[2]))


def f_scan(f, H, M, hit, miss):
    """One scan on top of f: H hits, then M misses, each pass one clamped add with its add saturated to 255 (rl_compose_scan)."""
    up = np.minimum(255, hit * H)
    down = np.minimum(255, miss * M)
    f = f_then(f, (up, -128, 127))
    return f_then(f, (-down, -128, 127))


def sequential(v, seq, hit, miss):
    """The reference's rule for one cell: per scan all hits, then all misses, each step saturating (mapping.cpp:73-99)."""
    v = np.asarray(v, np.int64).copy()
    for H, M in seq:
        v = np.minimum(127, v + hit * H)
        v = np.maximum(-128, v - miss * M)
    return v


def sum_then_clamp(v, seq, hit, miss):
    total = sum(hit * H - miss * M for H, M in seq)
    return np.clip(np.asarray(v, np.int64) + total, -128, 127)


# ---------------------------------------------------------------- geometry
def ray_cells(orc, scan, begin, end, origin, cpm, max_laser):
    """(n, 4) int64 start and end cells of the rays the map update traces: the oracle's moving scan, mapping.cpp:45-49 in float32 with
    the oracle's own cosf / sinf, and the kernels' 2^24 limit."""
    rays = orc.moving_scan(scan, begin, end)
    rays = rays[rays[:, 2] <= np.float32(max_laser)]
    if len(rays) == 0:
        return np.zeros((0, 4), np.int64)
    cpm = np.float32(cpm)
    sx = ((rays[:, 0].astype(np.float64) - np.float64(np.float32(origin[0]))) * np.float64(cpm)).astype(np.float32)
    sy = ((rays[:, 1].astype(np.float64) - np.float64(np.float32(origin[1]))) * np.float64(cpm)).astype(np.float32)
    cs = np.array([orc.lib.orc_cosf(float(t)) for t in rays[:, 3]], np.float32)
    sn = np.array([orc.lib.orc_sinf(float(t)) for t in rays[:, 3]], np.float32)
    fx = ((rays[:, 2] * cs).astype(np.float32) * cpm).astype(np.float32) + sx
    fy = ((rays[:, 2] * sn).astype(np.float32) * cpm).astype(np.float32) + sy
    lim = np.float32(CELL_LIMIT)
    ok = (np.abs(fx) < lim) & (np.abs(fy) < lim) & (np.abs(sx) < lim) & (np.abs(sy) < lim)
    c = np.stack([np.trunc(sx[ok]), np.trunc(sy[ok]), np.trunc(fx[ok]), np.trunc(fy[ok])], axis=1)
    return c.astype(np.int64)


def walk_cells(x0, y0, x1, y1):
    """The cells of Mapping::bresenham from (x0, y0) to (x1, y1), start included, end excluded, by the closed form the kernels use:
    the major axis advances k, the minor axis floor((2 k dmin + dmaj) / (2 dmaj))."""
    dx, dy = abs(x1 - x0), abs(y1 - y0)
    K = max(dx, dy)
    k = np.arange(K, dtype=np.int64)
    sx, sy = (1 if x0 < x1 else -1), (1 if y0 < y1 else -1)
    if dx >= dy:
        return x0 + sx * k, y0 + sy * ((2 * k * dy + dx) // (2 * dx) if dx else k)
    return x0 + sx * ((2 * k * dx + dy) // (2 * dy)), y0 + sy * k


_counts = {}


def scan_counts(cells, W, H):
    """(hits, misses, box): per cell of the W x H grid how many rays end there and how many cross it, and the box of all start and end
    cells clipped to the grid ((x0, y0, x1, y1), or None when it is empty)."""
    key = (W, H, cells.tobytes())
    if key in _counts:
        return _counts[key]
    hits, misses = np.zeros((H, W), np.int64), np.zeros((H, W), np.int64)
    box = None
    if len(cells):
        x0, x1 = max(int(min(cells[:, 0].min(), cells[:, 2].min())), 0), min(int(max(cells[:, 0].max(), cells[:, 2].max())), W - 1)
        y0, y1 = max(int(min(cells[:, 1].min(), cells[:, 3].min())), 0), min(int(max(cells[:, 1].max(), cells[:, 3].max())), H - 1)
        if x0 <= x1 and y0 <= y1:
            box = (x0, y0, x1, y1)
    if box is not None:
        e = cells[(cells[:, 2] >= 0) & (cells[:, 2] < W) & (cells[:, 3] >= 0) & (cells[:, 3] < H)]
        np.add.at(hits, (e[:, 3], e[:, 2]), 1)
        uniq, mult = np.unique(cells, axis=0, return_counts=True)
        for (a, b, c, d), m in zip(uniq.tolist(), mult.tolist()):
            x, y = walk_cells(a, b, c, d)
            ok = (x >= 0) & (x < W) & (y >= 0) & (y < H)
            np.add.at(misses, (y[ok], x[ok]), m)
    _counts[key] = (hits, misses, box)
    return _counts[key]


# ---------------------------------------------------------------- the definition and the restatement
def _opose(orc, p):
    return orc.pose(p[0], p[1], p[2], utime=p[3])


def steps(scans, poses, prev):
    """[(scan, begin, end)] of the updates that change cells: with prev None the first scan only latches its pose."""
    out, before = [], prev
    for s, p in zip(scans, poses):
        if before is not None:
            out.append((s, before, p))
        before = p
    return out


def truth(orc, scans, poses, prev, base, mpc, cpm, origin, max_laser, hit, miss):
    """scans: LidarScan list; poses: (x, y, theta, utime) list; prev: one more or None; base: (H, W) int8.  The rebuilt cells."""
    om = oracle_lib.OracleMapping(orc, max_laser, hit, miss)
    ref = np.ascontiguousarray(base, np.int8).copy()
    if prev is not None:
        om.update(scans[0], _opose(orc, prev), np.zeros_like(ref), mpc, cpm, origin)      # latches prev; changes no cell
    for s, p in zip(scans, poses):
        om.update(s, _opose(orc, p), ref, mpc, cpm, origin)
    return ref


def chunk_size(n):
    c = CHUNK
    if -(-n // c) > MAX_CHUNKS:
        c = -(-n // MAX_CHUNKS)
    return c


def _meets(box, tx0, ty0, tx1, ty1):
    return box is not None and box[0] <= tx1 and box[2] >= tx0 and box[1] <= ty1 and box[3] >= ty0


def fold(orc, scans, poses, prev, base, mpc, cpm, origin, max_laser, hit, miss):
    """(cells, info): the kernels' computation restated; info: scans, chunk_scans, chunks, tiles, pairs [(tile, chunk)], per_scan
    [(hits, misses, box)]."""
    base = np.ascontiguousarray(base, np.int8)
    H, W = base.shape
    per = [scan_counts(ray_cells(orc, s, _opose(orc, b), _opose(orc, e), origin, cpm, max_laser), W, H) for s, b, e in steps(scans, poses, prev)]
    n = len(per)
    C = chunk_size(n)
    nchunks = -(-n // C)
    cboxes = []
    for c in range(nchunks):
        u = None
        for _, _, b in per[c * C:(c + 1) * C]:
            if b is not None:
                u = b if u is None else (min(u[0], b[0]), min(u[1], b[1]), max(u[2], b[2]), max(u[3], b[3]))
        cboxes.append(u)
    ntx, nty = -(-W // TILE), -(-H // TILE)
    out = base.astype(np.int64)
    pairs = []
    for t in range(ntx * nty):
        tx0, ty0 = (t % ntx) * TILE, (t // ntx) * TILE
        tx1, ty1 = min(tx0 + TILE, W) - 1, min(ty0 + TILE, H) - 1
        sl = (slice(ty0, ty1 + 1), slice(tx0, tx1 + 1))
        for c in range(nchunks):
            if not _meets(cboxes[c], tx0, ty0, tx1, ty1):
                continue
            pairs.append((t, c))
            shape = out[sl].shape
            f = (np.zeros(shape, np.int64), np.full(shape, -128, np.int64), np.full(shape, 127, np.int64))
            for hits, misses, b in per[c * C:(c + 1) * C]:
                if _meets(b, tx0, ty0, tx1, ty1):
                    f = f_scan(f, hits[sl], misses[sl], hit, miss)
            assert (np.abs(f[0]) <= 255).all() and (f[1] <= f[2]).all()            # fits int16, int8, int8
            out[sl] = f_apply(f, out[sl])                   # pairs of a tile in chunk order
    return out.astype(np.int8), dict(scans=n, chunk_scans=C, chunks=nchunks, tiles=ntx * nty, pairs=pairs, per_scan=per)


def naive(base, per_scan, hit, miss):
    """Sum-then-clamp: what the result would be if the scans' adds were summed and clamped once."""
    total = np.zeros(base.shape, np.int64)
    for hits, misses, _ in per_scan:
        total += hit * hits - miss * misses
    return np.clip(base.astype(np.int64) + total, -128, 127).astype(np.int8)
