"""The model of the wide correlative scan match (bl_scanmatch_match_wide, include/botlab_hip.h): the definition of
tests/scan_match_model.py without the +-64 / +-180 limits, the pooled map, the block bounds, and a pruned matcher that must return
what the exhaustive one returns.  Plain numpy; float32 step by step as the existing model (the endpoints are its own)."""
import numpy as np

import scan_match_model as sm

F32 = np.float32
MAX_N, MAX_NTHETA, MAX_RAYS = 4096, 720, 4096
INT32_MAX = 2 ** 31 - 1


def saturate(n):
    """`ties` as the result struct carries it."""
    return min(int(n), INT32_MAX)


def check_params(nx, ny, ntheta, dtheta):
    return 0 <= nx <= MAX_N and 0 <= ny <= MAX_N and 0 <= ntheta <= MAX_NTHETA and F32(dtheta) > 0


def _finish(centre, mpc, dtheta, di, dj, dk, top, ties, score_centre, rays, min_score, utime):
    accepted = int(top >= min_score)
    if accepted:
        x = F32(float(centre[0]) + di * float(F32(mpc)))
        y = F32(float(centre[1]) + dj * float(F32(mpc)))
        theta = sm.wrap_to_pi(F32(centre[2] + F32(F32(dk) * dtheta)))
    else:
        x, y, theta = centre
    return dict(x=F32(x), y=F32(y), theta=F32(theta), utime=int(utime), di=int(di), dj=int(dj), dk=int(dk), score=int(top),
                score_centre=int(score_centre), ties=saturate(ties), rays_used=int(rays), accepted=accepted)


def _prepare(scan_ranges, scan_thetas, centre, nx, ny, ntheta, dtheta, max_range):
    assert check_params(nx, ny, ntheta, dtheta)
    centre = (F32(centre[0]), F32(centre[1]), F32(centre[2]))
    ranges, thetas = sm.valid_rays(scan_ranges, scan_thetas, max_range)
    assert len(ranges) <= MAX_RAYS
    return F32(dtheta), centre, ranges, thetas


def match_exhaustive(cells, origin, mpc, cpm, scan_ranges, scan_thetas, centre, nx, ny, ntheta, dtheta, max_range, min_score=0,
                     utime=0, keep_volume=False):
    """Every candidate scored (score_volume + best_candidate of the existing model, no window limits)."""
    dtheta, centre, ranges, thetas = _prepare(scan_ranges, scan_thetas, centre, nx, ny, ntheta, dtheta, max_range)
    vol = sm.score_volume(cells, origin, cpm, ranges, thetas, centre, nx, ny, ntheta, dtheta)
    di, dj, dk, top, ties = sm.best_candidate(vol, nx, ny, ntheta)
    out = _finish(centre, mpc, dtheta, di, dj, dk, top, ties, vol[ntheta, ny, nx], len(ranges), min_score, utime)
    if keep_volume:
        out["volume"] = vol
    return out


def pooled(cells, h):
    """M_h with a frame of B - 1 cells to the left and above: M[y + B - 1][x + B - 1] = max P[y .. y+B-1][x .. x+B-1], P the
    positive part of the map and 0 outside the grid; x from -(B-1) to W-1, y from -(B-1) to H-1.  uint8."""
    cells = np.asarray(cells)
    H, W = cells.shape
    B = 1 << h
    P = np.zeros((H + 2 * (B - 1), W + 2 * (B - 1)), dtype=np.uint8)
    P[B - 1:B - 1 + H, B - 1:B - 1 + W] = np.maximum(cells.astype(np.int32), 0).astype(np.uint8)
    A = P[:H + B - 1].copy()                                   # separable: down the rows, then along them
    for t in range(1, B):
        np.maximum(A, P[t:t + H + B - 1], out=A)
    M = A[:, :W + B - 1].copy()
    for t in range(1, B):
        np.maximum(M, A[:, t:t + W + B - 1], out=M)
    return M


def heading_endpoints(cells_shape, origin, cpm, ranges, thetas, centre, dk, dtheta, nx, ny):
    """Endpoint cells of heading dk that some shift of the window brings onto the grid (the others count nothing)."""
    H, W = cells_shape
    ex, ey, has = sm.endpoints(ranges, thetas, centre, dk, dtheta, origin, cpm)
    on = has & (ex >= -nx) & (ex < W + nx) & (ey >= -ny) & (ey < H + ny)
    return ex[on], ey[on]


def block_counts(nx, ny, h):
    B = 1 << h
    return (2 * nx + 1 + B - 1) >> h, (2 * ny + 1 + B - 1) >> h


def _padded(img, pad):
    out = np.zeros((img.shape[0] + 2 * pad[0], img.shape[1] + 2 * pad[1]), dtype=np.uint8)
    out[pad[0]:pad[0] + img.shape[0], pad[1]:pad[1] + img.shape[1]] = img
    return out


def block_bounds(cells, origin, cpm, ranges, thetas, centre, nx, ny, ntheta, dtheta, h):
    """int64 [2 ntheta + 1][nby][nbx]: bound of the block of shifts di in [i0, i0 + B), dj in [j0, j0 + B), i0 = -nx + bi B,
    j0 = -ny + bj B: the sum over the heading's endpoints of M_h[ey + j0][ex + i0]."""
    cells = np.asarray(cells)
    H, W = cells.shape
    B = 1 << h
    nbx, nby = block_counts(nx, ny, h)
    M = pooled(cells, h)
    padx, pady = 2 * nx + 2 * B + 2, 2 * ny + 2 * B + 2
    Mp = _padded(M, (pady, padx))                              # Mp[y + B - 1 + pady][x + B - 1 + padx] = M_h[y][x]
    out = np.zeros((2 * ntheta + 1, nby, nbx), dtype=np.int64)
    for k in range(2 * ntheta + 1):
        ex, ey = heading_endpoints((H, W), origin, cpm, ranges, thetas, centre, k - ntheta, dtheta, nx, ny)
        acc = out[k]
        for x, y in zip(ex.tolist(), ey.tolist()):
            y0, x0 = y - ny + B - 1 + pady, x - nx + B - 1 + padx
            acc += Mp[y0:y0 + nby * B:B, x0:x0 + nbx * B:B]
    return out


def block_maxima(vol, h):
    """[k][bj][bi]: the largest score of each block of an exhaustive volume (edge blocks clipped to the window)."""
    B = 1 << h
    nk, ch, cw = vol.shape
    nby, nbx = (ch + B - 1) >> h, (cw + B - 1) >> h
    pad = np.full((nk, nby * B, nbx * B), -1, dtype=np.int64)
    pad[:, :ch, :cw] = vol
    return pad.reshape(nk, nby, B, nbx, B).max(axis=(2, 4))


class _Scorer:
    """Exact scores of whole blocks from a padded positive map."""

    def __init__(self, cells, origin, cpm, ranges, thetas, centre, nx, ny, ntheta, dtheta, h):
        cells = np.asarray(cells)
        self.shape = cells.shape
        self.args = (origin, cpm, ranges, thetas, centre)
        self.nx, self.ny, self.ntheta, self.dtheta, self.B = nx, ny, ntheta, dtheta, 1 << h
        self.padx, self.pady = 2 * nx + self.B + 2, 2 * ny + self.B + 2
        self.P = _padded(np.maximum(cells.astype(np.int32), 0).astype(np.uint8), (self.pady, self.padx))
        self.ends = {}

    def endpoints(self, k):
        if k not in self.ends:
            origin, cpm, ranges, thetas, centre = self.args
            self.ends[k] = heading_endpoints(self.shape, origin, cpm, ranges, thetas, centre, k - self.ntheta, self.dtheta, self.nx, self.ny)
        return self.ends[k]

    def block(self, k, bj, bi):
        """(scores [dj][di] int64, i0, j0) of the block clipped to the window."""
        B = self.B
        i0, j0 = -self.nx + bi * B, -self.ny + bj * B
        i1, j1 = min(i0 + B - 1, self.nx), min(j0 + B - 1, self.ny)
        ex, ey = self.endpoints(k)
        ys = ey[:, None, None] + np.arange(j0, j1 + 1)[None, :, None] + self.pady
        xs = ex[:, None, None] + np.arange(i0, i1 + 1)[None, None, :] + self.padx
        return self.P[ys, xs].sum(axis=0, dtype=np.int64), i0, j0


def match_pruned(cells, origin, mpc, cpm, scan_ranges, scan_thetas, centre, nx, ny, ntheta, dtheta, max_range, h, min_score=0, utime=0):
    """The pruned form: bounds of all blocks, a threshold L from the exact scores of each heading's best-bounded block and of the
    centre, exact scores of every block with bound >= L.  Returns the result fields plus `blocks`, `kept` (blocks this model
    scored), `kept_min` (blocks whose bound reaches the best score: what any exact single-level pruner must score),
    `candidates`, `candidates_scored`."""
    dtheta, centre, ranges, thetas = _prepare(scan_ranges, scan_thetas, centre, nx, ny, ntheta, dtheta, max_range)
    nk = 2 * ntheta + 1
    candidates = nk * (2 * nx + 1) * (2 * ny + 1)
    bounds = block_bounds(cells, origin, cpm, ranges, thetas, centre, nx, ny, ntheta, dtheta, h)
    nby, nbx = bounds.shape[1:]
    extra = dict(blocks=int(bounds.size), candidates=candidates)
    if bounds.max(initial=0) == 0:
        out = _finish(centre, mpc, dtheta, 0, 0, 0, 0, candidates, 0, len(ranges), min_score, utime)
        out.update(extra, kept=0, kept_min=int(bounds.size), candidates_scored=0)
        return out
    sc = _Scorer(cells, origin, cpm, ranges, thetas, centre, nx, ny, ntheta, dtheta, h)
    ex, ey = sc.endpoints(ntheta)
    score_centre = int(sc.P[ey + sc.pady, ex + sc.padx].sum(dtype=np.int64))
    L = score_centre
    for k in range(nk):
        bj, bi = divmod(int(np.argmax(bounds[k])), nbx)
        L = max(L, int(sc.block(k, bj, bi)[0].max()))
    best = None                                                # (score, -d2, -|dk|, -dk, -dj, -di): the definition's order, as a maximum
    ties, scored, top = 0, 0, -1
    ks, bjs, bis = np.nonzero(bounds >= L)
    for k, bj, bi in zip(ks.tolist(), bjs.tolist(), bis.tolist()):
        s, i0, j0 = sc.block(k, bj, bi)
        scored += s.size
        m = int(s.max())
        if m < top:
            continue
        js, is_ = np.nonzero(s == m)
        if m > top:
            top, ties = m, 0
        ties += len(js)
        dk = k - ntheta
        for j, i in zip(js.tolist(), is_.tolist()):
            di, dj = i0 + i, j0 + j
            key = (m, -(di * di + dj * dj), -abs(dk), -dk, -dj, -di)
            if best is None or key > best:
                best = key
    di, dj, dk = -best[5], -best[4], -best[3]
    out = _finish(centre, mpc, dtheta, di, dj, dk, top, ties, score_centre, len(ranges), min_score, utime)
    out.update(extra, kept=int(len(ks)), kept_min=int((bounds >= top).sum()), candidates_scored=int(scored))
    return out


RESULT_FIELDS = ("x", "y", "theta", "utime", "di", "dj", "dk", "score", "score_centre", "ties", "rays_used", "accepted")


def same_result(a, b):
    """Every field of the result, the pose bit for bit."""
    for f in RESULT_FIELDS:
        va, vb = a[f], b[f]
        if f in ("x", "y", "theta"):
            if F32(va).tobytes() != F32(vb).tobytes():
                return False
        elif int(va) != int(vb):
            return False
    return True
