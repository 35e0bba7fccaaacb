"""The model of the obstacle tracks: a restatement of the definition in include/botlab_hip.h ("obstacle tracks"), which the HIP
kernels of botlab_amd/csrc/bl_obstracks.hip must reproduce value for value: the slots, the blobs, the label of every live cell, the
stats and the composed grid.

Written from the definition, not from the kernels: blobs by flood fill (not union-find), the association by sorting the candidate
pairs (not by rounds).  mutual_best() is the device's procedure on its own; the CPU test holds it against the sort, and the model
takes only the number of rounds from it (a figure of the stats).
"""
import numpy as np

from obstacle_layer_model import ArgError, StateError

MAX_BLOBS, MAX_CELLS, MAX_TRACKS, MAX_HORIZON, MAX_KEEP_CLEAR = 1024, 65536, 256, 64, 64
REFUSED_CELLS, REFUSED_IDS = 1, 2
CONFIRMED, MOVING, MATCHED, BORN = 1, 2, 4, 8
SAT, VMAX, POS_MAX, ID_END = 65535, 1023, 1 << 30, 2 ** 32 - 1
BASE = dict(min_cells=1, max_cells=65536, gate_cells=4, alpha=128, beta=64, confirm_hits=3, max_missed=3, min_speed=16)
PARAM_NAMES = ("min_cells", "max_cells", "gate_cells", "alpha", "beta", "confirm_hits", "max_missed", "min_speed")

TRACK_DTYPE = np.dtype([("id", "<u4"), ("px", "<i4"), ("py", "<i4"), ("vx", "<i4"), ("vy", "<i4"), ("hits", "<i4"), ("missed", "<i4"),
                        ("area", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("flags", "<i4"), ("slot", "<i4")])
BLOB_DTYPE = np.dtype([("sum_x", "<i8"), ("sum_y", "<i8"), ("area", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"),
                       ("cx", "<i4"), ("cy", "<i4"), ("eligible", "<i4"), ("track", "<i4"), ("rep", "<i4")])
STAT_NAMES = ("n", "next_id", "live_cells", "blobs", "eligible", "dropped", "matched", "born", "deleted", "unborn", "tracks", "confirmed",
              "refused", "rounds")


def params_ok(min_cells, max_cells, gate_cells, alpha, beta, confirm_hits, max_missed, min_speed):
    """bl_obstracks_set_params' rule."""
    return (1 <= min_cells <= 65536 and min_cells <= max_cells <= 65536 and 1 <= gate_cells <= 64 and 0 <= alpha <= 256 and
            0 <= beta <= 256 and 1 <= confirm_hits <= 255 and 0 <= max_missed <= 255 and 0 <= min_speed <= 1023)


def flood_blobs(live):
    """(blobs, labels): the 8-connected components of the bool grid `live` by flood fill, in the order in which a row-major scan
    meets them (which is the order of their least flat indices); labels per live cell in row-major order."""
    h, w = live.shape
    lab = -np.ones((h, w), np.int64)
    blobs = []
    ys, xs = np.nonzero(live)
    for y, x in zip(ys.tolist(), xs.tolist()):
        if lab[y, x] >= 0:
            continue
        k = len(blobs)
        lab[y, x] = k
        stack, cells = [(x, y)], []
        while stack:
            cx, cy = stack.pop()
            cells.append((cx, cy))
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    nx, ny = cx + dx, cy + dy
                    if 0 <= nx < w and 0 <= ny < h and live[ny, nx] and lab[ny, nx] < 0:
                        lab[ny, nx] = k
                        stack.append((nx, ny))
        blobs.append(cells)
    return blobs, lab[ys, xs]


def candidate_pairs(preds, cents, gate_cells):
    """[(d2, i, j)] of the pairs within the gate; preds {i: (x, y)}, cents {j: (x, y)}."""
    g2 = (256 * gate_cells) ** 2
    out = []
    for i, (px, py) in preds.items():
        for j, (cx, cy) in cents.items():
            d2 = (cx - px) ** 2 + (cy - py) ** 2
            if d2 <= g2:
                out.append((d2, i, j))
    return out


def greedy(pairs):
    """{i: j}: the pairs in ascending order of (d2, i, j), each accepted when both ends are still free."""
    ti, bj, out = set(), set(), {}
    for d2, i, j in sorted(pairs):
        if i not in ti and j not in bj:
            ti.add(i)
            bj.add(j)
            out[i] = j
    return out


def mutual_best(pairs):
    """({i: j}, rounds): rounds in which every free track takes its least (d2, j), every free blob its least (d2, i) and the mutual
    pairs are accepted, until a round accepts none."""
    out, rounds = {}, 0
    left = list(pairs)
    while True:
        tb, bb = {}, {}
        for d2, i, j in left:
            if i not in tb or (d2, j) < tb[i]:
                tb[i] = (d2, j)
            if j not in bb or (d2, i) < bb[j]:
                bb[j] = (d2, i)
        acc = {i: j for i, (d2, j) in tb.items() if bb[j][1] == i}
        if not acc:
            return out, rounds
        out.update(acc)
        rounds += 1
        js = set(acc.values())
        left = [(d2, i, j) for d2, i, j in left if i not in acc and j not in js]


def clamp(v, lo, hi):
    return lo if v < lo else hi if v > hi else v


def stamp_offset(s, v):
    """floor((s v + 512) / 1024)"""
    return (s * v + 512) >> 10


class Tracker:
    def __init__(self, width, height, **params):
        self.w, self.h = int(width), int(height)
        p = dict(BASE, **params)
        assert params_ok(**p)
        self.p = p
        self.reset()

    def set_params(self, **p):
        """False (and nothing changes) when refused."""
        if not params_ok(**p):
            return False
        self.p = dict(p)
        return True

    def _forget_blobs(self, live_cells=0):
        self.blobs = np.zeros(0, BLOB_DTYPE)
        self.labels = -np.ones(min(live_cells, MAX_CELLS), np.int32)
        self.live_xy = np.zeros((0, 2), np.int32)
        self.st = dict.fromkeys(STAT_NAMES, 0)
        self.st["live_cells"] = live_cells

    def reset(self):
        self.slots = np.zeros(MAX_TRACKS, TRACK_DTYPE)
        self.slots["slot"] = np.arange(MAX_TRACKS)
        self.next_id, self.n, self.fresh = 1, 0, True
        self._forget_blobs()

    def download(self):
        return self.slots.copy(), dict(n=self.n, next_id=self.next_id, fresh=int(self.fresh))

    def upload(self, slots, n, next_id, fresh):
        slots = np.array(slots, dtype=TRACK_DTYPE)
        if slots.shape != (MAX_TRACKS,) or next_id < 1:
            raise ArgError("state")
        occ = slots[slots["id"] != 0]
        if (np.any(occ["id"] >= next_id) or len(set(occ["id"].tolist())) != len(occ) or np.any(np.abs(occ["vx"]) > VMAX) or
                np.any(np.abs(occ["vy"]) > VMAX) or np.any(np.abs(occ["px"].astype(np.int64)) > POS_MAX) or
                np.any(np.abs(occ["py"].astype(np.int64)) > POS_MAX) or np.any(occ["hits"] < 1) or np.any(occ["hits"] > SAT) or
                np.any(occ["missed"] < 0) or np.any(occ["missed"] > 255)):
            raise ArgError("slot")
        slots[slots["id"] == 0] = 0
        slots["slot"] = np.arange(MAX_TRACKS)
        self.slots, self.next_id, self.n, self.fresh = slots, int(next_id), int(n), bool(fresh)
        self._forget_blobs()
        self.st["tracks"] = len(occ)
        self.st["confirmed"] = int(np.count_nonzero(occ["flags"] & CONFIRMED))

    def _refuse(self, code, live_cells):
        occ = self.slots[self.slots["id"] != 0]
        self._forget_blobs(live_cells)
        self.st.update(refused=code, tracks=len(occ), confirmed=int(np.count_nonzero(occ["flags"] & CONFIRMED)))

    def update(self, live, layer_n, info=None):
        """One bl_obstracks_update with the layer's live(c) and its counter.  StateError: the order of calls."""
        live = np.asarray(live, bool)
        assert live.shape == (self.h, self.w)
        if not self.fresh and layer_n != (self.n + 1) & 0xFFFFFFFF:
            raise StateError("order")
        self.n, self.fresh = int(layer_n), False
        p = self.p
        L = int(live.sum())
        if L > MAX_CELLS:
            return self._refuse(REFUSED_CELLS, L)
        comps, labels = flood_blobs(live)
        kept = comps[:MAX_BLOBS]
        blobs = np.zeros(len(kept), BLOB_DTYPE)
        for j, cells in enumerate(kept):
            xs, ys = [c[0] for c in cells], [c[1] for c in cells]
            A, sx, sy = len(cells), sum(xs), sum(ys)
            blobs[j] = (sx, sy, A, min(xs), min(ys), max(xs), max(ys), (256 * sx) // A + 128, (256 * sy) // A + 128,
                        int(p["min_cells"] <= A <= p["max_cells"]), -1, min(y * self.w + x for x, y in cells))
        # ---- association
        slots = self.slots.copy()
        occupied = [i for i in range(MAX_TRACKS) if slots["id"][i] != 0]
        preds = {i: (int(slots["px"][i]) + int(slots["vx"][i]), int(slots["py"][i]) + int(slots["vy"][i])) for i in occupied}
        cents = {j: (int(blobs["cx"][j]), int(blobs["cy"][j])) for j in range(len(blobs)) if blobs["eligible"][j]}
        pairs = candidate_pairs(preds, cents, p["gate_cells"])
        match = greedy(pairs)
        rounds = mutual_best(pairs)[1]
        # ---- transition
        deleted = 0
        for i in occupied:
            t = slots[i]
            px, py = preds[i]
            if i in match:
                b = blobs[match[i]]
                rx, ry = int(b["cx"]) - px, int(b["cy"]) - py
                t["px"], t["py"] = px + ((p["alpha"] * rx) >> 8), py + ((p["alpha"] * ry) >> 8)
                t["vx"] = clamp(int(t["vx"]) + ((p["beta"] * rx) >> 8), -VMAX, VMAX)
                t["vy"] = clamp(int(t["vy"]) + ((p["beta"] * ry) >> 8), -VMAX, VMAX)
                t["hits"], t["missed"] = min(int(t["hits"]) + 1, SAT), 0
                for k in ("area", "x0", "y0", "x1", "y1"):
                    t[k] = b[k]
                t["flags"] = MATCHED
                blobs["track"][match[i]] = i
            else:
                t["px"], t["py"] = px, py
                t["missed"] = min(int(t["missed"]) + 1, SAT)
                t["flags"] = 0
                if t["missed"] > p["max_missed"]:
                    slots[i] = 0
                    deleted += 1
        matched_blobs = set(match.values())
        wanted = [j for j in sorted(cents) if j not in matched_blobs]
        free = [i for i in range(MAX_TRACKS) if slots["id"][i] == 0]
        nb = min(len(wanted), len(free))
        if nb > 0 and self.next_id + nb - 1 >= ID_END:
            return self._refuse(REFUSED_IDS, L)
        for k in range(nb):
            j, i = wanted[k], free[k]
            b = blobs[j]
            slots[i] = (self.next_id + k, b["cx"], b["cy"], 0, 0, 1, 0, b["area"], b["x0"], b["y0"], b["x1"], b["y1"], BORN, i)
            blobs["track"][j] = i
        for i in range(MAX_TRACKS):
            t = slots[i]
            t["slot"] = i
            if t["id"] != 0:
                if t["hits"] >= p["confirm_hits"]:
                    t["flags"] |= CONFIRMED
                if int(t["vx"]) ** 2 + int(t["vy"]) ** 2 >= p["min_speed"] ** 2:
                    t["flags"] |= MOVING
        self.slots, self.blobs = slots, blobs
        self.next_id += nb
        self.labels = np.where(labels < MAX_BLOBS, labels, -1).astype(np.int32)
        ys, xs = np.nonzero(live)
        self.live_xy = np.stack([xs, ys], axis=1).astype(np.int32)
        occ = slots[slots["id"] != 0]
        self.st = dict(n=0, next_id=0, live_cells=L, blobs=len(comps), eligible=len(cents), dropped=len(comps) - len(kept), matched=len(match),
                       born=nb, deleted=deleted, unborn=len(wanted) - nb, tracks=len(occ),
                       confirmed=int(np.count_nonzero(occ["flags"] & CONFIRMED)), refused=0, rounds=rounds)
        if info is not None:
            info.update(pairs=pairs, match=match, rounds=rounds, preds=preds, cents=cents, wanted=wanted, free=free)

    def tracks(self):
        return self.slots[self.slots["id"] != 0].copy()

    def stats(self):
        return dict(self.st, n=self.n, next_id=self.next_id)

    def compose(self, layer_live, layer_n, cells, horizon, robot=(0, 0), keep_clear=-1):
        """bl_obstracks_compose: `layer_live` is the layer's live(c) now (what bl_obslayer_compose paints)."""
        if not (0 <= horizon <= MAX_HORIZON and -1 <= keep_clear <= MAX_KEEP_CLEAR):
            raise ArgError("compose")
        if horizon > 0 and not self.fresh and layer_n != self.n:
            raise StateError("order")
        out = np.array(cells, dtype=np.int8)
        out[np.asarray(layer_live, bool)] = 127
        want = CONFIRMED | MOVING
        for (x, y), lab in zip(self.live_xy.tolist(), self.labels.tolist()):
            if horizon == 0 or lab < 0 or self.blobs["track"][lab] < 0:
                continue
            t = self.slots[self.blobs["track"][lab]]
            if (int(t["flags"]) & want) != want:
                continue
            for s in range(1, 4 * horizon + 1):
                sx, sy = x + stamp_offset(s, int(t["vx"])), y + stamp_offset(s, int(t["vy"]))
                if not (0 <= sx < self.w and 0 <= sy < self.h):
                    continue
                if keep_clear >= 0 and abs(sx - robot[0]) <= keep_clear and abs(sy - robot[1]) <= keep_clear:
                    continue
                out[sy, sx] = 127
        return out


def track_metric(track, origin, mpc, scan_period):
    """(x, y, vx, vy) in metres and m/s of a track record: what botlab_amd.host.track_to_metric computes, in double."""
    return (float(origin[0]) + int(track["px"]) / 256.0 * float(mpc), float(origin[1]) + int(track["py"]) / 256.0 * float(mpc),
            int(track["vx"]) / 256.0 * float(mpc) / float(scan_period), int(track["vy"]) / 256.0 * float(mpc) / float(scan_period))
