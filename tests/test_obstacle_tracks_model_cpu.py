"""The obstacle tracks' model (tests/obstacle_tracks_model.py) on its own: every condition of the definition reached at least once
(each printed as a count; a count of 0 fails).  The GPU tests run the scripts built here on the device and compare every step with
the model."""
import collections
import functools

import numpy as np

import obstacle_layer_model as om
import obstacle_tracks_model as tm
from test_obstacle_layer_model_cpu import CPM, MPC, ORIGIN

F32 = np.float32
SIZES = ((37, 23), (64, 64), (131, 67))
LAYER = dict(max_range=5.0, occ_min=1, tol_cells=1, ttl_scans=50, min_hits=1)


# ---------------------------------------------------------------------------------------------------------------- scripts
class Script:
    """A map, a layer, a tracker and a list of steps that the model and the device both run:
    ("layer", count, last, n)  bl_obslayer_upload          ("scan", ranges, thetas, pose)  bl_obslayer_update
    ("layer_reset",)                                         ("update",)  bl_obstracks_update
    ("compose", horizon, (rx, ry), keep_clear)               ("params", dict)  ("reset",)
    ("upload", slots, n, next_id, fresh)                     ("roundtrip",)  download, then upload of what came back"""

    def __init__(self, w, h, cells=None, layer=None, **params):
        if cells is None:
            cells = np.full((h, w), -100, np.int8)
            cells[h // 2, 1:4] = 100
            cells[0, w - 1] = 55
        self.cells = np.ascontiguousarray(cells, np.int8)
        self.origin, self.mpc, self.cpm = ORIGIN, MPC, CPM
        self.layer = dict(LAYER, **(layer or {}))
        self.params = dict(tm.BASE, **params)
        self.steps = []
        self.n = 0

    @property
    def shape(self):
        return self.cells.shape[1], self.cells.shape[0]

    def live(self, mask, n=None):
        """The layer's state replaced so that exactly `mask` is live, at counter n (the last one + 1 when None)."""
        self.n = self.n + 1 if n is None else n
        mask = np.asarray(mask, bool)
        self.steps.append(("layer", mask.astype(np.uint8), np.where(mask, self.n, 0).astype(np.uint32), self.n))

    def frame(self, mask, n=None):
        self.live(mask, n)
        self.steps.append(("update",))

    def cells_frame(self, xy, n=None):
        w, h = self.shape
        m = np.zeros((h, w), bool)
        for x, y in xy:
            m[y, x] = True
        self.frame(m, n)

    def add(self, *step):
        self.steps.append(tuple(step))

    def upload(self, tracks, next_id=None, fresh=0, n=None):
        """tracks: {slot: record dict}"""
        slots = np.zeros(tm.MAX_TRACKS, tm.TRACK_DTYPE)
        for i, t in tracks.items():
            for k, v in t.items():
                slots[k][i] = v
        if next_id is None:
            next_id = max([int(t["id"]) for t in tracks.values()] + [0]) + 1
        self.steps.append(("upload", slots, self.n if n is None else n, next_id, fresh))


def trk(tid, cx, cy, vx=0, vy=0, hits=5, ox=0, oy=0, missed=0, flags=0):
    """A slot whose position is the middle of cell (cx, cy) plus (ox, oy) in 1/256 cell."""
    return dict(id=tid, px=256 * cx + 128 + ox, py=256 * cy + 128 + oy, vx=vx, vy=vy, hits=hits, missed=missed, flags=flags)


def run_model(script, infos=None):
    """The model over a script: per step (outcome, snapshot); outcome "ok", "arg" or "state"."""
    w, h = script.shape
    layer = om.Layer(w, h, **script.layer)
    tr = tm.Tracker(w, h, **script.params)
    out = []
    for st in script.steps:
        res, composed = "ok", None
        try:
            if st[0] == "layer":
                layer.upload(st[1], st[2], st[3])
            elif st[0] == "scan":
                layer.update(script.cells, script.origin, script.cpm, st[1], st[2], st[3])
            elif st[0] == "layer_reset":
                layer.reset()
            elif st[0] == "update":
                info = {}
                tr.update(layer.live(), layer.n, info)
                if infos is not None:
                    infos.append(info)
            elif st[0] == "compose":
                composed = tr.compose(layer.live(), layer.n, script.cells, st[1], st[2], st[3])
            elif st[0] == "params":
                res = "ok" if tr.set_params(**dict(tr.p, **st[1])) else "arg"
            elif st[0] == "reset":
                tr.reset()
            elif st[0] == "upload":
                tr.upload(st[1], st[2], st[3], st[4])
            elif st[0] == "roundtrip":
                slots, state = tr.download()
                tr.upload(slots, state["n"], state["next_id"], state["fresh"])
            else:
                raise AssertionError(st[0])
        except om.ArgError:
            res = "arg"
        except om.StateError:
            res = "state"
        snap = dict(tracks=tr.tracks(), blobs=tr.blobs.copy(), labels=tr.labels.copy(), stats=tr.stats(), live=layer.live_cells())
        if composed is not None:
            snap["composed"] = composed
            snap["layer_composed"] = layer.compose(script.cells)
        out.append((res, snap))
    return out


# ---------------------------------------------------------------------------------------------------------------- shapes
def spiral(S):
    """A spiral of one-cell width in an S x S box from its corner (0, 0) inwards, one empty cell between the windings."""
    g = np.zeros((S, S), bool)
    x = y = d = turns = 0
    g[0, 0] = True
    dirs = ((1, 0), (0, 1), (-1, 0), (0, -1))
    while turns < 2:
        dx, dy = dirs[d]
        nx, ny, fx, fy = x + dx, y + dy, x + 2 * dx, y + 2 * dy
        if 0 <= nx < S and 0 <= ny < S and not g[ny, nx] and not (0 <= fx < S and 0 <= fy < S and g[fy, fx]):
            x, y, turns = nx, ny, 0
            g[y, x] = True
        else:
            d, turns = (d + 1) % 4, turns + 1
    return g


def links_from_least(cells):
    """The largest number of 8-connected steps by which a cell of the blob is away from the blob's least cell."""
    cells = set(cells)
    start = min(cells, key=lambda c: (c[1], c[0]))
    seen, frontier, depth = {start}, [start], 0
    while frontier:
        nxt = []
        for x, y in frontier:
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    c = (x + dx, y + dy)
                    if c in cells and c not in seen:
                        seen.add(c)
                        nxt.append(c)
        if nxt:
            depth += 1
        frontier = nxt
    assert seen == cells
    return depth


def shapes_script(w, h):
    s = Script(w, h)
    m = np.zeros((h, w), bool)                      # 0: a single cell, and a row of up to 65 cells on the top border
    m[h - 3, w - 2] = True
    m[h - 1, :min(65, w)] = True
    s.frame(m)
    m = np.zeros((h, w), bool)                      # 1: the spiral
    m[1:22, 1:22] = spiral(21)
    s.frame(m)
    m = np.zeros((h, w), bool)                      # 2: checkerboard, ring, diagonal touch, one-cell gap
    yy, xx = np.mgrid[0:17, 0:17]
    m[0:17, 0:17] = (xx + yy) % 2 == 0
    m[0:5, 19:24] = True
    m[1:4, 20:23] = False
    m[7:9, 19:21] = True
    m[9:11, 21:23] = True
    m[0:2, 26:28] = True
    m[0:2, 29:31] = True
    s.frame(m)
    m = np.zeros((h, w), bool)                      # 3: the borders and the corners
    m[h // 2:h // 2 + 2, 0] = True
    m[h // 2 - 1:h // 2 + 1, w - 1] = True
    m[0, w // 2:w // 2 + 2] = True
    m[h - 1, w // 2] = True
    m[0, 0] = m[h - 1, w - 1] = m[0, w - 1] = m[h - 1, 0] = True
    s.frame(m)
    s.add("reset")                                  # 4: a row of five whose middle cell has expired: two blobs
    count = np.zeros((h, w), np.uint8)
    last = np.zeros((h, w), np.uint32)
    count[3, 5:10] = 2
    last[3, 5:10] = 100
    last[3, 7] = 100 - s.layer["ttl_scans"]
    s.n = 100
    s.add("layer", count, last, 100)
    s.add("update")
    return s


def area_script(w, h):
    """min_cells 3, max_cells 6: blobs of 2, 3, 6 and 7 cells."""
    s = Script(w, h, min_cells=3, max_cells=6)
    m = np.zeros((h, w), bool)
    m[2, 2:4] = True
    m[2, 6:9] = True
    m[5:7, 2:5] = True
    m[5:7, 8:11] = True
    m[7, 8] = True
    s.frame(m)
    s.frame(m)
    return s


def caps_script(w, h):
    """Live cells at even x and even y: every one a blob of its own."""
    s = Script(w, h)
    m = np.zeros((h, w), bool)
    m[0::2, 0::2] = True
    s.frame(m)
    s.frame(m)
    s.add("compose", 2, (0, 0), -1)
    return s


# ---------------------------------------------------------------------------------------------------------------- association, filter
def assoc_script(w, h):
    s = Script(w, h, gate_cells=6, alpha=100, beta=77)

    def case(tracks, cells, **params):
        s.add("reset")
        if params:
            s.add("params", params)
        s.upload(tracks, fresh=1)
        s.cells_frame(cells)

    # 0: equal d2 from one track to two blobs, and (further up) from two tracks to one blob
    case({3: trk(1, 10, 10), 5: trk(2, 8, 16), 9: trk(3, 12, 16)}, [(8, 10), (12, 10), (10, 16)], gate_cells=3)
    # 1: d2 exactly (256 gate)^2 and one more
    case({0: trk(1, 10, 4), 1: trk(2, 10, 12, ox=-1)}, [(12, 4), (12, 12)], gate_cells=2)
    # 2: a chain where the greedy choice is not the least total: tracks at x = 10 and 13, blobs at 12 and 15
    case({0: trk(1, 10, 8), 1: trk(2, 13, 8)}, [(12, 8), (15, 8)], gate_cells=6)
    # 3: three rounds: b0 15, t0 16, t1 13, b1 10, t2 6, b2 1
    case({0: trk(1, 16, 8), 1: trk(2, 13, 8), 2: trk(3, 6, 8)}, [(15, 8), (10, 8), (1, 8)])
    # 4: a negative residual whose alpha r is no multiple of 256; the velocity clamp at both signs (beta 256)
    case({0: trk(1, 10, 5, ox=37, oy=-11, vx=-3, vy=2), 1: trk(2, 20, 5, vx=1000, ox=-900), 2: trk(3, 20, 15, vx=-1000, ox=900),
          3: trk(4, 5, 15, hits=tm.SAT)}, [(10, 5), (25, 5), (15, 15), (5, 15)], alpha=101, beta=256)
    # 5, 6: alpha 0 and 256
    case({0: trk(1, 10, 5, ox=37, oy=-11, vx=40, vy=-9)}, [(11, 5)], alpha=0, beta=0)
    case({0: trk(1, 10, 5, ox=37, oy=-11, vx=40, vy=-9)}, [(11, 5)], alpha=256, beta=256)
    return s


# ---------------------------------------------------------------------------------------------------------------- life cycle
def lifecycle_script(w, h):
    s = Script(w, h, confirm_hits=3, max_missed=2, gate_cells=4)
    A = [(5, 5), (6, 5), (5, 6), (6, 6)]
    s.cells_frame(A)                                # 0-1: born, id 1, slot 0
    s.cells_frame(A)                                # 2-3: hits 2
    s.cells_frame(A)                                # 4-5: hits 3: confirmed
    s.cells_frame([(x + 1, y) for x, y in A] + [(20, 15)])   # 6-7: A moves; B born, id 2, slot 1
    s.cells_frame([(20, 15)])                       # 8-9: A coasts, missed 1
    s.cells_frame([(20, 15)])                       # 10-11: missed 2
    s.cells_frame([(20, 15), (30, 5)])              # 12-13: missed 3 > 2: deleted, and C born into the slot that became free, id 3
    s.add("update")                                 # 14: the layer has not moved on
    s.live(np.zeros((h, w), bool))                  # 15, 16: two layer steps
    s.live(np.zeros((h, w), bool))
    s.add("update")                                 # 17: the layer is two ahead
    s.add("compose", 2, (0, 0), -1)                 # 18: and so is it for a compose that stamps
    s.add("compose", 0, (0, 0), -1)                 # 19: but not for one that does not
    s.add("roundtrip")                              # 20
    s.add("reset")                                  # 21
    s.add("update")                                 # 22: fresh: any n
    # the id limit, through upload
    s.upload({2: trk(5, 5, 5)}, next_id=tm.ID_END - 1, fresh=0)          # 23
    s.cells_frame([(5, 5), (20, 15)])               # 24-25: one birth with the last id there is
    s.cells_frame([(5, 5), (20, 15), (30, 5)])      # 26-27: refused on the device: the slots stay
    s.cells_frame([(5, 5), (20, 15)])               # 28-29: fine again
    s.add("roundtrip")                              # 30
    s.cells_frame([(5, 5), (20, 15)])               # 31-32: the same continuation
    # refusals of upload, set_params and compose
    s.upload({0: trk(7, 5, 5)}, next_id=7)
    s.upload({0: trk(1, 5, 5), 1: trk(1, 9, 9)}, next_id=7)
    s.upload({0: trk(1, 5, 5, vx=1024)}, next_id=7)
    s.upload({0: trk(1, 5, 5, hits=0)}, next_id=7)
    s.upload({}, next_id=0)
    s.add("params", dict(min_cells=0))
    s.add("params", dict(max_cells=0))
    s.add("params", dict(gate_cells=65))
    s.add("params", dict(alpha=257))
    s.add("params", dict(min_speed=1024))
    s.add("compose", 65, (0, 0), -1)
    s.add("compose", 1, (0, 0), 65)
    s.cells_frame([(5, 5), (20, 15)])               # and nothing of that changed anything
    return s


# ---------------------------------------------------------------------------------------------------------------- compose
def compose_script(w, h):
    s = Script(w, h, confirm_hits=3, min_speed=64, gate_cells=4, alpha=128, beta=64)
    tracks = {0: trk(1, 10, 10, vx=300, vy=150), 1: trk(2, w - 4, 12, vx=900), 2: trk(3, 3, 5, vx=-700, vy=-200),
              3: trk(4, 15, 3, vy=-800), 4: trk(5, 20, h - 4, vx=100, vy=900), 5: trk(6, 28, 8, vx=500, hits=1),
              6: trk(7, 28, 16, vx=5, vy=5)}
    s.upload(tracks, fresh=1)
    cells = []
    for t in tracks.values():                       # a 2 x 2 blob whose least cell holds the prediction
        x, y = (t["px"] + t["vx"]) >> 8, (t["py"] + t["vy"]) >> 8
        cells += [(x, y), (x + 1, y), (x, y + 1), (x + 1, y + 1)]
    s.cells_frame([(x, y) for x, y in cells if 0 <= x < w and 0 <= y < h])
    # the robot: a cell that track 1's sweep stamps (found with the model)
    model = tm.Tracker(w, h, **s.params)
    model.upload(s.steps[0][1], 0, 8, 1)
    live = s.steps[1][1].astype(bool)
    model.update(live, 1)
    plain = model.compose(live, 1, s.cells, 0)
    swept = model.compose(live, 1, s.cells, 8)
    ys, xs = np.nonzero((swept == 127) & (plain != 127))
    near = [(int(x), int(y)) for x, y in zip(xs, ys) if abs(x - 14) <= 3 and abs(y - 12) <= 3]
    robot = near[0]
    for horizon in (0, 1, 8, 64):
        s.add("compose", horizon, robot, -1)
    for keep in (0, 3, 64):
        s.add("compose", 8, robot, keep)
    s.add("compose", 8, (-5000, 2), 3)
    s.add("compose", 8, (w + 7, h + 2), 10)
    return s


def reversed_scan_scripts(w, h):
    """Two scripts whose scans hold the same rays in opposite orders: the same live set either way."""
    out = []
    for rev in (False, True):
        s = Script(w, h, cells=np.full((h, w), -100, np.int8))
        from test_obstacle_layer_model_cpu import Script as LayerScript
        ls = LayerScript(s.cells)
        pose = ls.pose_at(w // 2 + 0.5, h // 2 + 0.5, 0.3)
        for k in range(3):
            targets = [(w // 2 + 6 + k, h // 2 + dy) for dy in (-1, 0, 1, 2)] + [(w // 2 - 7, h // 2 + 4 + dx) for dx in (0, 1)] + [(4, 3 + k)]
            rays = [ls.ray_to(pose, x, y) for x, y in targets]
            if rev:
                rays = rays[::-1]
            s.add("scan", np.array([r for r, _ in rays], np.float32), np.array([t for _, t in rays], np.float32), pose)
            s.add("update")
            s.add("compose", 4, (w // 2, h // 2), 1)
        out.append(s)
    return out


ALL = (("shapes", shapes_script), ("area", area_script), ("caps", caps_script), ("assoc", assoc_script), ("lifecycle", lifecycle_script),
       ("compose", compose_script))


@functools.lru_cache(maxsize=None)
def model_of(name, w, h):
    """(script, model results, infos), computed once and shared (nobody changes them)."""
    script = dict(ALL)[name](w, h)
    infos = []
    return script, run_model(script, infos), infos


# ---------------------------------------------------------------------------------------------------------------- the conditions
def test_every_condition_is_reached():
    n = collections.Counter()
    for w, h in SIZES:
        # ---- shapes
        s, res, _ = model_of("shapes", w, h)
        assert all(r == "ok" for r, _ in res)
        upd = [snap for st, (_, snap) in zip(s.steps, res) if st[0] == "update"]
        b0 = upd[0]["blobs"]
        n["single cell"] += int(np.count_nonzero(b0["area"] == 1))
        n["65-cell row"] += int(np.count_nonzero((b0["area"] == 65) & (b0["y0"] == b0["y1"])))
        assert len(b0) == 2
        b1 = upd[1]["blobs"]
        assert len(b1) == 1 and b1["rep"][0] == 1 * w + 1
        depth = links_from_least([(int(x), int(y)) for x, y in upd[1]["live"]])
        n["spiral, least cell more than 64 links away"] += int(depth > 64)
        b2 = upd[2]["blobs"]
        assert [int(a) for a in b2["area"]] == [145, 16, 4, 4, 8], b2["area"]
        n["checkerboard 17 x 17 is one blob"] += int(b2["area"][0] == 145)
        n["ring"] += int(b2["area"][1] == 16 and (b2["x0"][1], b2["x1"][1]) == (19, 23))
        n["diagonal touch is one blob"] += int(b2["area"][4] == 8)
        n["one-cell gap is two blobs"] += int(b2["area"][2] == 4 and b2["area"][3] == 4)
        b3 = upd[3]["blobs"]
        n["border blobs"] += int(np.count_nonzero((b3["x0"] == 0) | (b3["y0"] == 0) | (b3["x1"] == w - 1) | (b3["y1"] == h - 1)))
        n["corner blobs"] += int(np.count_nonzero(((b3["x0"] == 0) | (b3["x1"] == w - 1)) & ((b3["y0"] == 0) | (b3["y1"] == h - 1))))
        assert len(b3) == 8
        b4 = upd[4]["blobs"]
        n["split by an expired cell"] += int(len(b4) == 2 and list(b4["area"]) == [2, 2])
        # ---- areas
        s, res, _ = model_of("area", w, h)
        b = res[1][1]["blobs"]
        assert list(b["area"]) == [2, 3, 6, 7] and list(b["eligible"]) == [0, 1, 1, 0]
        n["area min_cells - 1"] += 1
        n["area min_cells"] += 1
        n["area max_cells"] += 1
        n["area max_cells + 1"] += 1
        assert list(b["track"]) == [-1, 0, 1, -1] and res[3][1]["stats"]["matched"] == 2
        # ---- caps
        s, res, _ = model_of("caps", w, h)
        st = res[1][1]["stats"]
        assert st["blobs"] == ((w + 1) // 2) * ((h + 1) // 2)
        if (w, h) == (64, 64):
            assert (st["blobs"], st["dropped"], st["born"], st["unborn"]) == (1024, 0, 256, 768)
            n["exactly 1024 blobs, 256 born, 768 unborn"] += 1
        if (w, h) == (131, 67):
            assert (st["blobs"], st["dropped"]) == (2244, 1220)
            lab = res[1][1]["labels"]
            assert np.array_equal(lab[:1024], np.arange(1024)) and np.all(lab[1024:] == -1)
            n["2244 blobs, 1220 dropped, the first by rank kept"] += 1
        assert res[3][1]["stats"]["matched"] == min(st["blobs"], 256)
        # ---- association and filter
        s, res, infos = model_of("assoc", w, h)
        upd = [snap for st_, (_, snap) in zip(s.steps, res) if st_[0] == "update"]
        for info in infos:                          # the device's procedure gives the sorted greedy choice
            assert tm.mutual_best(info["pairs"])[0] == tm.greedy(info["pairs"])
        p0 = infos[0]["pairs"]
        n["one track, two blobs, equal d2"] += int(len({d for d, i, j in p0 if i == 3}) == 1 and infos[0]["match"][3] == 0)
        n["two tracks, one blob, equal d2"] += int(infos[0]["match"].get(5) == 2 and 9 not in infos[0]["match"])
        g2 = (256 * 2) ** 2
        n["d2 exactly at the gate"] += int(any(d == g2 for d, _, _ in infos[1]["pairs"]) and 0 in infos[1]["match"])
        n["d2 one past the gate"] += int(1 not in infos[1]["match"] and upd[1]["stats"]["born"] == 1)
        m2 = infos[2]["match"]
        d = {(i, j): d2 for d2, i, j in infos[2]["pairs"]}
        n["greedy is not the least total"] += int(m2 == {1: 0, 0: 1} and d[(1, 0)] + d[(0, 1)] > d[(0, 0)] + d[(1, 1)])
        n["three mutual-best rounds"] += int(infos[3]["rounds"] >= 3)
        t4 = upd[4]["tracks"]
        n["negative residual, alpha r no multiple of 256"] += int((101 * -34) % 256 != 0 and t4["px"][0] == 256 * 10 + 128 + 37 - 3 + ((101 * -34) >> 8))
        n["velocity clamp +"] += int(t4["vx"][1] == tm.VMAX)
        n["velocity clamp -"] += int(t4["vx"][2] == -tm.VMAX)
        n["hits saturate"] += int(t4["hits"][3] == tm.SAT)
        t5, t6 = upd[5]["tracks"][0], upd[6]["tracks"][0]
        n["alpha 0"] += int(t5["px"] == 256 * 10 + 128 + 37 + 40 and t5["vx"] == 40)
        n["alpha 256"] += int(t6["px"] == 256 * 11 + 128 and t6["py"] == 256 * 5 + 128)
        # ---- life cycle
        s, res, _ = model_of("lifecycle", w, h)
        T = lambda k: res[k][1]["tracks"]
        assert not T(3)["flags"][0] & tm.CONFIRMED and T(3)["hits"][0] == 2
        n["confirmed at exactly confirm_hits"] += int(T(5)["flags"][0] & tm.CONFIRMED and T(5)["hits"][0] == 3)
        n["coasting"] += int(T(9)["missed"][0] == 1 and T(11)["missed"][0] == 2 and T(9)["px"][0] == T(7)["px"][0] + T(7)["vx"][0])
        n["deleted at max_missed + 1"] += int(res[13][1]["stats"]["deleted"] == 1 and 1 not in T(13)["id"])
        n["lowest free slot reused in the same update"] += int(T(13)["id"][0] == 3 and T(13)["slot"][0] == 0 and bool(T(13)["flags"][0] & tm.BORN))
        ids = [int(i) for k in (1, 7, 13) for i in res[k][1]["tracks"]["id"]]
        n["ids strictly increasing"] += int(sorted(set(ids)) == [1, 2, 3])
        n["update refused: the layer has not moved on"] += int(res[14][0] == "state")
        n["update refused: the layer is two ahead"] += int(res[17][0] == "state")
        n["compose refused: the layer is ahead"] += int(res[18][0] == "state" and res[19][0] == "ok")
        n["fresh after a reset"] += int(res[22][0] == "ok")
        n["the last id"] += int(res[25][1]["stats"]["born"] == 1 and tm.ID_END - 1 in res[25][1]["tracks"]["id"])
        r27 = res[27][1]
        n["id limit"] += int(r27["stats"]["refused"] == tm.REFUSED_IDS and len(r27["blobs"]) == 0 and np.all(r27["labels"] == -1) and
                             np.array_equal(r27["tracks"], res[25][1]["tracks"]))
        assert res[29][1]["stats"]["refused"] == 0 and res[29][1]["stats"]["matched"] == 2
        k0 = 33
        assert [r for r, _ in res[k0:k0 + 12]] == ["arg"] * 12, [r for r, _ in res[k0:k0 + 12]]
        n["refusals of upload, set_params, compose"] += 12
        assert res[-1][0] == "ok" and res[-1][1]["stats"]["matched"] == 2
        # ---- compose
        s, res, _ = model_of("compose", w, h)
        comp = [(st_, snap) for st_, (r, snap) in zip(s.steps, res) if st_[0] == "compose"]
        assert all(r == "ok" for r, _ in res)
        n["horizon 0 is the layer's compose"] += int(np.array_equal(comp[0][1]["composed"], comp[0][1]["layer_composed"]))
        tr = res[2][1]["tracks"]
        want = tm.CONFIRMED | tm.MOVING
        n["an unconfirmed track"] += int(tr["flags"][5] & want == tm.MOVING)
        n["a slow track"] += int(tr["flags"][6] & want == tm.CONFIRMED)
        n["negative velocities"] += int(np.count_nonzero((tr["flags"] & want == want) & ((tr["vx"] < 0) | (tr["vy"] < 0))))
        n["positive velocities"] += int(np.count_nonzero((tr["flags"] & want == want) & ((tr["vx"] > 0) | (tr["vy"] > 0))))
        full = comp[3][1]["composed"]
        for name, t_, inside in (("right", 1, lambda x, y: x >= w), ("left", 2, lambda x, y: x < 0), ("bottom", 3, lambda x, y: y < 0),
                                 ("top", 4, lambda x, y: y >= h)):
            t_ = tr[t_]
            n["a sweep leaves through the " + name] += int(any(inside(int(t_["x0"]) + tm.stamp_offset(k, int(t_["vx"])),
                                                                      int(t_["y0"]) + tm.stamp_offset(k, int(t_["vy"]))) for k in range(1, 257)))
        assert np.count_nonzero(full == 127) > np.count_nonzero(comp[2][1]["composed"] == 127) > np.count_nonzero(comp[1][1]["composed"] == 127)
        stamped = (comp[1][1]["composed"] == 127) & (comp[0][1]["composed"] != 127)
        assert stamped.any()
        for t_ in (tr[5], tr[6]):                   # nothing in front of the unconfirmed and the slow track (horizon 1: the others are far)
            assert not stamped[t_["y0"]:t_["y1"] + 1, t_["x1"] + 1:t_["x1"] + 4].any()
        h8 = comp[2][1]["composed"]
        robot = comp[4][0][2]
        n["keep_clear -1"] += int(h8[robot[1], robot[0]] == 127)
        k0_, k3 = comp[4][1]["composed"], comp[5][1]["composed"]
        n["keep_clear 0"] += int(k0_[robot[1], robot[0]] != 127 and np.count_nonzero(k0_ != h8) == 1)
        n["keep_clear 3"] += int(np.count_nonzero(k3 != h8) > 1 and np.all((k3 != h8) <= (np.abs(np.mgrid[0:h, 0:w][1] - robot[0]) <= 3)))
        assert np.all(comp[5][1]["composed"][comp[0][1]["composed"] == 127] == 127)       # live cells are painted inside the box too
        n["a robot cell far outside"] += int(np.array_equal(comp[7][1]["composed"], h8) and np.array_equal(comp[8][1]["composed"], h8))
    # ---- the sweep of one cell is 8-connected for every velocity
    v = np.arange(-tm.VMAX, tm.VMAX + 1, dtype=np.int64)[:, None]
    k = np.arange(0, 4 * tm.MAX_HORIZON + 1, dtype=np.int64)[None, :]
    off = (k * v + 512) >> 10
    assert np.all(off[:, 0] == 0) and np.all(np.abs(np.diff(off, axis=1)) <= 1)
    n["every sweep is 8-connected, |v| <= 1023"] += off.size
    for name, c in sorted(n.items()):
        print(f"{c:8d}  {name}")
    zero = [name for name, c in n.items() if c == 0]
    assert not zero, zero
    assert len(n) >= 45, len(n)


def test_reversed_rays_give_the_same_output():
    for w, h in SIZES:
        a, b = (run_model(s) for s in reversed_scan_scripts(w, h))
        assert a[-2][1]["stats"]["blobs"] >= 3 and a[-2][1]["stats"]["matched"] >= 2
        for (ra, sa), (rb, sb) in zip(a, b):
            assert ra == rb == "ok"
            for key in sa:
                assert np.array_equal(sa[key], sb[key]) if key != "stats" else sa[key] == sb[key], key


def test_too_many_live_cells_and_exactly_the_most():
    s = large_script()
    res = run_model(s)
    assert res[1][1]["stats"]["live_cells"] == tm.MAX_CELLS and res[1][1]["stats"]["refused"] == 0 and res[1][1]["blobs"]["area"][0] == tm.MAX_CELLS
    assert res[3][1]["stats"]["refused"] == tm.REFUSED_CELLS and len(res[3][1]["labels"]) == tm.MAX_CELLS
    assert np.array_equal(res[3][1]["tracks"], res[1][1]["tracks"])
    assert res[5][1]["stats"]["refused"] == 0 and res[5][1]["stats"]["matched"] == 1


def large_script():
    """300 x 300: a block of exactly 65536 live cells, then one cell more, then the block again."""
    s = Script(300, 300)
    m = np.zeros((300, 300), bool)
    m[:256, :256] = True
    s.frame(m)
    m2 = m.copy()
    m2[299, 299] = True
    s.frame(m2)
    s.frame(m)
    return s


def test_track_metric():
    t = np.zeros(1, tm.TRACK_DTYPE)[0]
    t["px"], t["py"], t["vx"], t["vy"] = 256 * 10 + 128, 256 * 4, -128, 64
    x, y, vx, vy = tm.track_metric(t, (-1.0, -2.0), 0.05, 0.1)
    assert abs(x - (-1.0 + 10.5 * 0.05)) < 1e-12 and abs(y - (-2.0 + 4 * 0.05)) < 1e-12 and abs(vx + 0.25) < 1e-12 and abs(vy - 0.125) < 1e-12
