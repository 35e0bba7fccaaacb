"""Scripts for the obstacle layer and the obstacle tracks that are chosen by how the kernels are laid out, not by the definition: the
strides of k_obt_sweep, the two forms of k_obt_fold, the rounds, the lane split and the slot compaction of k_obt_assoc, the rows per
thread of k_obs_rowscan, the chunks and ballots of k_obs_livewrite, and poses that leave the host's box empty.  The scripts are built
with the Script classes of test_obstacle_tracks_model_cpu.py and test_obstacle_layer_model_cpu.py; the models are the yardstick as they
stand.  test_obstacle_edge_cases_cpu.py proves from the models' output that every script reaches what it is here for, and
test_gpu_obstacle_edges.py runs them on the device.
"""
import functools

import numpy as np

import obstacle_tracks_model as tm
import test_obstacle_layer_model_cpu as lcpu
import test_obstacle_tracks_model_cpu as tcpu
from test_obstacle_tracks_model_cpu import trk

F32 = np.float32

# The launch constants the cases depend on.  A change of one of these in the kernels should send the reader here.
WAVE = 64                   # the wavefront of gfx950: every __ballot and __shfl of both files
OBT_WG = 256                # bl_obstracks.hip, OBT_WG: the workgroup of the per-cell kernels
SWEEP_STRIDE = 64 * 256     # bl_obstracks.hip, OBT_SWEEP_BLOCKS * OBT_WG: the items k_obt_sweep takes per pass
ROWSCAN_THREADS = 1024      # bl_obslayer.hip, k_obs_rowscan's __launch_bounds__: per = ceil(H / 1024) rows per thread
LIVEWRITE_CHUNK = 256       # bl_obslayer.hip, k_obs_livewrite's __launch_bounds__: a row is walked in chunks of 256, four ballots each
LANES_PER_TRACK = 4         # bl_obstracks.hip, k_obt_assoc: t >> 2 is the track, t & 3 the sub-lane, blobs j = sub, sub + 4, ...
SLOT_GROUP = 64             # bl_obstracks.hip, k_obt_assoc's births: the free slots compacted over four ballots of 64 slots


def mask_of(w, h, xy=()):
    m = np.zeros((h, w), bool)
    for x, y in xy:
        m[y, x] = True
    return m


def to_pred(tid, px, py, vx, vy, **kw):
    """A slot whose prediction (position + velocity) is (px, py), in 1/256 cell."""
    return dict(dict(id=tid, px=px - vx, py=py - vy, vx=vx, vy=vy, hits=5, missed=0, flags=0), **kw)


# ---------------------------------------------------------------------------------------------------------------- tracks: k_obt_sweep
SWEEP_BLOB = (40, 60, 6, 6)                                  # x, y, width, height


def sweep_strides_script():
    """96 x 80: 600 isolated live cells first in the list, then a 6 x 6 blob with a confirmed moving track: the blob's cells are list
    entries 600.., so every one of their items but the first sub-steps lies in a second or later pass of k_obt_sweep's loop."""
    w, h = 96, 80
    s = tcpu.Script(w, h, confirm_hits=3, min_speed=64)
    bx, by, bw, bh = SWEEP_BLOB
    m = mask_of(w, h)
    m[0:60:2, 0:40:2] = True
    m[by:by + bh, bx:bx + bw] = True
    s.upload({5: trk(1, 42, 62, vx=-300, vy=150)}, fresh=1)
    s.frame(m)
    s.add("compose", 64, (0, 0), -1)
    s.add("compose", 7, (0, 0), -1)
    s.add("compose", 7, (30, 66), 2)
    s.add("compose", 7, (37, 63), 2)                          # a robot cell whose box the sweep does cross
    m2 = m.copy()                                             # one isolated cell more: L = 637, odd
    m2[0, 44] = True
    s.upload({200: trk(9, 42, 62, vx=300, vy=-150)}, fresh=1)
    s.frame(m2)
    s.add("compose", 64, (0, 0), -1)
    s.add("compose", 9, (0, 0), -1)
    s.add("compose", 9, (47, 58), 1)
    return s


# ---------------------------------------------------------------------------------------------------------------- tracks: k_obt_fold
def fold_waves_script():
    """131 x 67: the columns x = 0 and x = 130 are two tall kept blobs with a cell in every row's part of the list; between them
    isolated cells, of which those past rank 1023 are dropped.  So waves of the list hold kept and dropped cells together."""
    w, h = 131, 67
    s = tcpu.Script(w, h)
    m = mask_of(w, h)
    m[:, 0] = m[:, w - 1] = True
    m[0::2, 2:w - 2:2] = True
    s.frame(m)
    s.frame(m)
    s.add("compose", 2, (0, 0), -1)
    return s


# ---------------------------------------------------------------------------------------------------------------- tracks: k_obt_assoc
CHAIN_SLOTS = (3, 63, 64, 65, 127, 128, 200, 255, 0, 1, 2, 10, 20, 30, 40, 50, 60)


def assoc_chain_script():
    """200 x 9: 17 one-cell blobs at shrinking spacings and 17 tracks, each a little nearer to its own blob than to the one before it,
    while every blob but the last is nearer to the next track: one pair per round, from the last to the first."""
    w, h = 200, 9
    s = tcpu.Script(w, h, gate_cells=12)
    xs = [1]
    for sp in range(17, 1, -1):
        xs.append(xs[-1] + sp)
    tracks = {CHAIN_SLOTS[0]: to_pred(1, 256 * xs[0] + 128 - (17 * 128 + 200), 256 * 4 + 128, 0, 0)}
    for i in range(1, 17):
        S = 256 * (xs[i] - xs[i - 1])
        tracks[CHAIN_SLOTS[i]] = to_pred(i + 1, 256 * xs[i - 1] + 128 + S // 2 + 32, 256 * 4 + 128, 0, 0)
    s.chain_xs = xs
    s.upload(tracks, fresh=1)
    s.cells_frame([(x, 4) for x in xs])
    return s


MANY_SHAPES = (((0, 0), (1, 0), (0, 1), (1, 1)), ((0, 0), (1, 0), (2, 0)), ((0, 0), (1, 0), (0, 1)),
               ((0, 0), (1, 0), (2, 0), (0, 1), (1, 1), (2, 1)))
MANY_TIE_A, MANY_TIE_B = (6, 9), (10, 14)                    # the ranks of the two ties' blobs


def assoc_many_script():
    """160 x 120: 140 tracks with velocities of all four sign pairs in slots all over the table, each matched to its own multi-cell
    blob (ranks 335 and up) with a non-zero residual; and two tracks each at the same d2 from two blobs: ranks 6 and 9 (the smaller j
    in the higher sub-lane: 6 & 3 = 2, 9 & 3 = 1) and ranks 10 and 14 (the same sub-lane).  One-cell blobs far from every track place
    the ranks."""
    w, h = 160, 120
    s = tcpu.Script(w, h, gate_cells=3, alpha=100, beta=77)
    rng = np.random.default_rng(41)
    cells = [(x, 0) for x in range(0, 12, 2)]                                   # ranks 0 .. 5
    cells += [(60, 0), (100, 0), (102, 0), (60, 2)]                             # 6, 7, 8, 9: a track's prediction in the middle of (60, 1)
    cells += [(120, 2), (150, 2), (152, 2), (154, 2), (120, 4)]                 # 10, 11, 12, 13, 14: one in the middle of (120, 3)
    cells += [(x, y) for y in (8, 10, 12, 14) for x in range(0, w, 2)]          # 15 .. 334
    slots = sorted(int(v) for v in rng.choice(tm.MAX_TRACKS, 142, replace=False))
    order = [int(v) for v in rng.permutation(142)]
    tracks = {}
    k = 0
    for gy in range(7):
        for gx in range(20):
            shape = MANY_SHAPES[k % 4]
            bx, by = 8 * gx + 2, 20 + 8 * gy
            pts = [(bx + dx, by + dy) for dx, dy in shape]
            cells += pts
            A, sx, sy = len(pts), sum(p[0] for p in pts), sum(p[1] for p in pts)
            cx, cy = (256 * sx) // A + 128, (256 * sy) // A + 128
            sgx, sgy = (1, 1, -1, -1)[k % 4], (1, -1, 1, -1)[(k // 4) % 4]
            vx, vy = sgx * int(rng.integers(20, 400)), sgy * int(rng.integers(20, 400))
            rx, ry = int(rng.integers(1, 300)) * (1 if rng.random() < 0.5 else -1), int(rng.integers(1, 300)) * (1 if rng.random() < 0.5 else -1)
            tracks[slots[order[k]]] = to_pred(k + 1, cx - rx, cy - ry, vx, vy, hits=int(rng.integers(1, 6)))
            k += 1
    s.tie_slots = (slots[order[140]], slots[order[141]])
    tracks[s.tie_slots[0]] = to_pred(141, 256 * 60 + 128, 256 * 1 + 128, 37, -21)
    tracks[s.tie_slots[1]] = to_pred(142, 256 * 120 + 128, 256 * 3 + 128, -15, 44)
    s.upload(tracks, fresh=1)
    s.cells_frame(cells)
    s.add("compose", 8, (0, 0), -1)
    return s


BIRTH_FREE = (1, 62, 63, 64, 130, 255)
BIRTH_DELETED = (0, 129)
BIRTH_SLOTS = (0, 1, 62, 63, 64, 129, 130, 255)


def births_scattered_script():
    """160 x 120, places 8 cells apart and a gate of 3: 250 tracks leave six slots free, the tracks of two more slots are deleted in this
    update, and nine blobs nobody matches ask for the eight slots, which lie in all four of the 64-slot ballots."""
    w, h = 160, 120
    s = tcpu.Script(w, h, gate_cells=3, max_missed=3)
    rng = np.random.default_rng(43)
    places = [(8 * gx + 3, 8 * gy + 3) for gy in range(15) for gx in range(20)]             # 300
    kind = ["match"] * 100 + ["coast"] * 148 + ["delete"] * 2 + ["new"] * 9 + ["none"] * 41
    kind = [kind[int(v)] for v in rng.permutation(300)]
    occupied = [i for i in range(tm.MAX_TRACKS) if i not in BIRTH_FREE and i not in BIRTH_DELETED]
    occupied = [occupied[int(v)] for v in rng.permutation(len(occupied))]
    deleted = list(BIRTH_DELETED)
    tracks, cells, tid = {}, [], 0
    for (x, y), what in zip(places, kind):
        if what in ("match", "new"):
            cells += [(x, y), (x + 1, y)] if (x + y) % 3 else [(x, y)]
        if what in ("match", "coast", "delete"):
            tid += 1
            vx, vy = int(rng.integers(-200, 201)), int(rng.integers(-200, 201))
            slot = deleted.pop() if what == "delete" else occupied.pop()
            tracks[slot] = to_pred(tid, 256 * x + 128 + int(rng.integers(-100, 101)), 256 * y + 128 + int(rng.integers(-100, 101)), vx, vy,
                                   missed=3 if what == "delete" else int(rng.integers(0, 3)))
    assert not occupied and not deleted and len(tracks) == 250
    s.upload(tracks, next_id=1000, fresh=1)
    s.cells_frame(cells)
    s.cells_frame(cells)                                                                   # and the update after: the born ones match
    return s


POS_MAX = tm.POS_MAX


def pos_limits_script():
    """37 x 23: tracks uploaded at px, py = +-2^30 with |v| = 1023, outwards and inwards, beside an ordinary matched one: the
    prediction and the coasting at the limit, obt_d2's early outs."""
    w, h = 37, 23
    s = tcpu.Script(w, h, confirm_hits=3, min_speed=16)
    V = tm.VMAX
    tracks = {0: trk(1, 10, 10, vx=300, vy=150), 70: dict(id=2, px=POS_MAX, py=POS_MAX, vx=V, vy=V, hits=5, missed=0, flags=0),
              3: dict(id=3, px=-POS_MAX, py=-POS_MAX, vx=-V, vy=-V, hits=5, missed=0, flags=0),
              130: dict(id=4, px=POS_MAX, py=-POS_MAX, vx=V, vy=-V, hits=5, missed=0, flags=0),
              255: dict(id=5, px=-POS_MAX, py=POS_MAX, vx=-V, vy=V, hits=5, missed=0, flags=0),
              64: dict(id=6, px=POS_MAX, py=256 * 10 + 128, vx=-V, vy=0, hits=5, missed=0, flags=0),
              63: dict(id=7, px=256 * 12 + 128, py=-POS_MAX, vx=0, vy=V, hits=5, missed=0, flags=0),
              192: dict(id=8, px=-POS_MAX, py=256 * 11, vx=V, vy=-V, hits=tm.SAT, missed=1, flags=0)}
    s.upload(tracks, fresh=1)
    s.cells_frame([(11, 10), (12, 10), (11, 11), (12, 11)])
    s.cells_frame([(12, 11), (13, 11), (12, 12), (13, 12)])
    s.add("compose", 8, (0, 0), -1)
    s.add("roundtrip")                                        # refused: the coasting has taken positions past the limit
    s.cells_frame([(13, 11), (14, 11), (13, 12), (14, 12)])
    return s


# ---------------------------------------------------------------------------------------------------------------- tall and wide grids
TALL = ((5, 1025), (3, 2049))
TALL_LAYER = dict(ttl_scans=40, min_hits=1)


@functools.lru_cache(maxsize=None)
def tall_state(w, h):
    """(count, last, n) with about 30 % of the cells live: count 0 .. 3 at min_hits 1, last 0 .. 99 at n = 90 and ttl 40."""
    rng = np.random.default_rng(1000 + h)
    count = rng.integers(0, 4, (h, w)).astype(np.uint8)
    last = rng.integers(0, 100, (h, w)).astype(np.uint32)
    count[h - 1, w - 1], last[h - 1, w - 1] = 2, 60           # the last cell of the last row is live
    count.flags.writeable = last.flags.writeable = False
    return count, last, 90


def tall_cells(w, h):
    c = np.full((h, w), -100, np.int8)
    c[::7, 0] = 100
    c[h - 1, :] = 33
    return c


def tall_layer_script(w, h):
    count, last, n = tall_state(w, h)
    s = lcpu.Script(tall_cells(w, h), **TALL_LAYER)
    s.upload(count, last, n)
    pose = s.pose_at(w / 2, h - 20.5, 0.0)
    far = [y for y in range(h - 60, h - 100, -1) if y % 7 == 3]       # rows more than tol_cells from the map's cells in column 0
    s.update([s.ray_to(pose, w // 2, h - 1), s.ray_to(pose, w // 2, far[0]), s.ray_to(pose, w - 1, far[3])], pose)
    return s


def tall_tracks_script(w, h):
    count, last, n = tall_state(w, h)
    s = tcpu.Script(w, h, cells=tall_cells(w, h), layer=TALL_LAYER)
    s.n = n
    s.add("layer", count, last, n)
    s.add("update")
    s.add("compose", 3, (1, h - 2), 1)
    return s


WIDE = (600, 3)
WIDE_ROW2 = (0, 63, 64, 127, 128, 191, 192, 255, 256, 511, 512, 599)
WIDE_CAPS = (608, 609, 611, 255, 256, 257, 612)              # 612: the full count


def wide_mask():
    w, h = WIDE
    m = mask_of(w, h, [(x, 2) for x in WIDE_ROW2])
    m[0, :] = True
    return m


def wide_layer_script():
    w, h = WIDE
    m = wide_mask()
    s = lcpu.Script(np.full((h, w), -100, np.int8))
    s.upload(m.astype(np.uint8), np.where(m, 7, 0).astype(np.uint32), 7)
    return s


def wide_tracks_script():
    w, h = WIDE
    s = tcpu.Script(w, h)
    s.frame(wide_mask())
    s.add("compose", 1, (0, 0), -1)
    return s


def caps_of(script, live):
    """The caps at which the device's live_cells(cap) is held against the first `cap` of the model's list: the listed ones of the wide
    rows; for a tall grid the counts around the first row that is some thread's second, around row 1024, and the full count."""
    w, h = script.shape
    if (w, h) == WIDE:
        return WIDE_CAPS
    before = lambda y: int(np.count_nonzero(live[:, 1] < y))
    return tuple(sorted({0, 1, before(1), before(1) + 1, before(ROWSCAN_THREADS), before(ROWSCAN_THREADS) + 1, before(h - 1), len(live) - 1,
                         len(live)}))


# ---------------------------------------------------------------------------------------------------------------- layer: far poses
def far_poses_script():
    """37 x 23: between ordinary updates, one from a pose whose grid position is beyond 2^30 in x (no ray has an end cell: OFF), one
    beyond -2^30 in y, and one 10 000 cells left of the grid (every valid ray OUTSIDE).  The host's box of the walks is empty each
    time: k_obs_apply is not launched, and stamps left by the update before must not count again."""
    w, h = 37, 23
    s = lcpu.Script(lcpu.open_cells(w, h))
    c = h // 2
    pose = s.pose_at(10.5, c + 0.5, 0.3)
    rays = list(lcpu.scan_a(s, pose, w, h).values())
    s.update(rays, pose)
    s.update(rays, s.pose_at(2.0 ** 31, c + 0.5, 0.3))
    s.update(rays, pose)
    s.update(rays, s.pose_at(-10000.5, c + 0.5, 0.3))
    s.update(rays[::2], pose)
    s.update(rays, s.pose_at(10.5, -2.0 ** 31, 0.3))
    s.update(rays, pose)
    return s


TRACK_CASES = (("sweep_strides", sweep_strides_script), ("fold_waves", fold_waves_script), ("assoc_chain", assoc_chain_script),
               ("assoc_many", assoc_many_script), ("births_scattered", births_scattered_script), ("pos_limits", pos_limits_script),
               ("tall_5x1025", lambda: tall_tracks_script(5, 1025)), ("tall_3x2049", lambda: tall_tracks_script(3, 2049)),
               ("wide_600x3", wide_tracks_script))
LAYER_CASES = (("tall_5x1025", lambda: tall_layer_script(5, 1025)), ("tall_3x2049", lambda: tall_layer_script(3, 2049)),
               ("wide_600x3", wide_layer_script), ("far_poses", far_poses_script))


@functools.lru_cache(maxsize=None)
def tracks_model_of(name):
    """(script, model results, infos), computed once and shared (nobody changes them)."""
    script = dict(TRACK_CASES)[name]()
    infos = []
    return script, tcpu.run_model(script, infos), infos


@functools.lru_cache(maxsize=None)
def layer_model_of(name):
    script = dict(LAYER_CASES)[name]()
    infos = []
    return script, lcpu.run_model(script, infos), infos
