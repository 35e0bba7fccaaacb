"""The scripts of tests/obstacle_edge_cases.py through the models alone: for every script the fact about the kernels' launch shape
that it exists for, derived from the model's output, printed as a count; a count of 0 fails.  test_gpu_obstacle_edges.py runs the
same scripts on the device."""
import collections

import numpy as np

import obstacle_edge_cases as ec
import obstacle_layer_model as om
import obstacle_tracks_model as tm


def updates(script, res):
    return [snap for st, (_, snap) in zip(script.steps, res) if st[0] == "update"]


def composes(script, res):
    return [(st, snap) for st, (_, snap) in zip(script.steps, res) if st[0] == "compose"]


def sweep_by_items(snap, w, h, horizon, late_only=False, first_only=False, wrong_s=False):
    """The cells k_obt_sweep's items stamp (no keep-clear), item by item as the kernel numbers them: item k is sub-step k // L + 1 of
    live cell k % L.  late_only: the items of the second and later passes alone; first_only: those of the first pass alone; wrong_s:
    the sub-step formed from k % stride."""
    live, labels, blobs, tracks = snap["live"], snap["labels"], snap["blobs"], snap["tracks"]
    by_slot = {int(t["slot"]): t for t in tracks}
    L = len(live)
    out = np.zeros((h, w), bool)
    want = tm.CONFIRMED | tm.MOVING
    for i in range(L):
        lab = int(labels[i])
        if lab < 0 or blobs["track"][lab] < 0:
            continue
        t = by_slot[int(blobs["track"][lab])]
        if int(t["flags"]) & want != want:
            continue
        for k in range(i, L * 4 * horizon, L):
            if (late_only and k < ec.SWEEP_STRIDE) or (first_only and k >= ec.SWEEP_STRIDE):
                continue
            s = (k % ec.SWEEP_STRIDE if wrong_s else k) // L + 1
            x, y = int(live[i][0]) + tm.stamp_offset(s, int(t["vx"])), int(live[i][1]) + tm.stamp_offset(s, int(t["vy"]))
            if 0 <= x < w and 0 <= y < h:
                out[y, x] = True
    return out


def wave_kinds(labels):
    """Per wave of 64 of the label list, k_obt_fold's case: how many kept blobs and whether dropped cells sit beside them."""
    n = collections.Counter()
    for a in range(0, len(labels), ec.WAVE):
        lab = labels[a:a + ec.WAVE]
        kept, dropped = len(set(lab[lab >= 0].tolist())), bool(np.any(lab < 0))
        if kept == 0:
            n["waves of dropped cells alone"] += 1
        else:
            n["waves of %s, %s" % ("one kept blob" if kept == 1 else "several kept blobs", "with dropped cells" if dropped else "no dropped cells")] += 1
    return n


def test_every_launch_shape_is_reached():
    n = collections.Counter()
    for name, _ in ec.TRACK_CASES:                    # the device's procedure gives the sorted greedy choice
        _, _, infos = ec.tracks_model_of(name)
        for info in infos:
            if "pairs" in info:
                assert tm.mutual_best(info["pairs"])[0] == tm.greedy(info["pairs"]), name
                n["updates whose mutual-best rounds equal the sorted greedy walk"] += 1

    # ---- k_obt_sweep's strides
    s, res, _ = ec.tracks_model_of("sweep_strides")
    assert all(r == "ok" for r, _ in res)
    w, h = s.shape
    upd, comp = updates(s, res), composes(s, res)
    bx, by, bw, bh = ec.SWEEP_BLOB
    mover = []
    for u, (L, slot) in zip(upd, ((636, 5), (637, 200))):
        assert len(u["live"]) == L and u["stats"]["matched"] == 1
        assert [(int(x), int(y)) for x, y in u["live"][-bw * bh:]] == [(x, y) for y in range(by, by + bh) for x in range(bx, bx + bw)]
        t = u["tracks"][u["tracks"]["slot"] == slot][0]
        assert t["flags"] & (tm.MATCHED | tm.CONFIRMED | tm.MOVING) == tm.MATCHED | tm.CONFIRMED | tm.MOVING
        mover.append(t)
    assert mover[0]["vx"] < 0 < mover[0]["vy"] and mover[1]["vx"] > 0 > mover[1]["vy"]
    for u, (st, c) in ((upd[0], comp[0]), (upd[1], comp[4])):
        L, horizon = len(u["live"]), st[1]
        items = L * 4 * horizon
        livem = c["layer_composed"] == 127
        every = sweep_by_items(u, w, h, horizon)
        assert np.array_equal((c["composed"] == 127), every | livem)
        late = sweep_by_items(u, w, h, horizon, late_only=True)
        first_pass = sweep_by_items(u, w, h, horizon, first_only=True)
        assert np.array_equal(late | first_pass, every)
        wrong = sweep_by_items(u, w, h, horizon, wrong_s=True)
        n["sweep: items beyond the first 16384 with a stamping track"] += max(items - ec.SWEEP_STRIDE, 0)
        n["sweep: passes of the loop"] += -(-items // ec.SWEEP_STRIDE)
        n["sweep: cells stamped beyond the live ones"] += int(np.count_nonzero(every & ~livem))
        n["sweep: cells stamped by items k >= 16384 alone"] += int(np.count_nonzero(late & ~first_pass & ~livem))
        n["sweep: cells that a sub-step formed from k % 16384 gets wrong"] += int(np.count_nonzero((wrong | livem) != (every | livem)))
        n["sweep: waves whose 64 items cross a sub-step boundary"] += sum(1 for a in range(0, items, ec.WAVE) if a // L != min(a + ec.WAVE - 1, items - 1) // L)
        n["sweep: L divides no power of two"] += int(L & (L - 1) != 0 and ec.SWEEP_STRIDE % L != 0)
    assert (len(upd[0]["live"]) * 4 * 64, int(np.count_nonzero((comp[0][1]["composed"] == 127) & (comp[0][1]["layer_composed"] != 127)))) == (162816, 219)
    assert np.array_equal(comp[2][1]["composed"], comp[1][1]["composed"])              # robot (30, 66): its box is off the sweep
    n["sweep: keep-clear box across the sweep, cells kept clear"] += int(np.count_nonzero(comp[3][1]["composed"] != comp[1][1]["composed"]))
    n["sweep: keep-clear box across the sweep, other signs"] += int(np.count_nonzero(comp[6][1]["composed"] != comp[5][1]["composed"]))

    # ---- k_obt_fold's two forms with dropped lanes
    s, res, _ = ec.tracks_model_of("fold_waves")
    upd = updates(s, res)
    st = upd[0]["stats"]
    assert (st["blobs"], st["dropped"], st["live_cells"]) == (2178, 2178 - 1024, 2310)
    b = upd[0]["blobs"]
    tall = np.flatnonzero(b["area"] == 67)
    assert len(tall) == 2 and b["x0"][tall[0]] == b["x1"][tall[0]] == 0 and b["x0"][tall[1]] == b["x1"][tall[1]] == 130
    print("fold_waves: the two columns are the blobs of ranks", tall.tolist())
    kinds = wave_kinds(upd[0]["labels"])
    for k, v in kinds.items():
        n["fold: " + k] += v
    for k in ("waves of several kept blobs, no dropped cells", "waves of several kept blobs, with dropped cells",
              "waves of one kept blob, with dropped cells"):
        n["fold: " + k] += 0
    assert (kinds["waves of several kept blobs, no dropped cells"], kinds["waves of several kept blobs, with dropped cells"],
            kinds["waves of one kept blob, with dropped cells"]) == (16, 18, 3), kinds
    assert upd[0]["stats"]["born"] == 256 and upd[1]["stats"]["matched"] == 256
    n["fold: tracks matched in the second update"] += upd[1]["stats"]["matched"]
    s, res, _ = ec.tracks_model_of("wide_600x3")
    for k, v in wave_kinds(updates(s, res)[0]["labels"]).items():
        n["fold (wide rows): " + k] += v
    n["fold (wide rows): waves of one kept blob, no dropped cells"] += 0

    # ---- k_obt_assoc: rounds
    s, res, infos = ec.tracks_model_of("assoc_chain")
    st = updates(s, res)[0]["stats"]
    assert (st["rounds"], st["matched"], st["born"]) == (17, 17, 0), st
    assert infos[0]["match"] == {slot: j for j, slot in enumerate(ec.CHAIN_SLOTS)}
    n["assoc: mutual-best rounds (16 or more)"] += st["rounds"] if st["rounds"] >= 16 else 0

    # ---- k_obt_assoc: many tracks, the lane split
    s, res, infos = ec.tracks_model_of("assoc_many")
    info, u = infos[0], updates(s, res)[0]
    resid = {i: (info["cents"][j][0] - info["preds"][i][0], info["cents"][j][1] - info["preds"][i][1]) for i, j in info["match"].items()}
    moved = [i for i, (rx, ry) in resid.items() if rx != 0 and ry != 0]
    n["assoc: tracks matched with a non-zero residual (128 or more)"] += len(moved) if len(moved) >= 128 else 0
    for g in range(4):
        n["assoc: matched slots in %d .. %d" % (ec.SLOT_GROUP * g, ec.SLOT_GROUP * g + 63)] += sum(1 for i in moved if i // ec.SLOT_GROUP == g)
    slots0 = s.steps[0][1]
    for sx_, sy_ in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
        n["assoc: matched tracks with velocity signs (%+d, %+d)" % (sx_, sy_)] += sum(
            1 for i in moved if np.sign(slots0["vx"][i]) == sx_ and np.sign(slots0["vy"][i]) == sy_)
    n["assoc: matched blobs of rank 256 and beyond"] += sum(1 for j in info["match"].values() if j >= 256)
    n["assoc: matched multi-cell blobs"] += sum(1 for j in info["match"].values() if u["blobs"]["area"][j] > 1)
    for label, slot, (ja, jb) in (("ranks 6 and 9: the smaller j in the higher sub-lane", s.tie_slots[0], ec.MANY_TIE_A),
                                  ("ranks j and j + 4: one sub-lane", s.tie_slots[1], ec.MANY_TIE_B)):
        mine = sorted((d2, j) for d2, i, j in info["pairs"] if i == slot)
        assert [j for _, j in mine] == [ja, jb] and mine[0][0] == mine[1][0] > 0, (label, mine)
        assert info["match"][slot] == ja
        n["assoc: tie of equal d2, " + label] += 1
    assert (ec.MANY_TIE_A[0] & 3) > (ec.MANY_TIE_A[1] & 3) and (ec.MANY_TIE_B[0] & 3) == (ec.MANY_TIE_B[1] & 3)
    assert u["stats"]["matched"] == 142 and u["stats"]["rounds"] == 1
    n["assoc: births beside the matches, and blobs left unborn"] += min(u["stats"]["born"], u["stats"]["unborn"])

    # ---- k_obt_assoc: births into scattered slots
    s, res, infos = ec.tracks_model_of("births_scattered")
    u = updates(s, res)[0]
    info = infos[0]
    st = u["stats"]
    assert (st["born"], st["unborn"], st["deleted"], st["matched"], st["tracks"]) == (8, 1, 2, 100, 256), st
    born = u["tracks"][(u["tracks"]["flags"] & tm.BORN) != 0]
    assert tuple(int(v) for v in born["slot"]) == ec.BIRTH_SLOTS and [int(v) for v in born["id"]] == list(range(1000, 1008))
    assert [int(u["blobs"]["track"][j]) for j in info["wanted"]] == list(ec.BIRTH_SLOTS) + [-1]
    assert info["wanted"] == sorted(info["wanted"]) and not set(ec.BIRTH_DELETED) & set(info["match"])
    n["births: slots taken, in rank order, ids consecutive"] += len(born)
    n["births: 64-slot ballots that hold a free slot"] += len({i // ec.SLOT_GROUP for i in ec.BIRTH_SLOTS})
    n["births: slots freed by a deletion in the same update"] += len(set(ec.BIRTH_DELETED) & set(int(v) for v in born["slot"]))
    n["births: deletions in slots other than 0"] += sum(1 for i in ec.BIRTH_DELETED if i != 0)
    n["births: tracks that coast"] += int(np.count_nonzero(u["tracks"]["missed"] > 0))
    n["births: the ninth blob born one update later"] += updates(s, res)[1]["stats"]["born"]

    # ---- positions at the limit
    s, res, _ = ec.tracks_model_of("pos_limits")
    upd = updates(s, res)
    t0 = s.steps[0][1]
    n["limits: tracks uploaded at |px| or |py| = 2^30"] += int(np.count_nonzero((np.abs(t0["px"].astype(np.int64)) == tm.POS_MAX) | (np.abs(t0["py"].astype(np.int64)) == tm.POS_MAX)))
    t2 = upd[1]["tracks"]
    n["limits: positions past 2^30 after coasting"] += int(np.count_nonzero(np.abs(t2["px"].astype(np.int64)) > tm.POS_MAX))
    n["limits: positions back inside after coasting"] += int(np.count_nonzero(np.abs(t2["px"].astype(np.int64)) == tm.POS_MAX - 2 * tm.VMAX))
    assert upd[0]["stats"]["matched"] == upd[1]["stats"]["matched"] == upd[2]["stats"]["matched"] == 1 and upd[1]["stats"]["tracks"] == 8
    assert [r for r, _ in res].count("arg") == 1 and res[[st[0] for st in s.steps].index("roundtrip")][0] == "arg"
    n["limits: the coasted state refused by upload"] += 1
    n["limits: a track at the limit deleted"] += upd[2]["stats"]["deleted"]
    c = composes(s, res)[0][1]
    n["limits: cells stamped by the ordinary track beside them"] += int(np.count_nonzero(c["composed"] != c["layer_composed"]))

    # ---- tall grids: rows per thread of k_obs_rowscan
    for w, h in ec.TALL:
        name = "tall_%dx%d" % (w, h)
        per = -(-h // ec.ROWSCAN_THREADS)
        s, res, _ = ec.layer_model_of(name)
        assert all(r == "ok" for r, _ in res)
        live = res[0][1]["live"]
        n["%s: rows per thread" % name] += per if per > 1 else 0
        n["%s: threads with fewer rows than the others" % name] += ec.ROWSCAN_THREADS - h // per
        n["%s: live cells in rows 1024 and up" % name] += int(np.count_nonzero(live[:, 1] >= ec.ROWSCAN_THREADS))
        n["%s: live cells in the last row" % name] += int(np.count_nonzero(live[:, 1] == h - 1))
        n["%s: live rows that are not a thread's first" % name] += len({int(y) for y in live[:, 1] if y % per})
        assert 0.25 < len(live) / (w * h) < 0.35
        stl = res[1][1]["stats"]
        n["%s: cells hit and cleared by an update near the last row (sums over rows per thread)" % name] += min(stl["hs"], stl["clr"])
        n["%s: caps compared" % name] += len(ec.caps_of(s, live))
        s, res, _ = ec.tracks_model_of(name)
        assert all(r == "ok" for r, _ in res)
        u = updates(s, res)[0]
        assert np.array_equal(u["live"], live)
        n["%s: blobs" % name] += u["stats"]["blobs"]
        n["%s: blobs with cells on both sides of row 1024" % name] += int(np.count_nonzero((u["blobs"]["y0"] < ec.ROWSCAN_THREADS) & (u["blobs"]["y1"] >= ec.ROWSCAN_THREADS)))

    # ---- wide rows: chunks and ballots of k_obs_livewrite
    s, res, _ = ec.layer_model_of("wide_600x3")
    live = res[0][1]["live"]
    assert len(live) == 612 == ec.WIDE_CAPS[-1] and res[0][1]["stats"]["live"] == 612
    row2 = [int(x) for x, y in live if y == 2]
    assert tuple(row2) == ec.WIDE_ROW2 and not any(y == 1 for _, y in live)
    for edge in (64, 128, 192, 256, 512):
        kind = "chunk" if edge % ec.LIVEWRITE_CHUNK == 0 else "wave"
        n["wide: row 2 live on both sides of the %s boundary %d|%d" % (kind, edge - 1, edge)] += int(edge - 1 in row2 and edge in row2)
    n["wide: an empty row between rows with live cells"] += 1
    for cap in ec.WIDE_CAPS[:3]:
        x = row2[cap - 600 - 1]
        n["wide: a cap whose last cell is in chunk %d of row 2" % (x // ec.LIVEWRITE_CHUNK)] += 1
    n["wide: caps inside row 0 around its chunk boundary"] += sum(1 for c in ec.WIDE_CAPS if c in (255, 256, 257))
    s, res, _ = ec.tracks_model_of("wide_600x3")
    u = updates(s, res)[0]
    assert u["stats"]["blobs"] == 8 and u["blobs"]["area"][0] == 600
    n["wide: blobs that straddle a boundary"] += int(np.count_nonzero((u["blobs"]["area"] == 2) & (u["blobs"]["y0"] == 2)))

    # ---- far poses
    s, res, infos = ec.layer_model_of("far_poses")
    assert all(r == "ok" for r, _ in res)
    for k in (1, 3, 5):
        cls, stl = res[k][1]["classes"], res[k][1]["stats"]
        assert stl["valid"] > 10 and stl["hs"] == 0 and stl["clr"] == 0 and res[k][1]["n"] == k + 1
        assert np.array_equal(res[k][1]["count"], res[k - 1][1]["count"]) and np.array_equal(res[k][1]["last"], res[k - 1][1]["last"])
        assert res[k - 1][1]["stats"]["hs"] > 0 and res[k - 1][1]["stats"]["clr"] > 0       # the update before left stamps
        if k == 3:
            assert stl["classes"][om.OUTSIDE] == len(infos[k]["rays"]) == stl["valid"] - 2         # the two rays of a non-finite theta: OFF
            assert stl["classes"][om.OUTSIDE] + stl["classes"][om.OFF] == len(cls) and all(r["s"][0] <= -10000 for r in infos[k]["rays"])
            n["far poses: rays OUTSIDE from 10 000 cells left of the grid"] += stl["classes"][om.OUTSIDE]
        else:
            assert stl["classes"][om.OFF] == len(cls) and not infos[k]["rays"]
            n["far poses: valid rays OFF from a grid position beyond 2^30 (%s)" % ("x" if k == 1 else "-y")] += stl["valid"]
    n["far poses: ordinary updates after them that hit and clear"] += sum(1 for k in (2, 4, 6) if res[k][1]["stats"]["hs"] > 0 and res[k][1]["stats"]["clr"] > 0)

    for name, c in sorted(n.items()):
        print(f"{c:8d}  {name}")
    zero = [name for name, c in n.items() if c == 0]
    assert not zero, zero
    assert len(n) >= 60, len(n)
