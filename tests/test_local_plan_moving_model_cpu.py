"""The model of the local planner's moving rule (tests/local_plan_moving_model.py) on its own: every condition of the definition is
reached at least once and printed as a count.  The inputs are tests/local_plan_moving_cases.py's, which the GPU test compares byte
for byte."""
import numpy as np
import pytest

import local_plan_model as lpm
import local_plan_moving_cases as mc
import local_plan_moving_model as lmm
import obstacle_tracks_model as tm
from obstacle_layer_model import StateError


def _plain(name, k=0):
    case = mc.get(name)
    rec, cs = lpm.command(case.world(), case.p, *case.states[k])
    return rec, cs


def test_no_used_slot_is_the_plain_command():
    n = 0
    for name in ("no_used", "unused_kinds"):
        rec, cs, fh = mc.model(name)[0]
        prec, pcs = _plain(name)
        assert rec.tobytes() == prec.tobytes() and np.array_equal(cs, pcs) and not fh.any()
        n += 1
    kinds = [int(s["flags"]) for s in mc.get("unused_kinds").slots[3:7]]
    assert kinds == [tm.MOVING | tm.MATCHED, tm.CONFIRMED | tm.MATCHED, tm.CONFIRMED | tm.MOVING, mc.USED] and int(mc.get("unused_kinds").slots[6]["id"]) == 0
    print(f"no used slot: {n} cases equal lpm.command; unused kinds ignored: unconfirmed, not moving, coasting, free")


def test_a_born_slot_is_used():
    rec, cs, fh = mc.model("born_used")[0]
    prec, _ = _plain("born_used")
    assert fh.any() and int(rec["n_admissible"]) < int(prec["n_admissible"])
    print(f"born slot used: {int(np.count_nonzero(fh))} candidates refused, {int(rec['n_admissible'])} of {int(prec['n_admissible'])} admissible")


def test_entry_at_exactly_step_k():
    out = {}
    for name, k in (("entry_1", 1), ("entry_n", 20), ("entry_n_plus_1", 21)):
        case = mc.get(name)
        rec, cs, fh = mc.model(name)[0]
        c = mc._straight(case.p)
        _, pcs = _plain(name)
        assert pcs[c] != lpm.COST_NONE
        if k <= case.p.n_steps:
            assert int(fh[c]) == k and cs[c] == lpm.COST_NONE
        else:
            assert int(fh[c]) == 0 and cs[c] == pcs[c]
        out[name] = int(fh[c])
    print("entry at exactly step k (first_hit of the straight candidate):", out)


def test_the_four_edges_at_three_margins():
    on = beyond = 0
    for mg, side, is_on in mc.EDGES:
        name = "edge_%d_%s_%s" % (mg, side, "on" if is_on else "beyond")
        rec, cs, fh = mc.model(name)[0]
        prec, _ = _plain(name)
        assert int(prec["flags"]) == 0 and int(prec["n_admissible"]) == 1
        if is_on:
            assert int(rec["flags"]) == lpm.BLOCKED and int(fh[0]) == 1
            on += 1
        else:
            assert rec.tobytes() == prec.tobytes() and int(fh[0]) == 0
            beyond += 1
    print(f"edges: {on} cells on an edge refused, {beyond} one cell beyond admitted (margins 0, 1, 64)")


def test_floor_not_truncation():
    for name in ("floor_x", "floor_y"):
        rec, cs, fh = mc.model(name)[0]
        assert int(rec["flags"]) == lpm.BLOCKED and int(fh[0]) == 1
    print("floor, not truncation: 2 cases (negative vx, negative vy) refused at step 1")


@pytest.mark.parametrize("name", ["q_1", "q_255", "lead_255", "lead_0_q_3", "v_1023", "v_1023_q_1_lead_255"])
def test_timing_knobs(name):
    case = mc.get(name)
    rec, cs, fh = mc.model(name)[0]
    c = mc._straight(case.p)
    assert 1 <= int(fh[c]) <= 13 and cs[c] == lpm.COST_NONE and int(rec["n_admissible"]) >= 1
    print(f"{name}: q {case.m.q}, lead {case.m.lead}, first_hit of the straight candidate {int(fh[c])}, {int(np.count_nonzero(fh))} candidates refused")


def test_boxes_beyond_int16():
    case = mc.get("beyond_int16")
    rec, cs, fh = mc.model("beyond_int16")[0]
    c = mc._straight(case.p)
    assert any(abs(int(s[k])) > 32767 for s in case.slots[:3] for k in ("x0", "y0", "x1", "y1"))
    assert int(fh[c]) > 0 and int(rec["n_admissible"]) >= 1
    print(f"beyond int16: {int(np.count_nonzero(fh))} candidates refused, {int(rec['n_admissible'])} admissible")


def test_blocked_shapes():
    rec, cs, fh = mc.model("own_cell")[0]
    assert int(rec["flags"]) == lpm.BLOCKED and int(rec["n_admissible"]) == 0 and (fh == 1).all()
    rec, cs, fh = mc.model("all_but_one")[0]
    assert int(rec["flags"]) == 0 and int(rec["n_admissible"]) == 1 and int(rec["index"]) == mc.get("all_but_one").note
    rec, cs, fh = mc.model("tie")[0]
    adm = np.flatnonzero(cs != lpm.COST_NONE)
    assert len(adm) == 2 and cs[adm[0]] == cs[adm[1]] and int(rec["index"]) == int(adm[0]) == mc.get("tie").note
    print(f"own cell: BLOCKED with 0 admissible; all but one: candidate {mc.get('all_but_one').note} alone; tie of {adm.tolist()} to {int(rec['index'])}")


def test_a_full_table_of_used_slots():
    case = mc.get("full_table")
    rec, cs, fh = mc.model("full_table")[0]
    assert len(lmm.used_slots(case.slots)) == 256
    assert 1 <= int(rec["n_admissible"]) and fh.any()
    print(f"256 used slots: {int(np.count_nonzero(fh))} candidates refused, {int(rec['n_admissible'])} admissible")


def test_the_cases_for_the_device_paths():
    for kept, v in mc.TABLE_SIDES:
        name = "table_%d_%s" % (kept, "staged" if v == 0.1 else "grids")
        rec, cs, fh = mc.model(name)[0]
        assert (kept == 0) == (not fh.any())
        print(f"{name}: {int(np.count_nonzero(fh))} candidates refused, {int(rec['n_admissible'])} admissible")
    rec, cs, fh = mc.model("reach_cull")[0]
    print(f"reach_cull: {int(np.count_nonzero(fh))} candidates refused")
    flags = [int(r["flags"]) for r, _, _ in mc.model("seven_states")]
    assert {0, lpm.REACHED, lpm.OFF_FIELD, lpm.BLOCKED} <= set(flags)
    print("seven_states flags:", flags)
    rec, cs, fh = mc.model("partial_last_workgroup")[0]
    assert int(fh[64 * 5 + 4]) > 0 and int(fh[3]) > 0


def test_the_twelve_refusals():
    w = mc.small_world()
    reasons = {k: lmm.refusal(w, p, m, shape, states) for k, (p, m, shape, states) in mc.refusals().items()}
    assert len(reasons) == 12 and all(reasons.values()), reasons
    good = mc.get("no_used")
    assert lmm.refusal(w, good.p, good.m, (w.w, w.h), good.states) is None
    print("refusals:", reasons)


@pytest.mark.parametrize("w,h", [(37, 23), (64, 64)])
def test_compose_static(w, h):
    rng = np.random.default_rng(w)
    cells = rng.integers(-100, 100, (h, w)).astype(np.int8)
    live_at = mc.blob_scene(w, h)
    t = tm.Tracker(w, h, **dict(tm.BASE, max_cells=9))
    # no tracks: the layer's compose
    plain = np.where(live_at(1), 127, cells).astype(np.int8)
    assert np.array_equal(lmm.compose_static(t, live_at(1), 0, cells), plain)
    left_out = 0
    for n in range(1, 7):
        live = live_at(n)
        t.update(live, n)
        out = lmm.compose_static(t, live, n, cells)
        moving = [s for s in t.slots if s["id"] != 0 and (s["flags"] & 3) == 3]
        exp = np.where(live, 127, cells).astype(np.int8)
        for s in moving:
            exp[s["y0"]:s["y1"] + 1, s["x0"]:s["x1"] + 1] = cells[s["y0"]:s["y1"] + 1, s["x0"]:s["x1"] + 1]
        assert np.array_equal(out, exp), n
        left_out += len(moving)
    assert len(moving) == 1 and len(t.tracks()) == 2              # the moving blob is left out, the standing one kept
    with pytest.raises(StateError):
        lmm.compose_static(t, live, 9, cells)
    # a dropped blob (label -1) is kept: a blob too large to be eligible has no track, and so is one beyond the kept blobs
    big = live.copy()
    big[1:5, 15:20] = True
    t.update(big, 7)
    out = lmm.compose_static(t, big, 7, cells)
    assert (out[1:5, 15:20] == 127).all()
    t.labels[:] = -1
    assert np.array_equal(lmm.compose_static(t, big, 7, cells), np.where(big, 127, cells))
    # after an upload: no blobs, the layer's compose
    slots, st = t.download()
    t.upload(slots, st["n"], st["next_id"], 0)
    assert np.array_equal(lmm.compose_static(t, big, 7, cells), np.where(big, 127, cells))
    print(f"compose_static {w} x {h}: the moving blob left out on {left_out} updates, the standing one, a trackless one and a dropped one kept")


def test_the_kernel_offset_without_a_division_is_the_floor():
    """lp_mov_offset (bl_localplan.hip) restated: floor(n / (256 q)) as ((n >> 8) + 2048 q) * ceil(2^28 / q) >> 28, minus 2048, over
    every q and every n = t v + 128 q that t <= 510 and |v| <= 1023 can form."""
    for q in range(1, 256):
        magic = (2 ** 28 + q - 1) // q
        n = np.arange(-510 * 1023 + 128 * q, 510 * 1023 + 128 * q + 1, dtype=np.int64)
        a = (n >> 8) + 2048 * q
        assert a.min() >= 9 and a.max() < 2 ** 20 and magic <= 2 ** 28
        assert np.array_equal(((a * magic) >> 28) - 2048, n // (256 * q)), q
    assert lmm.offset(1, -300, 2) == -1
