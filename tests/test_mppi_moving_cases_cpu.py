"""tests/mppi_moving_cases.py against the model (tests/mppi_model.py) alone: every case reaches the path it is named for.  The GPU
tests (tests/test_gpu_mppi_moving_edges.py) take the same cases, so what is asserted here is what they compare on."""
import numpy as np
import pytest

import local_plan_moving_model as lmm
import mppi_cases as mc
import mppi_model as mm
import mppi_moving_cases as mv
import obstacle_tracks_model as tm

NONE = mm.COST_NONE


@pytest.mark.parametrize("name", sorted(mv.BUILDERS))
def test_every_table_is_one_the_tracker_takes(name):
    """bl_obstracks_upload's rule, from the tracker's model: ids, velocities within 1023, px and py within 2^30, hits."""
    case = mv.get(name)
    w = case.world()
    t = tm.Tracker(w.w, w.h, **tm.BASE)
    t.upload(case.slots, 0, int(case.slots["id"].max()) + 1, 1)
    assert len(lmm.used_slots(t.slots)) == len(lmm.used_slots(case.slots)) > 0
    assert case.p.K <= 1024 and case.p.staged(mv.CPM) == (name != "direct_38")


def test_used_slots_in_every_wave_are_each_needed():
    case = mv.get("every_wave")
    costs, fh, _ = mv.samples(case)
    assert 0 < np.count_nonzero(fh) < case.p.K
    kinds = {(int(s["id"]) != 0, int(s["flags"])) for s in case.slots if not lmm.used(s) and (int(s["x1"]) or int(s["flags"]))}
    assert kinds == {(bool(i), f) for _, i, f in mv.UNUSED_KINDS}
    for wave in range(4):                                                       # each kind in each wave, each over the whole grid
        rows = [s for s in case.slots[64 * wave:64 * wave + 64] if not lmm.used(s) and int(s["x1"])]
        assert len(rows) == 4 and all(int(s["x0"]) < 0 and int(s["y0"]) < 0 and int(s["x1"]) >= case.world().w and int(s["y1"]) >= case.world().h for s in rows)
    hitters = mv.first_hitters(case)
    for sl in mv.WAVE_SLOTS:
        c2, f2, _ = mv.samples(case, slots=mv.without(case.slots, sl))
        print("slot", sl, "first hitter of", int((hitters == sl).sum()), "; without it", int((f2 != fh).sum()), "first hits and", int((c2 != costs).sum()), "costs change")
        assert (f2 != fh).any() and (c2 != costs).any(), sl
    vs = case.slots[list(mv.WAVE_SLOTS)]
    assert (vs["vx"] < 0).any() and (vs["vx"] > 0).any() and (vs["vy"] < 0).any() and (vs["vy"] > 0).any() and case.m.lead > 0


def test_full_table_has_many_first_hitters_and_leaves_samples():
    case = mv.get("full_table")
    costs, fh, _ = mv.samples(case)
    hitters = mv.first_hitters(case)
    first = set(hitters[hitters >= 0].tolist())
    print("full table:", len(first), "slots are a first hitter,", int((costs != NONE).sum()), "samples admissible, waves", sorted({s // 64 for s in first}))
    assert len(first) >= 20 and int((costs != NONE).sum()) >= 10 and {s // 64 for s in first} == {0, 1, 2, 3}
    assert (case.slots["vx"] < 0).any() and (case.slots["vx"] > 0).any() and (case.slots["vy"] < 0).any() and (case.slots["vy"] > 0).any()


@pytest.mark.parametrize("name,staged,static_adm", [("direct_38", False, 192), ("staged_37", True, None)])
def test_boxes_refuse_some_admissible_samples_on_both_sides_of_the_window_rule(name, staged, static_adm):
    case = mv.get(name)
    assert case.p.staged(mv.CPM) == staged
    costs, fh, _ = mv.samples(case)
    plain, _, _ = mv.samples(case, slots=None)
    if static_adm is not None:
        assert int((plain != NONE).sum()) == static_adm
    refused = int(((plain != NONE) & (fh > 0)).sum())
    print(name, "statically admissible", int((plain != NONE).sum()), "of those refused by a box", refused, "left", int((costs != NONE).sum()))
    assert refused > 0 and (costs != NONE).any()
    used = lmm.used_slots(case.slots)
    assert all(int(s["vx"]) and int(s["vy"]) for s in used) and set(mv.first_hitters(case).tolist()) == {-1} | {int(s["slot"]) for s in used}
    assert int(mv.plans(case)[0][0]["flags"]) in (0, mm.FELL_BACK)
    assert mv.get("direct_38").slots.tobytes() == mv.get("staged_37").slots.tobytes()


def test_a_box_alone_causes_the_fall_back():
    fell = []
    for seed in range(1, 6):
        for tick in range(12):
            case = mv.box_pillar(seed, tick)
            if int(mv.plans(case)[0][0]["flags"]) == mm.FELL_BACK and int(mv.plans(case, None)[0][0]["flags"]) == 0:
                fell.append((seed, tick))
    print("a box alone falls back at", len(fell), "of 60 (seed, tick)")
    assert (mv.BOX_SEED, mv.BOX_TICK) in fell
    case = mv.get("box_pillar")
    slot = int(lmm.used_slots(case.slots)[0]["slot"])
    assert slot >= 64 and lmm.box_at(case.slots[slot], 1, case.m) == lmm.box_at(case.slots[slot], case.p.n_steps, case.m) == (20, 19, 20, 21)
    r, so, info = mv.plans(case)[0]
    best = int(r["index_best"])
    assert int(r["flags"]) == mm.FELL_BACK and best > 1 and int(r["cost_out"]) == int(r["cost_best"]) and (so == info["seqs"][best]).all()
    assert int(mv.plans(case, None)[0][0]["flags"]) == 0                        # the static call on the same state does not fall back
    _, cfh = mm.seq_costs(case.world(), case.p, case.states[0][0], info["candidate"][None], case.slots, case.m)
    plain, _ = mm.seq_costs(case.world(), case.p, case.states[0][0], info["candidate"][None])
    assert int(cfh[0]) > 0 and int(plain[0]) != NONE                            # the candidate is refused by the box and by nothing else


def test_a_box_beside_the_way_leaves_the_candidate():
    case = mv.get("box_aside")
    r, so, info = mv.plans(case)[0]
    assert int(r["flags"]) == 0 and np.count_nonzero(info["first_hit"]) > 0 and int(lmm.used_slots(case.slots)[0]["slot"]) >= 64
    assert r.tobytes() != mv.plans(case, None)[0][0].tobytes()


def test_first_hits_after_the_map_has_refused():
    case = mv.get("after_the_pillar")
    late = mv.refused_before_hit(case)
    print("refused by the map strictly before the first hit:", int(late.sum()))
    assert int(late.sum()) >= 50
    back = mv.get("out_and_back")
    gone = mv.left_before_hit(back)
    costs, fh, _ = mv.samples(back)
    print("without a cell strictly before the first hit:", int(gone.sum()), "of", int(np.count_nonzero(fh)), "hits")
    assert int(gone.sum()) >= 5 and (costs != NONE).any() and (costs[gone] == NONE).all()


@pytest.mark.parametrize("q,lead,v", mv.TIMINGS)
def test_timings_hit_at_more_than_one_step(q, lead, v):
    case = mv.get("timing_q%d_lead%d_v%d" % (q, lead, v))
    s = lmm.used_slots(case.slots)[0]
    assert (case.m.q, case.m.lead, int(s["vx"]), int(s["vy"])) == (q, lead, v, -v) and case.p.n_steps == 255 and case.p.staged(mv.CPM)
    _, fh, _ = mv.samples(case)
    steps = set(fh[fh > 0].tolist())
    print((q, lead, v), "hits", int(np.count_nonzero(fh)), "first-hit steps", len(steps), "box starts at column", int(s["x0"]))
    assert np.count_nonzero(fh) > 0 and len(steps) >= 2


def test_timings_have_both_signs_and_floor_differs_from_truncation():
    vx = [v for _, _, v in mv.TIMINGS]
    assert min(vx) < 0 < max(vx) and min(-v for v in vx) < 0 < max(-v for v in vx)          # vy = -vx
    assert {q for q, _, _ in mv.TIMINGS} >= {1, 255} and {l for _, l, _ in mv.TIMINGS} >= {0, 255} and max(abs(v) for v in vx) == 1023
    case = mv.get("floor_step")
    q, lead, v = mv.FLOOR_Q, mv.FLOOR_LEAD, mv.FLOOR_VX
    differ = [t for t in range(1 + lead, 256 + lead) if t * v + 128 * q < 0 and (t * v + 128 * q) % (256 * q) and lmm.offset(t, v, q) != mv.trunc_offset(t, v, q)]
    assert v % 2 and len(differ) > 200
    _, fh, _ = mv.samples(case)
    assert np.count_nonzero(fh) > 0 and (mv.first_hits_truncating(case) != fh).any()
    plain = mv.get("timing_q1_lead255_v1023")                                               # a positive velocity: nothing to tell apart
    assert (mv.first_hits_truncating(plain) == mv.samples(plain)[1]).all()


def test_clamped_boxes():
    case = mv.get("everywhere")
    s = lmm.used_slots(case.slots)[0]
    assert (int(s["x0"]), int(s["y0"]), int(s["x1"]), int(s["y1"]), int(s["px"]), int(s["py"]), case.m.margin) == (mv.INT32_MIN, mv.INT32_MIN, mv.INT32_MAX, mv.INT32_MAX, 0, 0, 64)
    r, so, info = mv.plans(case)[0]
    assert int(r["flags"]) == mm.BLOCKED and (mv.samples(case)[1] == 1).all() and not so.any()
    for name, c, v in (("corner_max", mv.INT32_MAX, 1023), ("corner_min", mv.INT32_MIN, -1023)):
        case = mv.get(name)
        s = lmm.used_slots(case.slots)[0]
        assert [int(s[n]) for n in ("x0", "y0", "x1", "y1", "vx", "vy")] == [c, c, c, c, v, v] and (case.m.margin, case.m.lead) == (64, 255)
        assert abs(int(s["px"])) == lmm.POS_MAX and abs(int(s["py"])) == lmm.POS_MAX
        costs, fh, _ = mv.samples(case)
        assert not fh.any() and (costs == mv.samples(case, slots=None)[0]).all()
        wrapped = (c + (64 if c > 0 else -64) + 2 ** 31) % 2 ** 32 - 2 ** 31                 # what 32-bit arithmetic makes of the unclamped sum
        assert (wrapped > 0) != (c > 0)


def test_batch_under_the_rule():
    case = mv.get("batch")
    world = case.world()
    assert world.cell(*case.states[1][0][:2]) == (5, 15) and lmm.in_box(lmm.box_at(case.slots[66], 1, case.m), (5, 15))
    got = mv.plans(case)
    assert [int(r["flags"]) & ~mm.FELL_BACK for r, _, _ in got] == mc.BATCH_FLAGS
    _, fh, _ = mv.samples(case)
    assert np.count_nonzero(fh) > 0                                             # the crossing box meets samples of the normal state
    # under POCKET every admissible sample is on the same cell at every step: no box can change the record and leave the flags
    costs, _, _ = mv.samples(case, slots=None)
    cx, cy, _, _ = mv.cells(case)
    adm = costs != NONE
    assert adm.sum() > 1 and (cx[adm] == cx[adm][0]).all() and (cy[adm] == cy[adm][0]).all()
    assert got[0][0].tobytes() == mv.plans(case, None)[0][0].tobytes()
    # with speeds that differ, the record of the normal state differs from the static call's
    fast = mv.get("batch_speeds")
    assert fast.slots[66].tobytes() == case.slots[66].tobytes() and [s[:3] for s in fast.states] == [s[:3] for s in case.states]
    got = mv.plans(fast)
    assert [int(r["flags"]) & ~mm.FELL_BACK for r, _, _ in got] == mc.BATCH_FLAGS
    plain = mv.plans(fast, None)
    assert got[0][0].tobytes() != plain[0][0].tobytes() and 0 < int(got[0][0]["n_admissible"]) < int(plain[0][0]["n_admissible"])
    print("batch, speeds differ: the normal state's flags", int(got[0][0]["flags"]), "admissible", int(got[0][0]["n_admissible"]), "of", int(plain[0][0]["n_admissible"]))
