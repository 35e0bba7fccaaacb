"""The sampling local planner's model (tests/mppi_model.py) on its own: the weight table, the feasibility of every sequence, the
closed loop on the obstacle map, the search that pins the fall-back case, and the moving rule.  The GPU tests compare the kernels
with the model on these inputs."""
import math

import numpy as np

import local_plan_model as lpm
import local_plan_moving_model as lmm
import moving_plan_loop as ml
import mppi_cases as mc
import mppi_model as mm
import obstacle_tracks_model as tm
import test_local_plan_model_cpu as cpu

F32 = np.float32


def test_weight_table():
    t = mm.weight_table()
    assert len(t) == 257 and t[0] == 1 << 24 and t[256] == 0 and t[16] == 6171987
    assert all(a >= b for a, b in zip(t[:-1], t[1:])) and all(a > b for a, b in zip(t[:229], t[1:230]))
    assert t.index(0) == 230
    assert mm.TABLE_MUL == math.floor(2 ** 32 * math.exp(-1 / 16))
    worst = max(abs(t[i] - round(2 ** 24 * math.exp(-i / 16))) for i in range(129))
    print("weight table: worst distance from round(2^24 e^(-i/16)) for i <= 128:", worst)
    assert worst <= 8


def _feasible(p, seqs, v, w):
    vmin, vmax, wmax, _, _, av, aw = p.derived()
    seqs = np.asarray(seqs, np.int64)
    prev = np.concatenate([np.broadcast_to(np.array([mm.q16(v), mm.q16(w)], np.int64), seqs[:, :1].shape), seqs[:, :-1]], axis=1)
    d = np.abs(seqs - prev)
    return bool((seqs[..., 0] >= vmin).all() and (seqs[..., 0] <= vmax).all() and (np.abs(seqs[..., 1]) <= wmax).all() and
                (d[..., 0] <= av).all() and (d[..., 1] <= aw).all())


def test_every_sample_and_every_output_is_feasible():
    world = cpu.ragged_world()
    changed = 0
    for seed, (v, w) in enumerate([(0.2, -0.3), (0.0, 0.0), (0.5, 2.5), (-0.1, -2.5)]):
        p = mm.Params(**dict(mc.RAGGED, n_samples=257, seed=seed))
        s = mc.ragged_state(world, tick=seed)
        u = mc.nominal(p, seed)
        seqs = mm.sample_seqs(p, v, w, s[3], s[4], u)
        assert _feasible(p, seqs, v, w)
        r, so, info = mm.plan(world, p, s[0], v, w, s[3], s[4], u)
        assert int(r["flags"]) in (0, mm.FELL_BACK) and _feasible(p, so[None], v, w)
        # an average of feasible sequences passes the clamp chain changed by at most one unit per entry
        avg = np.array(mm.average(info["weights"], seqs), np.int64)
        diff = np.abs(mm.clamp_seq(p, avg, v, w) - avg)
        assert diff.max() <= 1
        changed += int(diff.sum())
        rng = np.random.default_rng(seed)
        W = rng.integers(0, 1 << 24, len(seqs)).astype(np.int64)
        avg = np.array(mm.average(W, seqs), np.int64)
        assert np.abs(mm.clamp_seq(p, avg, v, w) - avg).max() <= 1
    print("entries the clamp chain moved by one unit:", changed)
    # a state outside the limits: both bounds become the clamped state, and the chain recovers from there
    p = mm.Params(**mc.RAGGED)
    seqs = mm.sample_seqs(p, 0.9, 5.0, 0, 0)
    assert (seqs[:, 0, 0] == mm.q16(0.5)).all() and (seqs[:, 0, 1] == mm.q16(2.5)).all() and _feasible(p, seqs[:, 1:], 0.5, 2.5)


def test_closed_loop_arrives():
    world = cpu.loop_world()[0]
    p = mm.Params(**mc.LOOP)
    assert p.ok() and not p.can_skip_a_cell(world.mpc)
    recs, seqs, cells = mc.model_loop()
    assert all(c is not None and world.tcell[c[1], c[0]] for c in cells)
    assert int(recs[-1]["flags"]) == mm.REACHED, (len(recs), recs[-1])
    ess = [int(r["weight_sum"]) ** 2 / int(r["weight_sq_sum"]) for r in recs[:-1]]
    fell = sum(int(r["flags"]) == mm.FELL_BACK for r in recs)
    print("closed loop: arrived after %d ticks (cap %d), %d fall-backs, effective sample size S^2/Q min %.1f median %.1f max %.1f of %d" %
          (len(recs) - 1, mc.LOOP_CAP, fell, min(ess), float(np.median(ess)), max(ess), p.K))
    assert len(recs) - 1 <= mc.LOOP_CAP


def test_fall_back_search():
    """Seeds and ticks are searched until the model flags FELL_BACK; mppi_cases pins one of those found."""
    world = mc.pillar_world()
    found = []
    for seed in range(1, 5):
        p = mm.Params(**dict(mc.PILLAR, seed=seed))
        for tick in range(10):
            s = mc.pillar_state(world, tick)
            r, so, info = mm.plan(world, p, s[0], s[1], s[2], s[3], s[4], mc.pillar_nominal(p))
            if int(r["flags"]) == mm.FELL_BACK:
                found.append((seed, tick))
                assert (so == info["seqs"][int(r["index_best"])]).all() and int(r["cost_out"]) == int(r["cost_best"]) == int(info["costs"].min())
                cc, _ = mm.seq_costs(world, p, s[0], info["candidate"][None])
                assert int(cc[0]) == mm.COST_NONE                              # the average goes through the pillar
    print("fall-backs found at (seed, tick):", found[:8], "...", len(found))
    assert (mc.PILLAR_SEED, mc.PILLAR_TICK) in found
    p = mm.Params(**dict(mc.PILLAR, seed=mc.PILLAR_SEED))
    s = mc.pillar_state(world, mc.PILLAR_TICK)
    info = mm.plan(world, p, s[0], s[1], s[2], s[3], s[4], mc.pillar_nominal(p))[2]
    turn = info["seqs"][info["costs"] != mm.COST_NONE][:, :, 1].sum(axis=1)
    assert (turn > 0).any() and (turn < 0).any()                               # admissible samples pass on both sides


def test_crossing_box_loop_drives_through_no_used_box():
    """tests/moving_plan_loop.py's scenario with the sampling planner in the local planner's place."""
    p = mm.Params(**dict(mc.LOOP, n_samples=256))
    st = dict(seq=np.zeros((p.T, 2), np.int32), tick=0, fell=0, checked=0)

    def step(world, slots, m, pose, v, w):
        r, so, info = mm.plan(world, p, pose, v, w, st["tick"], 0, st["seq"], slots, m)
        flags = int(r["flags"])
        if not flags & ~mm.FELL_BACK:
            for k, q in enumerate(mm.drive(pose, so[0], p), 1):
                c = world.cell(q[0], q[1])
                for s in lmm.used_slots(slots):
                    assert not lmm.in_box(lmm.box_at(s, k, m), c), (st["tick"], k, c)
                    st["checked"] += 1
        st["fell"] += flags == mm.FELL_BACK
        st["seq"], st["tick"] = mm.advance(so, flags), st["tick"] + 1
        out = np.zeros((), lpm.RESULT)                                         # what the loop reads: the command and the local planner's flags
        out["trans_v"], out["angular_v"], out["flags"] = r["trans_v"], r["angular_v"], flags & ~mm.FELL_BACK
        return out, (None if info is None else info["first_hit"])

    res = ml.run_loop(step=step)
    print("crossing box: %d ticks, %d steps inside the true box, %d ticks blocked, crossed %s, most samples refused in a tick %d, %d fall-backs, %d box tests" %
          (len(res["recs"]), res["inside"], res["blocked"], res["crossed"], max(res["refused"]), st["fell"], st["checked"]))
    assert int(res["recs"][-1]["flags"]) == lpm.REACHED and res["inside"] == 0 and st["checked"] > 0 and max(res["refused"]) > 0


def moving_case():
    """(world, Params, state, slots with one used box crossing ahead, Moving): the GPU test's case."""
    world = cpu.uniform_world()
    p = mm.Params(**dict(mc.RAGGED, n_samples=257, horizon=10))
    s = (cpu.cell_centre(world, 20, 23) + (F32(0.3),), F32(0.3), F32(0.0), 2, 1)
    slots = lmm.slot_table([lmm.make_slot(1, 26, 18, 28, 22, vx=-100, vy=60), lmm.make_slot(2, 40, 40, 42, 42, flags=tm.CONFIRMED | tm.MATCHED)])
    return world, p, s, slots, lmm.Moving(2, 1, 1)


def test_moving_rule_refuses_samples_and_no_used_slot_is_the_static_model():
    world, p, s, slots, m = moving_case()
    costs, fh, seqs = mm.debug_samples(world, p, s[0], s[1], s[2], s[3], s[4], None, slots, m)
    plain, fh0, _ = mm.debug_samples(world, p, s[0], s[1], s[2], s[3], s[4])
    assert not fh0.any() and 10 < np.count_nonzero(fh) < p.K - 10 and len(set(fh.tolist())) > 3
    assert (costs[fh > 0] == mm.COST_NONE).all() and (costs[fh == 0] == plain[fh == 0]).all() and (plain[fh > 0] != mm.COST_NONE).any()
    r, so, _ = mm.plan(world, p, s[0], s[1], s[2], s[3], s[4], None, slots, m)
    r0, so0, _ = mm.plan(world, p, s[0], s[1], s[2], s[3], s[4])
    assert r.tobytes() != r0.tobytes()
    unused = lmm.slot_table([lmm.make_slot(1, 26, 18, 28, 22, vx=-100, vy=60, flags=tm.CONFIRMED | tm.MOVING)])      # coasting: stale
    assert not lmm.used_slots(unused)
    r1, so1, _ = mm.plan(world, p, s[0], s[1], s[2], s[3], s[4], None, unused, m)
    assert r1.tobytes() == r0.tobytes() and so1.tobytes() == so0.tobytes()
    over = lmm.slot_table([lmm.make_slot(3, 15, 18, 25, 28)])                   # a box over the pose's own cell
    r2, so2, _ = mm.plan(world, p, s[0], s[1], s[2], s[3], s[4], None, over, m)
    assert int(r2["flags"]) == mm.BLOCKED and not so2.any()


def test_parameter_rules():
    assert mm.Params(**mc.LOOP).ok() and mm.Params(**mc.RAGGED).ok() and mm.Params(**mc.PILLAR).ok() and mm.Params(**mc.POCKET).ok()
    for bad in (dict(v_min=0.6), dict(w_max=-0.1), dict(dt_sim=0.0), dict(acc_v=float("nan")), dict(noise_v=-0.1), dict(acc_w=-1.0), dict(w_max=32.0),
                dict(n_samples=0), dict(n_samples=16385), dict(horizon=65), dict(n_sub=17), dict(horizon=32, n_sub=8), dict(lam=0), dict(lam=(1 << 30) + 1),
                dict(w_field=65536), dict(w_clear=-1)):
        assert not mm.Params(**dict(mc.LOOP, **bad)).ok(), bad
    assert mm.q16(0.5) == 32768 and mm.q16(-31.0) == -31 * 65536 and mm.q16(F32(2.5e-6 * 3)) == 0
    assert mm.Params(**dict(mc.LOOP, v_max=1.5)).can_skip_a_cell(0.05) and not mm.Params(**mc.LOOP).can_skip_a_cell(0.05)
