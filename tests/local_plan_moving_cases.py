"""Named inputs for the local planner's moving rule (bl_localplan_commands_moving) and the proof -- on the CPU, from the model
(tests/local_plan_moving_model.py) alone -- that each is what it is named for.  A builder returns a Case and asserts its own
property before it returns; tests/test_local_plan_moving_model_cpu.py counts the conditions, tests/test_gpu_local_plan_moving.py
compares the device with the model on every case, byte for byte.  The grids are 37 x 23 and 64 x 64, free inside a one-cell wall.
"""
import collections
import functools

import numpy as np

import local_plan_cases as lc
import local_plan_model as lpm
import local_plan_moving_model as lmm
import obstacle_tracks_model as tm
import test_local_plan_model_cpu as cpu

F32 = np.float32
CPM = cpu.CPM
USED = tm.CONFIRMED | tm.MOVING | tm.MATCHED
Case = collections.namedtuple("Case", "world p states slots m note")


@functools.lru_cache(maxsize=None)
def small_world():
    return cpu.make_world(cpu.uniform_cells(37, 23), cpu.ORIGIN, cpu.MPC, [(30, 11)], 0, cpu.SMALL_NAV)[0]


@functools.lru_cache(maxsize=None)
def square_world():
    return cpu.make_world(cpu.uniform_cells(64, 64), cpu.ORIGIN, cpu.MPC, [(55, 32)], 0, cpu.SMALL_NAV)[0]


BASE = dict(v_min=0.0, v_max=0.5, w_max=2.0, acc_v=10.0, acc_w=30.0, dt_control=0.1, dt_sim=0.05, w_field=3, w_heading=1, w_clear=1, w_speed=2)
ONE = dict(BASE, n_v=1, n_w=1, n_steps=1)                    # a single candidate with a single cell
FAN = dict(BASE, n_v=3, n_w=9, n_steps=20)
SAME_SPEED = dict(BASE, v_min=0.5, n_v=1, n_w=9, n_steps=20)  # nine headings at one speed
START = (8.3, 11.4, 0.0)                                     # grid coordinates and heading, small world
V0, W0 = F32(0.25), F32(0.0)


def P(**kw):
    return lc._P(**kw)


def start(world, at=START):
    return (lc.on_cell(world, *at), V0, W0)


@functools.lru_cache(maxsize=None)
def cells(world_factory, p, state):
    return lmm.cells_of(world_factory(), p, *state)


def timed_box(world_factory, p, state, c, k, m, vx=0, vy=0, size=(1, 1), id=1, flags=USED):
    """A slot whose box, at rollout step k, has its low corner on candidate c's cell of step k."""
    cell = cells(world_factory, p, state)[c][k - 1]
    assert cell is not None
    ox, oy = lmm.offset(k + m.lead, vx, m.q), lmm.offset(k + m.lead, vy, m.q)
    x0, y0 = cell[0] - ox, cell[1] - oy
    return lmm.make_slot(id, x0, y0, x0 + size[0] - 1, y0 + size[1] - 1, vx, vy, flags)


@functools.lru_cache(maxsize=None)
def model(name):
    """[(record, costs, first_hit)] of a case's states, once; costs and first_hit also for a flagged state."""
    case = get(name)
    world, out = case.world(), []
    for s in case.states:
        rec, cs, fh = lmm.command_moving(world, case.p, case.slots, case.m, *s)
        if cs is None:
            cs, fh = lmm.costs_moving(world, case.p, case.slots, case.m, *s)
        out.append((rec, cs, fh))
    return out


def _case(world, p, states, records, m, note=""):
    assert p.ok() and m.ok() and not p.can_skip_a_cell(cpu.MPC)
    return Case(world, p, list(states), lmm.slot_table(records), m, note)


# ---------------------------------------------------------------------------------------------------------------- builders
def no_used():
    return _case(small_world, P(**FAN), [start(small_world())], [], lmm.Moving(2))


def unused_kinds():
    """One slot each unconfirmed, not moving, coasting and free, every one a box over the whole grid."""
    kinds = [tm.MOVING | tm.MATCHED, tm.CONFIRMED | tm.MATCHED, tm.CONFIRMED | tm.MOVING, USED]
    recs = {3 + i: lmm.make_slot(0 if i == 3 else i + 1, -5, -5, 50, 50, 40, -40, f) for i, f in enumerate(kinds)}
    case = _case(small_world, P(**FAN), [start(small_world())], recs, lmm.Moving(2, 1))
    assert not lmm.used_slots(case.slots)
    return case


def born_used():
    """A blob born by a real update with confirm_hits = 1 and min_speed = 0: BORN | CONFIRMED | MOVING at once, and used."""
    w = small_world()
    t = tm.Tracker(w.w, w.h, **dict(tm.BASE, confirm_hits=1, min_speed=0))
    live = np.zeros((w.h, w.w), bool)
    live[10:13, 12:14] = True
    t.update(live, 1)
    us = lmm.used_slots(t.slots)
    assert len(us) == 1 and int(us[0]["flags"]) == tm.BORN | tm.CONFIRMED | tm.MOVING and int(us[0]["hits"]) == 1
    return _case(small_world, P(**FAN), [start(w)], list(t.slots), lmm.Moving(2))


def _straight(p):
    return (p.n_w // 2) * p.n_v + p.n_v - 1                  # w = 0 at the highest speed


def entry(k):
    """A 1 x 1 box running up a column at a cell per step that is on the straight candidate's cell of step k at step k, and at no
    other step on any cell of it.  k = n_steps + 1 is looked up with one step more; it does not block."""
    p, m = P(**FAN), lmm.Moving(1)
    st = start(small_world())
    c = _straight(p)
    pk = P(**dict(FAN, n_steps=k)) if k > p.n_steps else p
    case = _case(small_world, p, [st], [timed_box(small_world, pk, st, c, k, m, 0, 256)], m)
    return case


def edge(margin, side, on):
    """The single candidate's single cell on the box's edge `side` widened by the margin (on), or one cell beyond it."""
    p, m = P(**ONE), lmm.Moving(2, margin)
    st = start(small_world())
    ex, ey = cells(small_world, p, st)[0][0]
    d = 0 if on else 1
    x0, y0 = {"left": (ex + margin + d, ey - 1), "right": (ex - margin - d - 2, ey - 1), "bottom": (ex - 1, ey + margin + d),
              "top": (ex - 1, ey - margin - d - 1)}[side]
    return _case(small_world, p, [st], [lmm.make_slot(7, x0, y0, x0 + 2, y0 + 1)], m)


def floor_not_truncation(axis):
    """q = 2, t = 1, v = -300: t v + 128 q = -44, whose floor over 512 is -1 and whose truncation is 0.  The box stands one cell
    beyond the candidate's cell and is on it only when the offset is -1."""
    p, m = P(**ONE), lmm.Moving(2)
    st = start(small_world())
    ex, ey = cells(small_world, p, st)[0][0]
    assert (1 * -300 + 128 * 2) % (256 * 2) != 0 and lmm.offset(1, -300, 2) == -1 and int((1 * -300 + 128 * 2) / 512) == 0
    rec = lmm.make_slot(2, ex + 1, ey, ex + 1, ey, -300, 0) if axis == "x" else lmm.make_slot(2, ex, ey + 1, ex, ey + 1, 0, -300)
    return _case(small_world, p, [st], [rec], m)


def timing(q, lead, vx, vy, k=13):
    """A 2 x 2 box that reaches the straight candidate's cell of step k at step k under (q, lead) and the given velocity."""
    p, m = P(**FAN), lmm.Moving(q, 0, lead)
    st = start(small_world())
    return _case(small_world, p, [st], [timed_box(small_world, p, st, _straight(p), k, m, vx, vy, (2, 2))], m)


def beyond_int16():
    """Boxes whose clamped coordinates do not fit 16 bits: a half plane from far left up to the column before the straight
    candidate's cell of step 15, a full-height strip far to the right, and one from beyond 2^30."""
    p, m = P(**FAN), lmm.Moving(2)
    st = start(small_world())
    cx = cells(small_world, p, st)[_straight(p)][14][0]
    recs = [lmm.make_slot(1, -2 ** 31, -40000, 4, 40000, 16, 0), lmm.make_slot(2, 40000, -70000, 2 ** 31 - 1, 70000, -1023, 0),
            lmm.make_slot(3, cx, -2 ** 31, cx, 2 ** 31 - 1, 0, 1023)]
    return _case(small_world, p, [st], recs, m)


def own_cell():
    p, m = P(**FAN), lmm.Moving(2)
    st = start(small_world())
    return _case(small_world, p, [st], [lmm.make_slot(1, 2, 5, 16, 17, 30, 0)], m)


def _end_boxes(p, st, spare):
    """1 x 1 boxes that do not move (MOVING by their flag) on the end cells of every candidate but those in `spare`."""
    cs = cells(small_world, p, st)
    keep = set()
    for c in spare:
        keep |= set(cs[c])
    recs = []
    for c, row in enumerate(cs):
        if c in spare:
            continue
        assert row[-1] not in keep
        recs.append(lmm.make_slot(len(recs) + 1, row[-1][0], row[-1][1], row[-1][0], row[-1][1]))
    return recs


def all_but_one():
    p, m = P(**SAME_SPEED), lmm.Moving(2)
    st = start(small_world())
    return _case(small_world, p, [st], _end_boxes(p, st, {6}), m, note=6)


def tie():
    """No weights: every admissible candidate costs 0.  Candidates 0 and 1 are blocked; 2 and 5 are left and tie."""
    p, m = P(**dict(SAME_SPEED, w_field=0, w_heading=0, w_clear=0, w_speed=0)), lmm.Moving(2)
    st = start(small_world())
    return _case(small_world, p, [st], _end_boxes(p, st, {2, 5}), m, note=2)


def full_table(seed=5):
    """256 used slots, scattered in and around the grid, every velocity up to the limit."""
    rng = np.random.default_rng(seed)
    recs = []
    for i in range(tm.MAX_TRACKS):
        x0, y0 = int(rng.integers(-40, 80)), int(rng.integers(-40, 60))
        if abs(x0 - 8) < 4 and abs(y0 - 11) < 4:
            x0 += 40
        recs.append(lmm.make_slot(i + 1, x0, y0, x0 + int(rng.integers(0, 2)), y0 + int(rng.integers(0, 2)), int(rng.integers(-1023, 1024)),
                                  int(rng.integers(-1023, 1024)), tm.CONFIRMED | tm.MOVING | (tm.BORN if i % 3 == 0 else tm.MATCHED)))
    return _case(small_world, P(**FAN), [start(small_world())], recs, lmm.Moving(7, 1, 3))


# ---- the device's paths: the number of kept boxes around BL_LOCALPLAN_MOVING_BYTES, the window staged or not
TABLE_FITS = lmm.MOVING_BYTES // (255 * 8)                   # kept boxes whose 255 steps fit the table


def table_side(kept, v_max):
    """`kept` slow boxes near the start on the 64 x 64 grid, 255 steps; v_max 0.1 stages the window, 1.0 does not."""
    p, m = P(**dict(BASE, v_max=v_max, n_v=3, n_w=9, n_steps=255)), lmm.Moving(2)
    w = square_world()
    st = start(w, (10.3, 32.4, 0.0))
    recs = [lmm.make_slot(i + 1, 14 + 2 * (i % 4), 31 + 3 * (i // 4), 14 + 2 * (i % 4), 32 + 3 * (i // 4), -6, 9 * (1 if i % 2 else -1)) for i in range(kept)]
    case = _case(square_world, p, [st], recs, m)
    assert p.staged(CPM) == (v_max == 0.1)
    assert len(lmm.kept_slots(w, p, case.slots, m, st[0])) == kept
    assert lmm.moving_path(w, p, case.slots, m, st[0]) == (2 if kept == 0 else 0 if kept <= TABLE_FITS else 1)
    return case


def reach_cull():
    """Used slots: one whose sweep ends one cell short of the reach square (culled), one whose sweep touches its border."""
    p, m = P(**FAN), lmm.Moving(2)
    w = square_world()
    st = start(w, (20.3, 32.4, 0.0))
    R = lmm.reach(p, CPM)
    far = lmm.make_slot(1, 20 + R + 5, 30, 20 + R + 6, 33, -102, 0)      # t = 20: floor((20 * -102 + 256) / 512) = -4: x0 ends at R + 1
    near = lmm.make_slot(2, 20 + R + 4, 30, 20 + R + 5, 33, -102, 0)
    inside = timed_box(square_world, p, st, _straight(p), 14, m, -102, 60, (2, 2), id=3)    # and one well inside, which refuses something
    case = _case(square_world, p, [st], [far, near, inside], m)
    assert lmm.box_at(far, 20, m)[0] == 20 + R + 1 and lmm.box_at(near, 20, m)[0] == 20 + R
    kept = lmm.kept_slots(w, p, case.slots, m, st[0])
    assert len(lmm.used_slots(case.slots)) == 3 and [int(s["id"]) for s in kept] == [2, 3]
    return case


def seven_states():
    """Seven states in one call on the 64 x 64 grid: their kept sets differ (0, 1, 2 and 3 boxes within reach), one stands on the
    goal (REACHED), one off the grid (OFF_FIELD), one inside a box (BLOCKED)."""
    p, m = P(**dict(BASE, n_v=5, n_w=9, n_steps=20)), lmm.Moving(2, 1)
    w = square_world()
    recs = [lmm.make_slot(1, 14, 30, 15, 31, 40, 30), lmm.make_slot(2, 18, 36, 18, 38, -60, -80), lmm.make_slot(3, 40, 10, 42, 11, 0, 200),
            lmm.make_slot(4, 44, 50, 45, 52, 100, -100)]
    ats = [(10.3, 32.4, 0.0), (40.6, 16.2, 1.0), (12.5, 50.5, -0.5), (55.5, 32.5, 2.0), (-3.0, 10.0, 0.0), (30.4, 31.7, 3.0), (14.5, 30.5, 0.3)]
    states = [start(w, a) for a in ats]
    case = _case(square_world, p, states, recs, m)
    kept = [len(lmm.kept_slots(w, p, case.slots, m, s[0])) for s in states]
    assert len(set(kept)) >= 3, kept
    return case


def partial_last_workgroup():
    """n_v = 5 and n_w = 65 at 20 steps: 32 headings per workgroup, three workgroups, the last with one heading."""
    p, m = P(**dict(BASE, n_v=5, n_w=65, n_steps=20)), lmm.Moving(2)
    assert lc.launch_shape(p) == (8, 32, 3, 1)
    st = start(small_world())
    recs = [timed_box(small_world, p, st, 64 * 5 + 4, 9, m, -90, 120, (2, 2)), timed_box(small_world, p, st, 3, 17, m, 200, 0, (1, 3), id=2)]
    return _case(small_world, p, [st], recs, m)


BUILDERS = {"no_used": no_used, "unused_kinds": unused_kinds, "born_used": born_used, "entry_1": lambda: entry(1), "entry_n": lambda: entry(20),
            "entry_n_plus_1": lambda: entry(21), "floor_x": lambda: floor_not_truncation("x"), "floor_y": lambda: floor_not_truncation("y"),
            "q_1": lambda: timing(1, 0, 130, -77), "q_255": lambda: timing(255, 0, -1000, 900), "lead_255": lambda: timing(2, 255, -35, 61),
            "lead_0_q_3": lambda: timing(3, 0, 500, 333), "v_1023": lambda: timing(2, 0, 1023, -1023), "v_1023_q_1_lead_255": lambda: timing(1, 255, -1023, 1023),
            "beyond_int16": beyond_int16, "own_cell": own_cell, "all_but_one": all_but_one, "tie": tie, "full_table": full_table,
            "reach_cull": reach_cull, "seven_states": seven_states, "partial_last_workgroup": partial_last_workgroup}
EDGES = [(mg, side, on) for mg in (0, 1, 64) for side in ("left", "right", "bottom", "top") for on in (True, False)]
for _mg, _side, _on in EDGES:
    BUILDERS["edge_%d_%s_%s" % (_mg, _side, "on" if _on else "beyond")] = functools.partial(edge, _mg, _side, _on)
TABLE_SIDES = [(kept, v) for kept in (0, TABLE_FITS, TABLE_FITS + 1) for v in (0.1, 1.0)]
for _kept, _v in TABLE_SIDES:
    BUILDERS["table_%d_%s" % (_kept, "staged" if _v == 0.1 else "grids")] = functools.partial(table_side, _kept, _v)


@functools.lru_cache(maxsize=None)
def get(name):
    return BUILDERS[name]()


# ---------------------------------------------------------------------------------------------------------------- refusals
def refusals():
    """The twelve argument refusals: name -> (Params, Moving, tracker shape, states).  The world is the small one."""
    w = small_world()
    good, st = P(**FAN), start(w)
    shape = (w.w, w.h)
    bad_m = dict(q_0=lmm.Moving(0), q_256=lmm.Moving(256), margin_minus=lmm.Moving(2, -1), margin_65=lmm.Moving(2, 65), lead_minus=lmm.Moving(2, 0, -1),
                 lead_256=lmm.Moving(2, 0, 256), reserved=lmm.Moving(2, 0, 0, 1))
    out = {k: (good, m, shape, [st]) for k, m in bad_m.items()}
    out["tracker_wider"] = (good, lmm.Moving(2), (w.w + 1, w.h), [st])
    out["tracker_taller"] = (good, lmm.Moving(2), (w.w, w.h + 1), [st])
    out["step_skips_a_cell"] = (P(**dict(FAN, v_max=1.5)), lmm.Moving(2), shape, [st])
    out["state_not_finite"] = (good, lmm.Moving(2), shape, [((F32("nan"), F32(0), F32(0)), V0, W0)])
    out["theta_beyond_limit"] = (good, lmm.Moving(2), shape, [((st[0][0], st[0][1], F32(70000.0)), V0, W0)])
    assert len(out) == 12
    return out


# ---------------------------------------------------------------------------------------------------------------- compose_static
def blob_scene(w, h):
    """Live cells of two 3 x 3 blobs per update on a w x h grid: one that moves a cell per update along x, one that stands."""
    def live_at(n):
        live = np.zeros((h, w), bool)
        live[5:8, 3 + n:6 + n] = True
        live[h - 8:h - 5, w - 9:w - 6] = True
        return live
    return live_at
