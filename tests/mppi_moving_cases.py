"""Named inputs for the sampling local planner's moving rule (bl_mppi_plan and bl_mppi_debug_samples with a tracker): used slots in
every wave of the slot table, the grids read directly with the rule on, a fall-back that a box alone causes, first hits after the map
has refused, the ends of (steps_per_update, lead_steps, velocity), clamped boxes and a mixed batch.  A builder returns a Case;
tests/test_mppi_moving_cases_cpu.py proves from the model (tests/mppi_model.py) alone that each case reaches the path it is named for,
tests/test_gpu_mppi_moving_edges.py compares the device with the model on every case, byte for byte.
"""
import collections
import functools

import numpy as np

import local_plan_moving_model as lmm
import mppi_cases as mc
import mppi_model as mm
import obstacle_tracks_model as tm
import test_local_plan_model_cpu as cpu

F32 = np.float32
CPM = cpu.CPM
USED = tm.CONFIRMED | tm.MOVING | tm.MATCHED
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
# world: a factory; states: (pose, v, w, tick, stream) each; u_in: int32 [n, T, 2] or None; slots: all 256 records; m: lmm.Moving
Case = collections.namedtuple("Case", "world p states u_in slots m")

# test_gpu_mppi_edges.py's FAST: up to a cell per step, four steps per period
FAST = dict(mc.RAGGED, v_min=0.0, v_max=1.0, acc_v=10.0, acc_w=30.0, w_max=3.0, horizon=10, n_sub=4, n_samples=257, noise_v=0.5, noise_w=3.0)


def _case(world, p, states, u_in, records, m):
    assert p.ok() and m.ok() and not p.can_skip_a_cell(cpu.MPC) and all(mm.state_ok(s[0], s[1], s[2]) for s in states)
    u = None if u_in is None else np.ascontiguousarray(u_in, np.int32).reshape(len(states), p.T, 2)
    return Case(world, p, list(states), u, lmm.slot_table(records), m)


# ---------------------------------------------------------------------------------------------------------------- what the conditions read
def samples(case, i=0, slots="case"):
    """(costs, first_hit, seqs) of state i's samples in the model; slots: the case's table, or another one (None: the static call)."""
    s = case.states[i]
    return mm.debug_samples(case.world(), case.p, s[0], s[1], s[2], s[3], s[4], None if case.u_in is None else case.u_in[i],
                            case.slots if isinstance(slots, str) else slots, case.m)


def plans(case, slots="case"):
    """[(record, seq_out, info)] of the case's states in the model."""
    sl = case.slots if isinstance(slots, str) else slots
    return [mm.plan(case.world(), case.p, s[0], s[1], s[2], s[3], s[4], None if case.u_in is None else case.u_in[i], sl, case.m)
            for i, s in enumerate(case.states)]


def cells(case, i=0, seqs=None):
    """(cx, cy, inside, trav) [K, n_steps] of state i's samples (or of `seqs`): the visited cells, where the pose has one, and where
    that cell is traversable."""
    s, world = case.states[i], case.world()
    if seqs is None:
        seqs = mm.sample_seqs(case.p, s[1], s[2], s[3], s[4], None if case.u_in is None else case.u_in[i])
    _, _, _, cx, cy, inside = mm.rollouts(world, case.p, s[0], seqs)
    return cx, cy, inside, inside & world.tcell[cy, cx].astype(bool)


def without(slots, index):
    """The table with slot `index` emptied."""
    out = slots.copy()
    out[index] = np.zeros((), tm.TRACK_DTYPE)
    out["slot"][index] = index
    return out


def first_hitters(case, i=0):
    """int [K]: the lowest used slot index whose box holds the sample's cell at its first hit, -1 where there is no hit."""
    _, fh, _ = samples(case, i)
    cx, cy, _, _ = cells(case, i)
    out = np.full(len(fh), -1, np.int64)
    used = [int(s["slot"]) for s in lmm.used_slots(case.slots)]
    for k in np.flatnonzero(fh):
        step = int(fh[k])
        cell = (int(cx[k, step - 1]), int(cy[k, step - 1]))
        out[k] = next(sl for sl in used if lmm.in_box(lmm.box_at(case.slots[sl], step, case.m), cell))
    return out


def trunc_offset(t, v, q):
    """The offset with the division rounding towards zero: what the rule is not."""
    n = t * v + 128 * q
    return abs(n) // (256 * q) * (1 if n >= 0 else -1)


def first_hits_truncating(case, i=0):
    """mm.first_hits with trunc_offset in the floor's place."""
    cx, cy, inside, _ = cells(case, i)
    out = np.zeros(cx.shape[0], np.int32)
    m = case.m
    for k in range(case.p.n_steps, 0, -1):
        hit = np.zeros(cx.shape[0], bool)
        for s in lmm.used_slots(case.slots):
            c = [tm.clamp(int(s[n]), -lmm.POS_MAX, lmm.POS_MAX) for n in ("x0", "y0", "x1", "y1")]
            ox, oy = trunc_offset(k + m.lead, int(s["vx"]), m.q), trunc_offset(k + m.lead, int(s["vy"]), m.q)
            hit |= (inside[:, k - 1] & (cx[:, k - 1] >= c[0] + ox - m.margin) & (cx[:, k - 1] <= c[2] + ox + m.margin) &
                    (cy[:, k - 1] >= c[1] + oy - m.margin) & (cy[:, k - 1] <= c[3] + oy + m.margin))
        out[hit] = k
    return out


def timed(cell, k, m, vx, vy, size=(1, 1), id=1, flags=USED):
    """A slot whose box has its low corner on `cell` at rollout step k."""
    ox, oy = lmm.offset(k + m.lead, vx, m.q), lmm.offset(k + m.lead, vy, m.q)
    x0, y0 = cell[0] - ox, cell[1] - oy
    return lmm.make_slot(id, x0, y0, x0 + size[0] - 1, y0 + size[1] - 1, vx, vy, flags)


# ---------------------------------------------------------------------------------------------------------------- 1. slots in every wave
WAVE_SLOTS = (0, 63, 64, 127, 128, 191, 192, 255)            # the first and the last lane of each of the four waves
UNUSED_KINDS = (("free", 0, USED), ("coasting", 1, tm.CONFIRMED | tm.MOVING), ("unconfirmed", 1, tm.MOVING | tm.MATCHED),
                ("at rest", 1, tm.CONFIRMED | tm.BORN))


def fan_state(world):
    """From cell (8, 18) of cpu.open_world() at 0.8 m/s, the nominal 0.5 m/s straight ahead: the samples fan out over the grid."""
    p = mm.Params(**FAST)
    return (cpu.cell_centre(world, 8, 18) + (F32(0.0),), F32(0.8), F32(0.0), 1, 2), np.tile(np.array([[mm.q16(0.5), 0]], np.int32), (p.T, 1))


def _scatter(rng, n, m, few, many):
    """n used records from `rng`: a 1 x 1 to 2 x 2 box with any velocity that stands on the cell of a random sample at a random step,
    redrawn until, alone in the table, it would refuse at least `few` and at most `many` of the fan's samples."""
    world, p = cpu.open_world(), mm.Params(**FAST)
    s, u = fan_state(world)
    _, _, _, cx, cy, inside = mm.rollouts(world, p, s[0], mm.sample_seqs(p, s[1], s[2], s[3], s[4], u))
    recs = []
    while len(recs) < n:
        vx, vy = int(rng.integers(-1023, 1024)), int(rng.integers(-1023, 1024))
        size = (int(rng.integers(1, 3)), int(rng.integers(1, 3)))
        j, k = int(rng.integers(2, p.K)), int(rng.integers(10, p.n_steps + 1))
        r = timed((int(cx[j, k - 1]), int(cy[j, k - 1])), k, m, vx, vy, size, id=len(recs) + 1,
                  flags=tm.CONFIRMED | tm.MOVING | (tm.BORN if len(recs) % 3 == 0 else tm.MATCHED))
        if few <= np.count_nonzero(mm.first_hits(p, lmm.slot_table([r]), m, cx, cy, inside)) <= many:
            recs.append(r)
    return recs


def every_wave(seed=1):
    """A used slot on the first and on the last lane of every wave, each a small box that other samples of the fan meet, and in
    every wave one unused record of each kind whose box covers the whole grid."""
    world = cpu.open_world()
    p, m = mm.Params(**FAST), lmm.Moving(2, 0, 1)
    recs = dict(zip(WAVE_SLOTS, _scatter(np.random.default_rng(seed), len(WAVE_SLOTS), m, 6, 20)))
    for wave in range(4):
        for n, (_, has_id, flags) in enumerate(UNUSED_KINDS):
            recs[64 * wave + 9 + 13 * n] = lmm.make_slot((100 + 4 * wave + n) * has_id, -5, -5, world.w + 5, world.h + 5, 40, -40, flags)
    s, u = fan_state(world)
    case = _case(cpu.open_world, p, [s], u[None], recs, m)
    assert [int(r["slot"]) for r in lmm.used_slots(case.slots)] == list(WAVE_SLOTS)
    return case


def full_table(seed=5):
    """All 256 slots used, from a fixed seed: small boxes, velocities of both signs up to the limit."""
    world = cpu.open_world()
    p, m = mm.Params(**FAST), lmm.Moving(3, 0, 2)
    s, u = fan_state(world)
    case = _case(cpu.open_world, p, [s], u[None], _scatter(np.random.default_rng(seed), tm.MAX_TRACKS, m, 1, 8), m)
    assert len(lmm.used_slots(case.slots)) == tm.MAX_TRACKS
    return case


# ---------------------------------------------------------------------------------------------------------------- 2. grids read directly
DIRECT = dict(mc.RAGGED, horizon=38, n_sub=4, v_max=0.5, acc_w=2.0, acc_v=0.3, n_samples=257)


def direct_reads(horizon):
    """The ragged world with 4 * horizon steps: 38 periods do not fit the staged window, 37 do.  Three used boxes cross the fan."""
    world = cpu.ragged_world()
    p, m = mm.Params(**dict(DIRECT, horizon=horizon)), lmm.Moving(4, 1, 2)
    recs = {3: timed((30, 57), 80, m, -60, 45, (2, 3), id=1), 70: timed((22, 62), 120, m, 50, -30, (3, 2), id=2),
            200: timed((31, 55), 40, m, 25, 20, (1, 2), id=3)}
    case = _case(cpu.ragged_world, p, [mc.ragged_state(world)], mc.nominal(p)[None], recs, m)
    assert p.staged(CPM) == (horizon <= 37)
    return case


# ---------------------------------------------------------------------------------------------------------------- 3. a box alone falls back
BOX_SEED, BOX_TICK = 3, 7                                    # test_mppi_moving_cases_cpu pins these from the sixty that fall back


@functools.lru_cache(maxsize=None)
def room_world():
    """mc.pillar_world() without the pillar."""
    return cpu.make_world(cpu.uniform_cells(47, 41), cpu.ORIGIN, cpu.MPC, [mc.PILLAR_GOAL], 0, cpu.SMALL_NAV)[0]


def box_pillar(seed=BOX_SEED, tick=BOX_TICK, slot=77):
    """The empty room with the pillar's three cells as a used box at rest, in a slot of the second wave."""
    world = room_world()
    p, m = mm.Params(**dict(mc.PILLAR, seed=seed)), lmm.Moving(2, 0, 0)
    return _case(room_world, p, [mc.pillar_state(world, tick)], mc.pillar_nominal(p)[None], {slot: lmm.make_slot(5, 20, 19, 20, 21)}, m)


def box_aside(seed=BOX_SEED, tick=BOX_TICK, slot=130):
    """The same room and state with a box beside the way: it refuses samples and leaves the candidate admissible."""
    world = room_world()
    p, m = mm.Params(**dict(mc.PILLAR, seed=seed)), lmm.Moving(2, 0, 0)
    return _case(room_world, p, [mc.pillar_state(world, tick)], mc.pillar_nominal(p)[None], {slot: lmm.make_slot(5, 16, 23, 22, 24, 0, 12)}, m)


# ---------------------------------------------------------------------------------------------------------------- 4. first hit after a refusal
def after_the_pillar():
    """mc.pillar_world() with a used box beyond the pillar: samples that the pillar refuses go on into the box."""
    world = mc.pillar_world()
    p, m = mm.Params(**dict(mc.PILLAR, seed=3, horizon=12, n_samples=257)), lmm.Moving(2, 0, 0)
    return _case(mc.pillar_world, p, [mc.pillar_state(world, 7)], mc.pillar_nominal(p)[None], [lmm.make_slot(1, 22, 10, 24, 30)], m)


def out_and_back(seed=1):
    """cpu.open_world() from cell (6, 1), heading out over the bottom border at 0.2 rad while turning back in: samples leave the grid
    and have a cell again some steps later, and a used box lies along the border where they come back."""
    world = cpu.open_world()
    p, m = mm.Params(**dict(FAST, seed=seed)), lmm.Moving(2, 0, 1)
    s = (cpu.cell_centre(world, 6, 1) + (F32(-0.2),), F32(0.8), F32(0.0), 1, 2)
    u = np.tile(np.array([[mm.q16(0.8), mm.q16(0.6)]], np.int32), (p.T, 1))
    return _case(cpu.open_world, p, [s], u[None], {129: lmm.make_slot(1, 16, -3, 45, 0, -20, 6)}, m)


def refused_before_hit(case, i=0):
    """bool [K]: the map refused the sample (no cell, or a cell that is not traversable) at a step strictly before its first hit."""
    _, fh, _ = samples(case, i)
    _, _, _, trav = cells(case, i)
    first_bad = np.where((~trav).any(axis=1), (~trav).argmax(axis=1) + 1, case.p.n_steps + 1)
    return (fh > 0) & (first_bad < fh)


def left_before_hit(case, i=0):
    """bool [K]: the pose had no cell at a step strictly before the sample's first hit."""
    _, fh, _ = samples(case, i)
    _, _, inside, _ = cells(case, i)
    first_out = np.where((~inside).any(axis=1), (~inside).argmax(axis=1) + 1, case.p.n_steps + 1)
    return (fh > 0) & (first_out < fh)


# ---------------------------------------------------------------------------------------------------------------- 5. time, divisor, sign
LONG = dict(mc.RAGGED, horizon=17, n_sub=15, v_max=0.1, n_samples=257)
TIMINGS = ((1, 255, 1023), (1, 255, -1023), (255, 255, 1023), (255, 0, -1023), (7, 100, 1023))


def _median_column(p, s, world, k):
    seqs = mm.sample_seqs(p, s[1], s[2], s[3], s[4])
    _, _, _, cx, _, _ = mm.rollouts(world, p, s[0], seqs)
    return int(np.median(cx[:, k - 1]))


def timing(q, lead, v, vy=None):
    """255 steps, staged.  One tall used box with vx = v and vy = -v, as wide as it moves in a step (four cells at q = 1, else one),
    whose offset at step 128 puts its first column on the samples' median column."""
    world = cpu.ragged_world()
    p, m = mm.Params(**LONG), lmm.Moving(q, 0, lead)
    s = mc.ragged_state(world)
    vy = -v if vy is None else vy
    col = _median_column(p, s, world, 128)
    x0, width = col - lmm.offset(128 + lead, v, q), -(-abs(v) // (256 * q))
    case = _case(cpu.ragged_world, p, [s], None, [lmm.make_slot(1, x0, -4000, x0 + width - 1, 4000, v, vy)], m)
    assert p.n_steps == 255 and p.staged(CPM)
    return case


FLOOR_Q, FLOOR_LEAD, FLOOR_VX = 3, 0, -77


def floor_step():
    """vx odd and negative: t vx + 128 q is negative and no multiple of 256 q at most steps, so floor and truncation differ there."""
    return timing(FLOOR_Q, FLOOR_LEAD, FLOOR_VX, vy=0)


# ---------------------------------------------------------------------------------------------------------------- 6. clamp and margin
def _plain_state():
    """test_mppi_model_cpu.moving_case()'s world, parameters and state."""
    world = cpu.uniform_world()
    return world, mm.Params(**dict(mc.RAGGED, n_samples=257, horizon=10)), (cpu.cell_centre(world, 20, 23) + (F32(0.3),), F32(0.3), F32(0.0), 2, 1)


def everywhere():
    """x0 = y0 = INT32_MIN, x1 = y1 = INT32_MAX, margin 64: the clamped box holds every cell at every step."""
    _, p, s = _plain_state()
    rec = lmm.make_slot(1, INT32_MIN, INT32_MIN, INT32_MAX, INT32_MAX)
    assert int(rec["px"]) == 0 and int(rec["py"]) == 0
    return _case(cpu.uniform_world, p, [s], None, {191: rec}, lmm.Moving(2, 64, 0))


def corner(sign):
    """A 1 x 1 box at (INT32_MAX, INT32_MAX) running outwards at 1023, or at (INT32_MIN, INT32_MIN) at -1023, margin 64, lead 255:
    2^30 + 64 + 2040 fits an int, INT32_MAX + 64 does not."""
    _, p, s = _plain_state()
    c = INT32_MAX if sign > 0 else INT32_MIN
    return _case(cpu.uniform_world, p, [s], None, {64: lmm.make_slot(1, c, c, c, c, 1023 * sign, 1023 * sign)}, lmm.Moving(1, 64, 255))


# ---------------------------------------------------------------------------------------------------------------- 7. batch under the rule
def batch(acc_v=0.0, cross=((6, 15), 12)):
    """mc.batch_states() with a box that stands over the REACHED pose's cell (5, 15) when the call is made and has moved off the
    corridor by step 4, and a 1 x 1 box that crosses the corridor ahead of the normal state.  Under mc.POCKET (acc_v = 0) every sample
    drives at 0.4 m/s and the corridor is one cell wide, so the admissible samples and the candidate visit the same cell at every step: a
    box refuses all of them or none, and the record of the normal state cannot differ from the static call's while its flags stay 0.
    The crossing box of that case refuses samples the walls refuse as well.  acc_v = 2 lets the speeds differ, and there a box on
    cell (8, 15) at step 5 refuses some admissible samples and the candidate."""
    p, m = mm.Params(**dict(mc.POCKET, acc_v=acc_v)), lmm.Moving(2, 0, 1)
    recs = {66: lmm.make_slot(1, 5, 14, 5, 15, 0, -64), 190: timed(cross[0], cross[1], m, 0, 256, id=2)}
    assert lmm.in_box(lmm.box_at(recs[66], 1, m), (5, 15)) and lmm.box_at(recs[66], 4, m)[3] < 15
    return _case(cpu.pocket_world, p, mc.batch_states(), None, recs, m)


BUILDERS = {"every_wave": every_wave, "full_table": full_table, "direct_38": lambda: direct_reads(38), "staged_37": lambda: direct_reads(37),
            "box_pillar": box_pillar, "box_aside": box_aside, "after_the_pillar": after_the_pillar, "out_and_back": out_and_back, "floor_step": floor_step,
            "everywhere": everywhere, "corner_max": lambda: corner(1), "corner_min": lambda: corner(-1), "batch": batch,
            "batch_speeds": lambda: batch(2.0, ((8, 15), 5))}
for _q, _lead, _v in TIMINGS:
    BUILDERS["timing_q%d_lead%d_v%d" % (_q, _lead, _v)] = functools.partial(timing, _q, _lead, _v)


@functools.lru_cache(maxsize=None)
def get(name):
    return BUILDERS[name]()
