"""Named inputs for the local planner (botlab_amd/csrc/bl_localplan.hip) that the cases of tests/test_local_plan_model_cpu.py do not
give it, and the proof -- on the CPU, from the model (tests/local_plan_model.py) alone -- that each one is what it is named for.
A builder returns (world factory, Params, states), states being [(pose, v, w)], and asserts its own property before it returns, so
a case cannot silently stop being what it claims.  tests/test_gpu_local_plan_edges.py compares the device with the model on every
one of them, byte for byte.

Groups:
  shapes         launch shapes (nvp, jpb, bps, size of the last run of j) the host derives: jpb capped by the 2048 (cos, sin) slots
                 with n_w > jpb, a jpb that is no power of two, both caps equal, all 256 threads walking a heading chain, a partial
                 last workgroup after long step counts; each staged, the long ones also not staged
  many           66 states at two workgroups per state (the second holds one heading), all four flag values among them, and a second
                 list in which every state that wrote partials in the first is flagged
  ties           every admissible candidate costs the same (all weights 0), or every j ties at one i (w_speed alone): the winner in
                 wave 1, 2, 3 of workgroup 0, in workgroup 1, 2, 3 behind workgroups without an admissible candidate, in a partial
                 last workgroup, in the upper half of its wave
  keys           costs beyond 2^32 whose low 32 bits elect another winner.  A field beyond 2^31 itself (the uint32 read as int) needs
                 a path of about half a million cells: out of scope for a test of a few seconds, no case has one.
  strip          poses and rollouts in the (-1, 0) strip of grid coordinates that the truncating cast gives to cell 0
  flagged_costs  OFF_FIELD states whose debug costs hold finite entries
  headings       pose.theta at +-(float)pi, its neighbours, 100, -1000 and BL_LOCALPLAN_MAX_THETA

launch_shape() restates the host's arithmetic; emulate() restates how the kernels spread a call over workgroups and collect it
again (per-workgroup partials that persist between calls, then one pass per state), with the model's costs in place of the
device's, so that tests/test_local_plan_cases_cpu.py can show which case notices which mistake in that plumbing."""
import functools
import math

import numpy as np

import helpers
import local_plan_model as lpm
import test_local_plan_model_cpu as cpu
from scan_match_model import PI_F

F32 = np.float32
CPM = helpers.CPM_DEFAULT
LP_THREADS, LP_TRIG_SLOTS = 256, 2048
NAV_MAX_GAIN = 4095
NO_C = 0x7FFFFFFF


def launch_shape(p):
    """(nvp, jpb, bps, size of the last run) as lp_prepare forms them."""
    nvp = 1
    while nvp < p.n_v:
        nvp *= 2
    jpb = min(LP_THREADS // nvp, LP_TRIG_SLOTS // (p.n_steps + 1), p.n_w)
    bps = -(-p.n_w // jpb)
    return nvp, jpb, bps, p.n_w - (bps - 1) * jpb


def place(p, c):
    """(workgroup of the state, wave, lane) of the thread that rolls candidate c out."""
    nvp, jpb, _, _ = launch_shape(p)
    j, i = divmod(c, p.n_v)
    tid = (j % jpb) * nvp + i
    return j // jpb, tid // 64, tid % 64


def on_cell(world, fx, fy, theta):
    """The pose at grid coordinates (fx, fy) -- cell (int(fx), int(fy)) -- of the world."""
    return (F32(float(F32(world.origin[0])) + fx * float(world.mpc)), F32(float(F32(world.origin[1])) + fy * float(world.mpc)), F32(theta))


@functools.lru_cache(maxsize=None)
def _model(factory, p, state):
    """(record, costs, stats) of one state, once: costs also for a flagged state."""
    world = factory()
    stats = {}
    rec, cs = lpm.command(world, p, *state, stats)
    if cs is None:                                                                      # flagged before any rollout
        cs = lpm.costs(world, p, *state, stats)
    return rec, cs, stats


class _P(lpm.Params):
    """Params that can be a cache key."""

    def __init__(self, **kw):
        lpm.Params.__init__(self, **kw)
        self._key = tuple(sorted(kw.items()))

    def __hash__(self):
        return hash(self._key)

    def __eq__(self, other):
        return self._key == other._key


def model(case, k=0):
    factory, p, states = case
    return _model(factory, p, states[k])


def _checked(case):
    factory, p, states = case
    assert p.ok() and not p.can_skip_a_cell(cpu.MPC)
    assert all(lpm.state_ok(*s) for s in states)
    return case


# ---------------------------------------------------------------------------------------------------------------- shapes
SHAPE = dict(v_min=-0.1, v_max=0.5, w_max=2.5, acc_v=3.0, acc_w=20.0, dt_control=0.1, dt_sim=0.05, w_field=7, w_heading=3, w_clear=2, w_speed=11)
# (n_v, n_w, n_steps) -> (nvp, jpb, bps, size of the last run)
SHAPES = {(3, 20, 255): (4, 8, 3, 4), (1, 19, 204): (1, 9, 3, 1), (64, 9, 255): (64, 4, 3, 1), (2, 130, 15): (2, 128, 2, 2),
          (1, 1025, 7): (1, 256, 5, 1), (1, 100, 255): (1, 8, 13, 4), (17, 40, 100): (32, 8, 5, 8)}
SHAPE_RUNS = [(k, 0.1) for k in SHAPES] + [(k, 0.5) for k in SHAPES if k[2] >= 152]


def ragged_start(world):
    return cpu.cell_centre(world, 24, 54) + (F32(0.4),)


def shape_name(n_v, n_w, n_steps, v_max):
    return "shape_%d_%d_%d_%s" % (n_v, n_w, n_steps, "staged" if v_max == 0.1 else "grids")


def shape_case(n_v, n_w, n_steps, v_max):
    p = _P(**dict(SHAPE, v_max=v_max, n_v=n_v, n_w=n_w, n_steps=n_steps))
    nvp, jpb, bps, last = launch_shape(p)
    assert (nvp, jpb, bps, last) == SHAPES[(n_v, n_w, n_steps)]
    assert jpb == min(256 // nvp, 2048 // (n_steps + 1), n_w) and bps == -(-n_w // jpb) and 1 <= last <= jpb and (bps - 1) * jpb + last == n_w
    assert nvp >= n_v and nvp & (nvp - 1) == 0 and (nvp == 1 or nvp // 2 < n_v)
    assert p.staged(CPM) == (v_max == 0.1)
    world = cpu.ragged_world()
    assert world.field.shape == (117, 203)
    case = _checked((cpu.ragged_world, p, [(ragged_start(world), F32(0.2), F32(-0.3))]))
    rec, cs, _ = model(case)
    assert int(rec["flags"]) == 0 and int(rec["n_admissible"]) > 0
    return case


def check_shape_table():
    """(checked by tests/test_local_plan_cases_cpu.py) which cap binds where"""
    cap = {k: (256 // v[0], 2048 // (k[2] + 1), k[1]) for k, v in SHAPES.items()}
    assert cap[(3, 20, 255)] == (64, 8, 20) and cap[(1, 19, 204)] == (256, 9, 19) and cap[(64, 9, 255)] == (4, 8, 9)
    assert cap[(2, 130, 15)] == (128, 128, 130) and cap[(1, 1025, 7)] == (256, 256, 1025)
    assert cap[(1, 100, 255)] == (256, 8, 100) and cap[(17, 40, 100)] == (8, 20, 40)


# ---------------------------------------------------------------------------------------------------------------- many
MANY = dict(SHAPE, v_min=0.3, n_v=5, n_w=33, n_steps=6)
MANY_MARKED = (0, 31, 63, 64, 65)


def _many_params():
    p = _P(**MANY)
    assert launch_shape(p) == (8, 32, 2, 1)
    return p


def _many_fixed(world):
    """the poses with a known flag: off the grid, on the goal, facing the right wall from 0.1 cell (v_min > 0: BLOCKED), free"""
    return dict(off=(on_cell(world, -2.5, 20.5, 0.0), F32(0.3), F32(0.0)), goal=(on_cell(world, 50.5, 23.5, 1.0), F32(0.4), F32(0.1)),
                blocked=(on_cell(world, 59.9, 30.5, 0.0), F32(0.4), F32(0.0)), free=(on_cell(world, 20.5, 23.5, 0.3), F32(0.4), F32(0.2)),
                free2=(on_cell(world, 30.25, 10.75, -2.0), F32(0.3), F32(-1.0)))


def _many_random(world, seed, n=66):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        x, y = rng.uniform(-2.0, world.w + 2.0), rng.uniform(-2.0, world.h + 2.0)        # some off the grid, some on the wall
        out.append((on_cell(world, x, y, rng.uniform(-4, 4)), F32(rng.uniform(0.3, 0.5)), F32(rng.uniform(-2.5, 2.5))))
    return out


def many_first():
    world = cpu.uniform_world()
    fx = _many_fixed(world)
    states = _many_random(world, 14)
    for k, name in zip(MANY_MARKED + (17,), ("off", "goal", "free", "blocked", "free2", "blocked")):
        states[k] = fx[name]
    case = _checked((cpu.uniform_world, _many_params(), states))
    flags = [int(model(case, k)[0]["flags"]) for k in range(66)]
    assert [flags[k] for k in MANY_MARKED] == [lpm.OFF_FIELD, lpm.REACHED, 0, lpm.BLOCKED, 0] and flags[17] == lpm.BLOCKED
    assert flags.count(0) >= 20 and flags.count(lpm.OFF_FIELD) >= 5
    return case


def many_second():
    """The same shape; every state of the first list that wrote partials (unflagged, or BLOCKED after the rollout) is flagged here
    before any rollout, so its slots keep what the first call left; states that were flagged in the first list roll out here."""
    first = many_first()
    world = cpu.uniform_world()
    fx = _many_fixed(world)
    states = []
    for k in range(66):
        f = int(model(first, k)[0]["flags"])
        if f in (0, lpm.BLOCKED):
            states.append(fx["goal"] if k % 2 else fx["off"])
        else:
            states.append(fx["free"] if k % 2 else fx["free2"])
    case = _checked((cpu.uniform_world, _many_params(), states))
    for k in range(66):
        f1, f2 = int(model(first, k)[0]["flags"]), int(model(case, k)[0]["flags"])
        assert (f2 in (lpm.REACHED, lpm.OFF_FIELD)) == (f1 in (0, lpm.BLOCKED)), (k, f1, f2)
    return case


# ---------------------------------------------------------------------------------------------------------------- ties
TIE = dict(v_min=0.3, v_max=0.5, w_max=2.5, acc_v=0.5, acc_w=30.0, dt_control=0.1, dt_sim=0.05, n_v=64, n_w=16, n_steps=12, w_field=0,
           w_heading=0, w_clear=0, w_speed=0)
# name -> (height above the bottom wall in cells, heading, n_w, w_speed, (workgroup, wave) the winner must sit in): the pose is at
# x = 20.5 cells, the bottom wall is row 0, a negative w turns towards it
TIES = {"tie_wave1": (3.2, 0.0, 16, 0, (0, 1)), "tie_wave2": (3.05, 0.0, 16, 0, (0, 2)), "tie_wave3": (2.9, 0.0, 16, 0, (0, 3)),
        "tie_wg1": (2.3, 0.0, 16, 0, (1, None)), "tie_wg2": (1.1, 0.0, 16, 0, (2, None)), "tie_wg3": (2.0, -0.6, 16, 0, (3, None)),
        "tie_last_partial": (2.0, -0.7, 14, 0, (3, None))}


def tie_case(name):
    off, theta, n_w, w_speed, (wg, wave) = TIES[name]
    p = _P(**dict(TIE, n_w=n_w, w_speed=w_speed))
    nvp, jpb, bps, last = launch_shape(p)
    assert (nvp, jpb, bps) == (64, 4, 4) and last == (4 if n_w == 16 else 2)
    world = cpu.uniform_world()
    case = _checked((cpu.uniform_world, p, [(on_cell(world, 20.5, off, theta), F32(0.4), F32(0.0))]))
    rec, cs, _ = model(case)
    adm = cs != lpm.COST_NONE
    assert int(rec["flags"]) == 0 and (cs[adm] == 0).all() and int(adm.sum()) > 64                 # every admissible candidate ties
    c = int(rec["index"])
    got = place(p, c)
    assert got[0] == wg and (wave is None or got[1] == wave), (name, c, got)
    assert not adm[:c].any() and c == int(np.flatnonzero(adm)[0])
    if wg:
        assert not adm[:wg * jpb * p.n_v].any()                                                     # n_adm == 0 in every earlier workgroup
    assert adm[(c // p.n_v + 1) * p.n_v:].any()                                                     # later waves tie with it
    if wg == bps - 1 and n_w == 14:
        assert c // p.n_v in (12, 13)
    return case


def tie_upper_half():
    """w_speed alone: a candidate costs w_speed * (63 - i), so the least cost sits at the largest admissible i, which every row of
    candidates that has it shares.  The pose faces the bottom wall from close by with a table of speeds from reversing to forward:
    the fast forward candidates (large i) hit the wall.  The winner sits in the upper half of its wave (lane >= 32, below lane 63:
    it reaches lane 0 through the first step of the shuffle reduction), rows of later waves and workgroups tie with it, and other
    rows have their best candidate at a lower i (a greater cost)."""
    p = _P(**dict(TIE, v_min=-0.5, v_max=0.5, acc_v=10.0, w_speed=9))
    world = cpu.uniform_world()
    case = _checked((cpu.uniform_world, p, [(on_cell(world, 20.5, 3.2, -math.pi / 2), F32(0.0), F32(0.0))]))
    rec, cs, _ = model(case)
    adm = (cs != lpm.COST_NONE).reshape(p.n_w, p.n_v)
    c = int(rec["index"])
    j, i = divmod(c, p.n_v)
    assert int(rec["flags"]) == 0 and 32 <= i < 63 and int(rec["cost"]) == 9 * (63 - i)
    assert not adm[:, i + 1:].any() and not adm[:j, i].any()
    ties = [r for r in range(p.n_w) if adm[r, i]]
    assert len(ties) >= 2 and ties[0] == j and len({place(p, r * p.n_v + i)[0] for r in ties}) >= 2, ties
    assert any(adm[r].any() and not adm[r, i] for r in range(p.n_w))                                 # rows whose best is at a lower i
    return case


def tie_i_before_j():
    """All weights 0 and a table of speeds from reversing to forward, the pose facing away from the bottom wall at an angle: the fast
    reversing candidates (low i) hit it, more of them in the rows that turn less.  The first admissible candidate by c is in row 0;
    a later row has an admissible candidate at a lower i, which an order by (cost, i, j) would elect."""
    p = _P(**dict(TIE, v_min=-0.5, v_max=0.5, acc_v=10.0))
    world = cpu.uniform_world()
    case = _checked((cpu.uniform_world, p, [(on_cell(world, 20.5, 2.6, 2.17), F32(0.0), F32(0.0))]))
    rec, cs, _ = model(case)
    adm = np.flatnonzero(cs != lpm.COST_NONE)
    assert int(rec["flags"]) == 0 and (cs[adm] == 0).all() and int(rec["index"]) == int(adm[0]) and int(adm[0]) // p.n_v == 0
    assert int((adm % p.n_v).min()) < int(adm[0]) % p.n_v
    return case


def tie_baseline():
    factory, p, pose, v, w = cpu.condition_cases()["ties"]
    case = _checked((factory, _P(**{k: getattr(p, k) for k in ("v_min", "v_max", "w_max", "acc_v", "acc_w", "dt_control", "dt_sim", "n_v", "n_w",
                                                                "n_steps", "w_field", "w_heading", "w_clear", "w_speed")}),
                     [(pose, F32(v), F32(w))]))
    rec, cs, _ = model(case)
    assert int((cs == cs.min()).sum()) > 1 and int(rec["index"]) == int(np.flatnonzero(cs == cs.min())[0]) and case[1].n_v * case[1].n_w == 36
    return case


# ---------------------------------------------------------------------------------------------------------------- keys
@functools.lru_cache(maxsize=None)
def keys_world():
    """The ragged world with obstacle_gain = NAV_MAX_GAIN.  With the 0.5 m over which the other worlds spread the penalty the largest
    field value of this grid is 25 494, and 65535 * 25 494 < 2^31: no weight makes the field term cross 2^31.  So the penalty here
    reaches 2 m from an obstacle; then every path pays it and the start's field is 160 037."""
    return cpu.make_world(cpu.ragged_cells(), (F32(-3.25), F32(1.5)), cpu.MPC, [(190, 100)], 1,
                          dict(cpu.SMALL_NAV, obstacle_gain=NAV_MAX_GAIN, maxDistanceWithCost=2.0))[0]


def low32(cs):
    """The costs as a key that kept only its low 32 bits (unsigned); inadmissible stays inadmissible."""
    return np.where(cs != lpm.COST_NONE, cs & 0xFFFFFFFF, lpm.COST_NONE)


def as_int32(cs):
    """The costs after truncation to int32."""
    return np.where(cs != lpm.COST_NONE, ((cs & 0xFFFFFFFF) ^ 0x80000000) - 0x80000000, lpm.COST_NONE)


def keys_case():
    """Weights of 65535 over a field of 10^5 and penalty sums of 10^5: every product passes 2^31 and the costs 2^32.  A field above
    2^31 itself would need a path of about half a million cells, out of scope for a test of a few seconds."""
    p = _P(v_min=0.0, v_max=0.25, w_max=2.5, acc_v=3.0, acc_w=20.0, dt_control=0.1, dt_sim=0.05, n_v=6, n_w=11, n_steps=255, w_field=65535,
           w_heading=65535, w_clear=65535, w_speed=65535)
    assert p.staged(CPM) and launch_shape(p) == (8, 8, 2, 3)
    world = keys_world()
    assert world.nav.obstacle_gain == NAV_MAX_GAIN and int(world.pcell.max()) <= NAV_MAX_GAIN and int(world.pcell.max()) > 2047
    case = _checked((keys_world, p, [(ragged_start(world), F32(0.1), F32(0.1))]))
    rec, cs, stats = model(case)
    adm = cs != lpm.COST_NONE
    terms = stats["terms"]
    assert any(p.w_field * t[0] >= 2 ** 31 for t in terms.values())
    assert any(p.w_clear * t[2] >= 2 ** 31 for t in terms.values())
    assert (cs[adm] >= 2 ** 32).any()
    assert int(rec["flags"]) == 0 and int(np.argmin(low32(cs))) != int(rec["index"]) == int(np.argmin(cs))
    return case


# ---------------------------------------------------------------------------------------------------------------- strip
STRIP = dict(v_min=-0.2, v_max=0.4, w_max=2.0, acc_v=10.0, acc_w=30.0, dt_control=0.1, dt_sim=0.05, n_v=5, n_w=9, n_steps=14, w_field=3,
             w_heading=2, w_clear=1, w_speed=5)
# name -> (fx, fy, heading): -0.5 is the middle of the strip; headings along it, into the grid and out of it
STRIPS = {"strip_x_along_up": (-0.5, 18.5, math.pi / 2), "strip_x_along_down": (-0.5, 18.5, -math.pi / 2), "strip_x_in": (-0.5, 18.5, 0.0),
          "strip_x_out": (-0.5, 18.5, math.pi), "strip_y_along": (20.5, -0.5, 0.0), "strip_y_in": (20.5, -0.5, math.pi / 2),
          "strip_y_out": (20.5, -0.5, -math.pi / 2), "strip_corner_in": (-0.5, -0.5, math.pi / 4), "strip_corner_out": (-0.5, -0.5, -3 * math.pi / 4),
          "strip_corner_along": (-0.5, -0.5, 0.0)}


def strip_case(name):
    fx, fy, theta = STRIPS[name]
    world = cpu.open_world()
    pose = on_cell(world, fx, fy, theta)
    assert world.cell(pose[0], pose[1]) == (max(int(fx), 0), max(int(fy), 0)) and (fx < 0 or fy < 0)
    assert world.start_flags(pose[0], pose[1]) == 0
    case = _checked((cpu.open_world, _P(**STRIP), [(pose, F32(0.1), F32(0.0))]))
    rec, cs, stats = model(case)
    assert int(rec["flags"]) == 0 and stats.get("strip", 0) > 0 and stats.get("strip_candidates", 0) > 0, (name, stats.get("strip"))
    if name.endswith("out"):
        assert stats.get("left", 0) + stats.get("bottom", 0) > 0                                    # and some leave the grid through it
    return case


# ---------------------------------------------------------------------------------------------------------------- flagged costs
FLAGGED = dict(v_min=0.0, v_max=0.5, w_max=2.0, acc_v=10.0, acc_w=8.0, dt_control=0.1, dt_sim=0.05, n_v=6, n_w=7, n_steps=10, w_field=3,
               w_heading=2, w_clear=1, w_speed=5)


def flagged_case(name):
    if name == "flagged_right":
        factory, world = cpu.open_world, cpu.open_world()
        pose = on_cell(world, world.w + 0.2, 18.5, math.pi)
        assert world.cell(pose[0], pose[1]) is None
    elif name == "flagged_top":
        factory, world = cpu.open_world, cpu.open_world()
        pose = on_cell(world, 20.5, world.h + 0.2, -math.pi / 2)
        assert world.cell(pose[0], pose[1]) is None
    else:
        assert name == "flagged_wall"
        factory, world = cpu.uniform_world, cpu.uniform_world()
        pose = on_cell(world, 0.9, 20.5, 0.0)
        assert world.cell(pose[0], pose[1]) == (0, 20) and not world.tcell[20, 0] and world.tcell[20, 1]
    case = _checked((factory, _P(**FLAGGED), [(pose, F32(0.2), F32(0.0))]))
    rec, cs, _ = model(case)
    assert int(rec["flags"]) == lpm.OFF_FIELD and int(rec["index"]) == -1 and int(rec["cost"]) == lpm.COST_NONE
    adm = cs != lpm.COST_NONE
    assert adm.any() and not adm.all(), (name, int(adm.sum()))
    return case


# ---------------------------------------------------------------------------------------------------------------- headings
HEADING = dict(v_min=0.0, v_max=0.5, w_max=2.0, acc_v=1.0, acc_w=8.0, dt_control=0.1, dt_sim=0.05, n_v=4, n_w=9, n_steps=12, w_field=2,
               w_heading=3, w_clear=1, w_speed=1)
THETAS = {"heading_pi": PI_F, "heading_minus_pi": F32(-PI_F), "heading_pi_below": np.nextafter(PI_F, F32(0)),
          "heading_pi_above": np.nextafter(PI_F, F32(4)), "heading_minus_pi_below": np.nextafter(F32(-PI_F), F32(-4)),
          "heading_minus_pi_above": np.nextafter(F32(-PI_F), F32(0)), "heading_100": F32(100.0), "heading_minus_1000": F32(-1000.0),
          "heading_max": lpm.MAX_THETA, "heading_minus_max": F32(-lpm.MAX_THETA)}


def heading_case(name):
    theta = THETAS[name]
    world = cpu.uniform_world()
    case = _checked((cpu.uniform_world, _P(**HEADING), [(on_cell(world, 20.5, 23.5, 0.0)[:2] + (F32(theta),), F32(0.2), F32(0.0))]))
    wt = lpm.tables(case[1], F32(0.2), F32(0.0))[1]
    assert wt[0] < 0 < wt[-1] and (wt == 0).any()
    rec, cs, _ = model(case)
    assert int(rec["flags"]) == 0 and int(rec["n_admissible"]) > 0
    return case


def check_theta_limit():
    """(checked by tests/test_local_plan_cases_cpu.py)"""
    steps, a = 0, lpm.MAX_THETA
    while a >= PI_F:                                                                    # wrap_to_pi's own loop, counted
        a, steps = F32(float(a) - 2.0 * math.pi), steps + 1
    assert steps == 10432 < 1 << 16 and a == lpm.wrap_to_pi(lpm.MAX_THETA), steps
    assert lpm.state_ok((F32(0), F32(0), lpm.MAX_THETA), 0, 0) and lpm.state_ok((F32(0), F32(0), -lpm.MAX_THETA), 0, 0)
    assert not lpm.state_ok((F32(0), F32(0), np.nextafter(lpm.MAX_THETA, F32(np.inf))), 0, 0)
    assert not lpm.state_ok((F32(0), F32(0), np.nextafter(-lpm.MAX_THETA, F32(-np.inf))), 0, 0)
    assert not lpm.state_ok((F32(0), F32(0), F32(np.nan)), 0, 0) and not lpm.state_ok((F32(0), F32(np.inf), F32(0)), 0, 0)


# ---------------------------------------------------------------------------------------------------------------- the list
BUILDERS = {}
for _k, _v in SHAPE_RUNS:
    BUILDERS[shape_name(*_k, _v)] = (lambda k=_k, v=_v: shape_case(*k, v))
BUILDERS.update(many_first=many_first, many_second=many_second)
for _n in TIES:
    BUILDERS[_n] = (lambda n=_n: tie_case(n))
BUILDERS.update(tie_upper_half=tie_upper_half, tie_i_before_j=tie_i_before_j, tie_baseline=tie_baseline, keys=keys_case)
for _n in STRIPS:
    BUILDERS[_n] = (lambda n=_n: strip_case(n))
for _n in ("flagged_right", "flagged_top", "flagged_wall"):
    BUILDERS[_n] = (lambda n=_n: flagged_case(n))
for _n in THETAS:
    BUILDERS[_n] = (lambda n=_n: heading_case(n))
GROUPS = dict(shapes=[shape_name(*k, v) for k, v in SHAPE_RUNS], many=["many_first", "many_second"],
              ties=list(TIES) + ["tie_upper_half", "tie_i_before_j", "tie_baseline"], keys=["keys"], strip=list(STRIPS),
              flagged_costs=["flagged_right", "flagged_top", "flagged_wall"], headings=list(THETAS))
SINGLE = [n for g in ("shapes", "ties", "keys", "strip", "flagged_costs", "headings") for n in GROUPS[g]]

_cases = {}


def get(name):
    if name not in _cases:
        _cases[name] = BUILDERS[name]()
    return _cases[name]


# the mistaken selection rules each case of `ties` and `keys` tells from the definition's (tests/test_local_plan_cases_cpu.py)
DEFEATS = {"tie_wave1": ("ties_to_highest_c",), "tie_wave2": ("ties_to_highest_c",), "tie_wave3": ("ties_to_highest_c",),
           "tie_wg1": ("ties_to_highest_c",), "tie_wg2": ("ties_to_highest_c",), "tie_wg3": ("ties_to_highest_c",),
           "tie_last_partial": ("ties_to_highest_c",), "tie_upper_half": ("ties_to_highest_c",),
           "tie_i_before_j": ("ties_to_highest_c", "order_cost_i_j"), "tie_baseline": ("ties_to_highest_c",), "keys": ("int32_cost",)}


# ---------------------------------------------------------------------------------------------------------------- the plumbing
def elect(cs, rule="definition", n_v=1):
    """The winner among the costs of one state under a selection rule: the definition's (cost, c), or a mistaken one."""
    adm = np.flatnonzero(cs != lpm.COST_NONE)
    if len(adm) == 0:
        return -1
    c32 = as_int32(cs)
    keyed = {"definition": lambda c: (int(cs[c]), c), "ties_to_highest_c": lambda c: (int(cs[c]), -c),
             "order_cost_i_j": lambda c: (int(cs[c]), c % n_v, c // n_v), "int32_cost": lambda c: (int(c32[c]), c)}
    return min(adm.tolist(), key=keyed[rule])


def narrow_products(p, terms, n_v):
    """The costs with each of the four products formed in int32 (wrapping), then summed in int64."""
    def w32(v):
        return ((v & 0xFFFFFFFF) ^ 0x80000000) - 0x80000000
    out = np.full(p.n_v * p.n_w, lpm.COST_NONE, np.int64)
    for c, (fe, h, pen) in terms.items():
        out[c] = w32(p.w_field * fe) + w32(p.w_heading * h) + w32(p.w_clear * pen) + w32(p.w_speed * (p.n_v - 1 - c % n_v))
    return out


def emulate(case, partial, mistake=None):
    """One bl_localplan_commands call as the kernels spread it: k_lp_rollout's workgroups write (cost, c, n_adm) into `partial`, a
    dict by slot that the caller keeps between calls like the handle keeps d_partial; k_lp_finish reads them back per state.  The
    costs are the model's.  mistake: None, or one of
      'ties_to_highest_c'   lp_key_less without the (cost, c) order
      'narrow_products'     a product formed in 32 bits
      'state_of_block'      state = blockIdx.x % n and blk = blockIdx.x / n in place of blockIdx.x / bps, blockIdx.x % bps
      'finish_reads_stale'  k_lp_finish takes the partials of a flagged state too
    Returns the RESULT records."""
    factory, p, states = case
    world = factory()
    n = len(states)
    nvp, jpb, bps, _ = launch_shape(p)
    rule = "ties_to_highest_c" if mistake == "ties_to_highest_c" else "definition"
    for b in range(n * bps):
        state, blk = (b % n, b // n) if mistake == "state_of_block" else (b // bps, b % bps)
        pose = states[state][0]
        if world.start_flags(pose[0], pose[1]):
            continue                                                                    # the early return: the slot keeps what it held
        rec, cs, stats = _model(factory, p, states[state])
        if mistake == "narrow_products":
            cs = narrow_products(p, stats.get("terms", {}), p.n_v)
        run = cs[blk * jpb * p.n_v:min((blk + 1) * jpb, p.n_w) * p.n_v]
        c = elect(run, rule)
        partial[b] = (int(run[c]), blk * jpb * p.n_v + c, int((run != lpm.COST_NONE).sum())) if c >= 0 else (lpm.COST_NONE, NO_C, 0)
    out = np.zeros(n, lpm.RESULT)
    for state in range(n):
        pose, v, w = states[state]
        r = out[state]
        r["index"], r["cost"] = -1, lpm.COST_NONE
        flags = world.start_flags(pose[0], pose[1])
        r["flags"] = flags
        if flags == lpm.REACHED:
            r["cost"] = 0
        if flags and mistake != "finish_reads_stale":
            continue
        best, adm = (lpm.COST_NONE, NO_C), 0
        for b in range(bps):
            cost, c, n_adm = partial.get(state * bps + b, (0, 0, 0))
            key = (cost, -c) if rule == "ties_to_highest_c" else (cost, c)
            if key < ((best[0], -best[1]) if rule == "ties_to_highest_c" else best):
                best = (cost, c)
            adm += n_adm
        r["n_admissible"] = adm
        if adm == 0:
            r["flags"] = flags | lpm.BLOCKED if not flags else flags
            continue
        vt, wt = lpm.tables(p, v, w)
        r["index"], r["cost"] = best[1], best[0]
        r["trans_v"], r["angular_v"] = vt[best[1] % p.n_v], wt[best[1] // p.n_v]
    return out


def model_records(case):
    return [model(case, k)[0] for k in range(len(case[2]))]


def same_records(got, exp):
    return all(got[k][f].tobytes() == exp[k][f].tobytes() for k in range(len(exp))
               for f in ("trans_v", "angular_v", "index", "n_admissible", "cost", "flags"))
