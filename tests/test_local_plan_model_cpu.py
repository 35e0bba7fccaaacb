"""The local planner's model (tests/local_plan_model.py) on its own: a closed loop on the obstacle map, and every condition of the
definition reached at least once (each printed as a count).  The GPU tests compare the kernels with the model on these inputs."""
import functools
import math

import numpy as np

import helpers
import local_plan_model as lpm
import nav_field_model as nm
from scan_match_model import wrap_to_pi

F32 = np.float32
CPM = helpers.CPM_DEFAULT
OBSTACLE = "obstacle_slam_10mx10m_5cm"
NAV = dict(minDistanceToObstacle=0.2, maxDistanceWithCost=2.0, distanceCostExponent=1.0, obstacle_gain=50)


@functools.lru_cache(maxsize=None)
def _maps():
    return helpers.load_reference_maps()


def make_world(cells, origin, mpc, goals, reach=0, nav=None):
    """(World, l1, nm.Params): the navigation field's model solved for `goals` on `cells`."""
    p = nm.Params(reach_cells=reach, **(nav or NAV))
    l1 = nm.l1_distances(cells)
    h, w = cells.shape
    trav, pen = nm.tables(nm.dist_table(w, h), p)
    field = nm.dijkstra(l1, trav, pen, goals, reach)
    world = lpm.World(field, l1, trav, pen, origin, mpc, CPM)
    world.cells, world.goals, world.nav = cells, list(goals), p          # what a device copy of this world is built from
    return world, l1, p


def cell_centre(world, x, y):
    return (F32(float(F32(world.origin[0])) + (x + 0.5) * float(world.mpc)), F32(float(F32(world.origin[1])) + (y + 0.5) * float(world.mpc)))


# ---------------------------------------------------------------------------------------------------------------- closed loop
LOOP_GOAL, LOOP_REACH = (98, 124), 2                     # in the passage between the two blocks of the map
LOOP_START = (72, 128, math.pi)                          # left of the first block, facing the wall: more than 90 degrees to turn
LOOP_PARAMS = dict(v_min=0.0, v_max=0.5, w_max=2.5, acc_v=2.0, acc_w=12.0, dt_control=0.1, dt_sim=0.05, n_v=4, n_w=15, n_steps=20,
                   w_field=16, w_heading=1, w_clear=1, w_speed=8)


@functools.lru_cache(maxsize=None)
def loop_world():
    m = _maps()[OBSTACLE]
    return make_world(m["cells"], m["origin"], m["mpc"], [LOOP_GOAL], LOOP_REACH)


def loop_start(world):
    x, y = cell_centre(world, LOOP_START[0], LOOP_START[1])
    return (x, y, F32(LOOP_START[2]))


def run_loop(world, p, pose, max_ticks, step):
    """Ticks of (command, drive) from `pose` at rest; step(pose, v, w) -> the command's RESULT record.  Returns the records, the poses
    at the ticks and the cells passed through."""
    v, w = F32(0), F32(0)
    recs, poses, cells = [], [pose], []
    for _ in range(max_ticks):
        r = step(pose, v, w)
        recs.append(r)
        if int(r["flags"]) & lpm.REACHED:
            break
        v, w = F32(r["trans_v"]), F32(r["angular_v"])
        for q in lpm.drive(pose, v, w, p):
            cells.append(world.cell(q[0], q[1]))
            pose = q
        poses.append(pose)
    return recs, poses, cells


def test_closed_loop_arrives_and_the_field_term_is_what_steers():
    world, l1, navp = loop_world()
    p = lpm.Params(**LOOP_PARAMS)
    assert p.ok() and not p.can_skip_a_cell(world.mpc)
    start = loop_start(world)
    path, _, cost = nm.descend(world.field, l1, *nm.tables(nm.dist_table(world.w, world.h), navp), [LOOP_GOAL], LOOP_REACH,
                               (0, start[0], start[1], start[2]), world.origin, world.mpc, CPM)
    assert len(path) > 10 and cost != nm.UNREACHED
    xy = np.stack([path["x"].astype(np.float64), path["y"].astype(np.float64)], axis=1)
    L = float(np.sqrt((np.diff(xy, axis=0) ** 2).sum(axis=1)).sum())
    cap = 4 * int(math.ceil(L / (float(p.v_max) * float(p.dt_control))))
    recs, poses, cells = run_loop(world, p, start, cap, lambda q, v, w: lpm.command(world, p, q, v, w)[0])
    assert all(c is not None and world.tcell[c[1], c[0]] for c in cells)
    assert int(recs[-1]["flags"]) == lpm.REACHED, (len(recs), recs[-1])
    turned = sum(abs(float(wrap_to_pi(F32(b[2] - a[2])))) for a, b in zip(poses[:-1], poses[1:]))
    through = sum(1 for c in cells if 94 <= c[0] <= 102 and 118 <= c[1] <= 138)
    print(f"closed loop: path {L:.2f} m, cap {cap} ticks, arrived after {len(recs) - 1} ticks, turned {math.degrees(turned):.0f} degrees, "
          f"{through} steps inside the passage")
    assert turned > math.pi / 2 and through > 0
    # the same start without the field term does not arrive
    p0 = lpm.Params(**dict(LOOP_PARAMS, w_field=0))
    recs0, _, cells0 = run_loop(world, p0, start, cap, lambda q, v, w: lpm.command(world, p0, q, v, w)[0])
    assert all(c is not None and world.tcell[c[1], c[0]] for c in cells0)
    assert int(recs0[-1]["flags"]) != lpm.REACHED and len(recs0) == cap
    print(f"closed loop, w_field = 0: not arrived after {cap} ticks")


# ---------------------------------------------------------------------------------------------------------------- conditions
def uniform_cells(w, h):
    """Free everywhere inside a one-cell wall."""
    c = np.full((h, w), -100, np.int8)
    c[0, :] = c[-1, :] = 100
    c[:, 0] = c[:, -1] = 100
    return c


def open_cells(w, h):
    """Free everywhere but one occupied cell in the middle: traversable up to the very border of the grid."""
    c = np.full((h, w), -100, np.int8)
    c[h // 2, w // 2] = 100
    return c


SMALL_NAV = dict(minDistanceToObstacle=0.04, maxDistanceWithCost=0.5, distanceCostExponent=1.0, obstacle_gain=50)
ORIGIN = (F32(-1.0), F32(-2.0))
MPC = F32(0.05)


@functools.lru_cache(maxsize=None)
def uniform_world():
    return make_world(uniform_cells(61, 47), ORIGIN, MPC, [(50, 23)], 0, SMALL_NAV)[0]


@functools.lru_cache(maxsize=None)
def open_world():
    return make_world(open_cells(41, 37), ORIGIN, MPC, [(30, 8)], 0, SMALL_NAV)[0]


@functools.lru_cache(maxsize=None)
def pocket_world():
    """Occupied everywhere but a corridor one cell wide, (5, 15) .. (15, 15), with the goal at its open end -- its far end (15, 15) is
    the one-cell pocket -- and a lone free cell (25, 25) that nothing connects to the goal."""
    c = np.full((31, 31), 100, np.int8)
    c[15, 5:16] = -100
    c[25, 25] = -100
    return make_world(c, ORIGIN, MPC, [(5, 15)], 0, SMALL_NAV)[0]


def ragged_cells(w=203, h=117, seed=9):
    """A 203 x 117 world, neither side a multiple of anything: a wall around it, two walls with gaps and scattered blocks."""
    rng = np.random.default_rng(seed)
    c = uniform_cells(w, h)
    c[20:h - 1, 60] = 100
    c[1:h - 25, 130] = 100
    for _ in range(25):
        x, y = int(rng.integers(3, w - 8)), int(rng.integers(3, h - 8))
        c[y:y + int(rng.integers(2, 6)), x:x + int(rng.integers(2, 6))] = 100
    c[50:60, 20:30] = -100                               # room for a start
    return c


@functools.lru_cache(maxsize=None)
def ragged_world():
    return make_world(ragged_cells(), (F32(-3.25), F32(1.5)), MPC, [(190, 100)], 1, SMALL_NAV)[0]


def condition_cases():
    """name -> (world factory, Params, pose (x, y, theta), v, w): the inputs the CPU test counts conditions on and the GPU test
    compares byte for byte."""
    u, o = uniform_world(), open_world()
    out = {}
    base = dict(v_min=0.0, v_max=0.5, w_max=2.0, acc_v=1.0, acc_w=8.0, dt_control=0.1, dt_sim=0.05, n_v=4, n_w=9, n_steps=12)
    ux, uy = cell_centre(u, 20, 23)
    out["ties"] = (uniform_world, lpm.Params(**dict(base, w_field=1, w_heading=0, w_speed=0, w_clear=0)), (ux, uy, F32(0.3)), 0.2, 0.0)
    px, py = cell_centre(pocket_world(), 15, 15)
    out["pocket"] = (pocket_world, lpm.Params(**dict(base, v_min=0.3, acc_v=0.0, w_field=1)), (px, py, F32(0.0)), 0.4, 0.0)
    out["off_grid"] = (uniform_world, lpm.Params(**dict(base, w_field=1)), (F32(-1.5), uy, F32(0.0)), 0.0, 0.0)
    wx, wy = cell_centre(u, 0, 10)
    out["on_wall"] = (uniform_world, lpm.Params(**dict(base, w_field=1)), (wx, wy, F32(0.0)), 0.0, 0.0)
    out["unreached"] = (pocket_world, lpm.Params(**dict(base, w_field=1)), cell_centre(pocket_world(), 25, 25) + (F32(0.0),), 0.0, 0.0)
    gx, gy = cell_centre(u, 50, 23)
    out["reached"] = (uniform_world, lpm.Params(**dict(base, w_field=1)), (gx, gy, F32(2.0)), 0.1, 0.1)
    fast = dict(base, v_max=1.0, acc_v=10.0, n_steps=40, n_w=17, w_max=3.0, acc_w=30.0, w_field=3, w_heading=2, w_clear=1, w_speed=5)
    for name, cell, th in (("exit_left", (2, 18), math.pi), ("exit_right", (38, 18), 0.0), ("exit_bottom", (20, 2), -math.pi / 2),
                           ("exit_top", (20, 34), math.pi / 2)):
        x, y = cell_centre(o, *cell)
        out[name] = (open_world, lpm.Params(**fast), (x, y, F32(th)), 0.8, 0.0)
    out["wrap"] = (uniform_world, lpm.Params(**dict(base, n_steps=30, w_field=2, w_heading=3, w_clear=1, w_speed=1)), (ux, uy, F32(3.1)), 0.3, 1.0)
    out["v_lo_above_v_hi"] = (uniform_world, lpm.Params(**dict(base, w_field=1, w_heading=1)), (ux, uy, F32(0.0)), 0.9, -5.0)
    out["one_v"] = (uniform_world, lpm.Params(**dict(base, n_v=1, w_field=1, w_heading=1)), (ux, uy, F32(-2.0)), 0.2, 0.5)
    out["one_w"] = (uniform_world, lpm.Params(**dict(base, n_w=1, w_field=1, w_speed=3)), (ux, uy, F32(0.5)), 0.2, 0.5)
    out["one_candidate"] = (uniform_world, lpm.Params(**dict(base, n_v=1, n_w=1, w_field=1)), (ux, uy, F32(0.0)), 0.2, 0.0)
    out["reverse"] = (uniform_world, lpm.Params(**dict(base, v_min=-0.4, w_field=4, w_heading=0, w_speed=0)), (ux, uy, F32(math.pi)), -0.1, 0.0)
    return out


def test_conditions_are_reached():
    cases = condition_cases()
    seen = {}

    def run(name):
        factory, p, pose, v, w = cases[name]
        assert p.ok() and not p.can_skip_a_cell(MPC), name
        stats = {}
        r, cs = lpm.command(factory(), p, pose, v, w, stats)
        seen[name] = stats
        return r, cs, p

    r, cs, p = run("ties")
    ties = int((cs == cs.min()).sum())
    assert ties > 1 and int(r["index"]) == int(np.flatnonzero(cs == cs.min())[0]) and int(r["flags"]) == 0
    print("ties: candidates sharing the least cost:", ties, "winner", int(r["index"]))

    r, cs, p = run("pocket")
    assert int(r["flags"]) == lpm.BLOCKED and int(r["index"]) == -1 and (cs == lpm.COST_NONE).all()
    assert (float(r["trans_v"]), float(r["angular_v"]), int(r["n_admissible"])) == (0.0, 0.0, 0)
    print("pocket: inadmissible candidates:", len(cs))

    kinds = 0
    for name in ("off_grid", "on_wall", "unreached"):
        r, cs, p = run(name)
        assert int(r["flags"]) == lpm.OFF_FIELD and cs is None and int(r["cost"]) == lpm.COST_NONE, name
        kinds += 1
    w = pocket_world()
    assert w.tcell[25, 25] and int(w.field[25, 25]) == nm.UNREACHED and w.cell(*cases["off_grid"][2][:2]) is None and not uniform_world().tcell[10, 0]
    print("OFF_FIELD kinds reached:", kinds)

    r, cs, p = run("reached")
    assert int(r["flags"]) == lpm.REACHED and int(r["cost"]) == 0 and cs is None
    print("REACHED: 1")

    for name, side in (("exit_left", "left"), ("exit_right", "right"), ("exit_bottom", "bottom"), ("exit_top", "top")):
        r, cs, p = run(name)
        assert seen[name].get(side, 0) > 0 and int(r["flags"]) == 0 and int(r["n_admissible"]) > 0, (name, seen[name])
        print(name, "rollouts that left the grid on that side:", seen[name][side], "admissible:", int(r["n_admissible"]))

    r, cs, p = run("wrap")
    assert seen["wrap"].get("wrapped", 0) > 0 and int(r["flags"]) == 0
    print("wrap: candidates whose heading stepped through +-pi:", seen["wrap"]["wrapped"])

    r, cs, p = run("v_lo_above_v_hi")
    vt, wt = lpm.tables(p, cases["v_lo_above_v_hi"][3], cases["v_lo_above_v_hi"][4])
    assert (vt == p.v_max).all() and (wt == -p.w_max).all() and int(r["flags"]) == 0
    print("v_lo > v_hi: tables collapse to", float(vt[0]), float(wt[0]))

    for name in ("one_v", "one_w", "one_candidate"):
        r, cs, p = run(name)
        assert len(cs) == p.n_v * p.n_w and int(r["flags"]) == 0, name
        print(name, "candidates:", len(cs), "winner", int(r["index"]))

    r, cs, p = run("reverse")
    vt, _ = lpm.tables(p, cases["reverse"][3], cases["reverse"][4])
    assert vt[0] < 0 and float(r["trans_v"]) < 0 and int(r["flags"]) == 0      # facing away from the goal: backing up wins
    print("reverse: v table from", float(vt[0]), "command", float(r["trans_v"]))


def test_parameter_rules():
    good = dict(LOOP_PARAMS)
    assert lpm.Params(**good).ok()
    for bad in (dict(v_min=0.6), dict(w_max=-0.1), dict(dt_control=0.0), dict(dt_sim=-1.0), dict(acc_v=float("nan")), dict(v_max=float("inf")),
                dict(n_v=0), dict(n_v=65), dict(n_w=1026), dict(n_steps=256), dict(n_steps=0), dict(w_field=65536), dict(w_speed=-1)):
        assert not lpm.Params(**dict(good, **bad)).ok(), bad
    assert lpm.Params(**dict(good, v_max=1.5)).can_skip_a_cell(0.05) and not lpm.Params(**good).can_skip_a_cell(0.05)
    assert lpm.Params(**good).staged(CPM) and not lpm.Params(**dict(good, v_max=1.0, dt_sim=0.05, n_steps=255)).staged(CPM)
