"""The local planner on the GPU (bl_localplan_*, botlab_amd/csrc/bl_localplan.hip) against its model (tests/local_plan_model.py):
commands, the cost of every candidate, the candidate tables and the rollouts of a sample of candidates (the winner among them), all
byte for byte, on the shapes at which the kernel takes another path."""
import functools
import math

import numpy as np
import pytest

import botlab_amd as bl
from botlab_amd import _capi
import helpers
import local_plan_model as lpm
import nav_field_model as nm
import test_local_plan_model_cpu as cpu

pytestmark = pytest.mark.gpu
F32 = np.float32
CPM = helpers.CPM_DEFAULT
_dev = {}


def _device(world, ctx):
    """(NavigationField, its distance grid and map) of a model world, once per world; the device's field is the model's."""
    key = id(world)
    if key not in _dev:
        g = bl.OccupancyGrid.from_cells(world.cells, world.origin, world.mpc, cellsPerMeter=CPM, ctx=ctx)
        d = bl.ObstacleDistanceGrid(ctx=ctx)
        d.setDistances(g)
        nf = bl.NavigationField(ctx)
        n = world.nav
        nf.compute(d, _capi.NavFieldParams(n.minDistanceToObstacle, n.maxDistanceWithCost, n.distanceCostExponent, n.obstacle_gain, n.reach_cells),
                   world.goals)
        assert np.array_equal(nf.cells(), world.field)
        _dev[key] = (nf, d, g, world)
    return _dev[key][0]


@pytest.fixture(scope="module")
def lp(gpu_ctx):
    p = bl.LocalPlanner(gpu_ctx)
    yield p
    p.close()


def _set(lp, p):
    lp.set_params(p.v_min, p.v_max, p.w_max, p.acc_v, p.acc_w, p.dt_control, p.dt_sim, p.n_v, p.n_w, p.n_steps, p.w_field, p.w_heading,
                  p.w_clear, p.w_speed)


def _state(pose, v, w, utime=99):
    return (bl.make_pose(pose[0], pose[1], pose[2], utime=utime), F32(v), F32(w))


def _same_record(got, exp):
    return all(got[k].tobytes() == exp[k].tobytes() for k in ("trans_v", "angular_v", "index", "n_admissible", "cost", "flags"))


def _compare(lp, nf, world, p, states, samples=4, seed=1):
    """Everything the device hands back for `states` (pose, v, w) against the model.  Returns the model's records."""
    _set(lp, p)
    dev_states = [_state(*s) for s in states]
    got = lp.commands(nf, dev_states)
    assert lp.debugPath() == (0 if p.staged(CPM) else 1)
    rng = np.random.default_rng(seed)
    recs = []
    for k, (pose, v, w) in enumerate(states):
        exp, ecs = lpm.command(world, p, pose, v, w)
        if ecs is None:                                      # flagged: nothing was rolled out for the command; the debug costs still are
            ecs = lpm.costs(world, p, pose, v, w)
        recs.append(exp)
        assert _same_record(got[k], exp), (k, got[k], exp)
        vt, wt = lp.tables(dev_states[k])
        evt, ewt = lpm.tables(p, v, w)
        assert vt.tobytes() == evt.tobytes() and wt.tobytes() == ewt.tobytes(), k
        cs = lp.costs(nf, dev_states[k]).ravel()
        bad = np.flatnonzero(cs != ecs)
        assert len(bad) == 0, (k, len(bad), int(bad[0]), int(cs[bad[0]]), int(ecs[bad[0]]))
        n = p.n_v * p.n_w
        pick = {0, n - 1} | {int(c) for c in rng.integers(0, n, samples)}
        if int(exp["index"]) >= 0:
            pick.add(int(exp["index"]))
        for c in sorted(pick):
            r = lp.rollout(nf, dev_states[k], c)
            e = lpm.rollout(pose, evt[c % p.n_v], ewt[c // p.n_v], p)
            assert (r["utime"] == 99).all()
            for a, col in (("x", 0), ("y", 1), ("theta", 2)):
                assert r[a].tobytes() == np.array([q[col] for q in e], np.float32).tobytes(), (k, c, a)
    return recs


# ---------------------------------------------------------------------------------------------------------------- conditions
@pytest.mark.parametrize("name", sorted(cpu.condition_cases()))
def test_condition_cases_equal_the_model(gpu_ctx, lp, name):
    factory, p, pose, v, w = cpu.condition_cases()[name]
    world = factory()
    recs = _compare(lp, _device(world, gpu_ctx), world, p, [(pose, v, w)])
    print(name, recs[0])


# ---------------------------------------------------------------------------------------------------------------- shapes
SHAPE = dict(v_min=-0.1, v_max=0.5, w_max=2.5, acc_v=3.0, acc_w=20.0, dt_control=0.1, dt_sim=0.05, w_field=7, w_heading=3, w_clear=2, w_speed=11)


def _ragged_start(world):
    return cpu.cell_centre(world, 24, 54) + (F32(0.4),)


@pytest.mark.parametrize("n_v,n_w,n_steps", [(1, 1, 7), (7, 9, 7), (63, 1, 7), (64, 1, 7), (8, 8, 7), (1, 65, 7), (5, 13, 7), (13, 5, 1), (33, 3, 20),
                                             (64, 1025, 1)])
def test_candidate_counts_on_the_ragged_grid(gpu_ctx, lp, n_v, n_w, n_steps):
    world = cpu.ragged_world()
    assert world.field.shape == (117, 203)
    p = lpm.Params(**dict(SHAPE, n_v=n_v, n_w=n_w, n_steps=n_steps))
    recs = _compare(lp, _device(world, gpu_ctx), world, p, [(_ragged_start(world), 0.2, -0.3)])
    assert int(recs[0]["flags"]) == 0 and int(recs[0]["n_admissible"]) > 0


@pytest.mark.parametrize("v_max,n_steps,staged", [(0.1, 255, True), (1.0, 255, False), (0.5, 148, True), (0.5, 152, False)])
def test_both_sides_of_the_window_rule(gpu_ctx, lp, v_max, n_steps, staged):
    """BL_LOCALPLAN_WINDOW_BYTES: (2 R + 1)^2 * 2 bytes with R = ceil(v * dt_sim * n_steps * cells_per_meter) + 2; at 0.5 m/s and
    5 cm cells R is 77 at 148 steps (48 050 bytes, staged) and 79 at 152 (50 562, not)."""
    world = cpu.ragged_world()
    p = lpm.Params(**dict(SHAPE, v_min=0.0, v_max=v_max, acc_v=20.0, n_v=3, n_w=5, n_steps=n_steps))
    assert p.staged(CPM) == staged
    recs = _compare(lp, _device(world, gpu_ctx), world, p, [(_ragged_start(world), 0.1, 0.1)], samples=1)
    assert lp.debugPath() == (0 if staged else 1) and int(recs[0]["n_admissible"]) > 0


def test_one_state_and_sixty_five_states_in_one_call(gpu_ctx, lp):
    world = cpu.uniform_world()
    nf = _device(world, gpu_ctx)
    p = lpm.Params(**dict(SHAPE, n_v=5, n_w=7, n_steps=10))
    rng = np.random.default_rng(4)
    states = []
    for k in range(65):
        x, y = rng.uniform(-2.0, world.w + 2.0), rng.uniform(-2.0, world.h + 2.0)      # some off the grid, some on the wall
        pose = (F32(float(F32(world.origin[0])) + x * float(world.mpc)), F32(float(F32(world.origin[1])) + y * float(world.mpc)), F32(rng.uniform(-4, 4)))
        states.append((pose, F32(rng.uniform(-0.1, 0.5)), F32(rng.uniform(-2.5, 2.5))))
    states[7] = (cpu.cell_centre(world, 50, 23) + (F32(1.0),), F32(0.1), F32(0.0))          # on the goal
    _set(lp, p)
    many = lp.commands(nf, [_state(*s) for s in states])
    flags = set()
    for k, (pose, v, w) in enumerate(states):
        exp, _ = lpm.command(world, p, pose, v, w)
        assert _same_record(many[k], exp), (k, many[k], exp)
        one = lp.commands(nf, [_state(pose, v, w)])
        assert len(one) == 1 and one[0].tobytes() == many[k].tobytes(), k
        flags.add(int(exp["flags"]))
    assert {0, lpm.REACHED, lpm.OFF_FIELD} <= flags
    assert len(lp.commands(nf, [])) == 0
    tv, av, fl = lp.command(nf, *_state(*states[0]))
    assert (F32(tv).tobytes(), F32(av).tobytes(), fl) == (many[0]["trans_v"].tobytes(), many[0]["angular_v"].tobytes(), int(many[0]["flags"]))


def test_closed_loop_twenty_ticks(gpu_ctx, lp):
    world, _, _ = cpu.loop_world()
    nf = _device(world, gpu_ctx)
    p = lpm.Params(**cpu.LOOP_PARAMS)
    _set(lp, p)

    def step(pose, v, w):
        exp, _ = lpm.command(world, p, pose, v, w)
        got = lp.commands(nf, [_state(pose, v, w)])[0]
        assert _same_record(got, exp), (pose, got, exp)
        return got

    recs, poses, cells = cpu.run_loop(world, p, cpu.loop_start(world), 20, step)
    assert len(recs) == 20 and all(int(r["flags"]) == 0 for r in recs)
    assert math.hypot(float(poses[-1][0]) - float(poses[0][0]), float(poses[-1][1]) - float(poses[0][1])) > 0.2


# ---------------------------------------------------------------------------------------------------------------- errors
def test_error_returns(gpu_ctx):
    world = cpu.uniform_world()
    nf = _device(world, gpu_ctx)
    st = _state(cpu.cell_centre(world, 20, 23) + (F32(0.0),), 0.1, 0.0)
    fresh = bl.LocalPlanner(gpu_ctx)
    try:
        for call in (lambda: fresh.commands(nf, [st]), lambda: fresh.tables(st), lambda: fresh.lastDeviceMs()):
            with pytest.raises(bl.BotlabHipError, match="status 4"):                  # before set_params: BL_ERR_STATE
                call()
        good = dict(cpu.LOOP_PARAMS)
        for bad in (dict(v_min=0.6), dict(w_max=-0.1), dict(dt_control=0.0), dict(dt_sim=-1.0), dict(acc_v=float("nan")), dict(v_max=float("inf")),
                    dict(n_v=0), dict(n_v=65), dict(n_w=1026), dict(n_steps=256), dict(w_field=65536), dict(w_speed=-1)):
            with pytest.raises(bl.BotlabHipError, match="status 2"):
                fresh.set_params(**dict(good, **bad))
        assert fresh.params is None
        fresh.set_params(**good)
        assert fresh.debugPath() == -1
        empty = bl.NavigationField(gpu_ctx)
        try:
            with pytest.raises(bl.BotlabHipError, match="status 4"):                  # a field handle without a field
                fresh.commands(empty, [st])
        finally:
            empty.close()
        fresh.set_params(**dict(good, v_max=1.5))                                     # 1.5 m/s * 0.05 s > 0.05 m: a step can skip a cell
        for call in (lambda: fresh.commands(nf, [st]), lambda: fresh.costs(nf, st), lambda: fresh.rollout(nf, st, 0)):
            with pytest.raises(bl.BotlabHipError, match="status 2"):
                call()
        fresh.set_params(**good)
        with pytest.raises(bl.BotlabHipError, match="status 2"):
            fresh.commands(nf, [_state((F32("nan"), F32(0), F32(0)), 0.0, 0.0)])
        with pytest.raises(bl.BotlabHipError, match="status 2"):
            fresh.rollout(nf, st, good["n_v"] * good["n_w"])
        assert len(fresh.commands(nf, [st])) == 1 and fresh.lastDeviceMs() > 0
    finally:
        fresh.close()
