"""The local planner on the GPU (bl_localplan_*, botlab_amd/csrc/bl_localplan.hip) on the inputs of tests/local_plan_cases.py: launch
shapes with several workgroups per state and a partial last one, several states at several workgroups each, partials left by an
earlier call, ties decided in every stage of the reduction, costs beyond 2^32, the (-1, 0) strip of grid coordinates, the debug
costs of flagged states, headings at +-(float)pi and at the limit, one handle across growing and shrinking calls, and a field that
changes under the planner.  The reference is tests/local_plan_model.py, byte for byte: the command records, all n_v * n_w costs,
the tables and sampled rollouts (tests/test_gpu_local_plan.py's _compare).  tests/test_local_plan_cases_cpu.py shows that each case
is what it claims to be."""
import ctypes as C

import numpy as np
import pytest

import botlab_amd as bl
from botlab_amd import _capi
import local_plan_cases as lc
import local_plan_model as lpm
import nav_field_cases as nc
import test_local_plan_model_cpu as cpu
from test_gpu_local_plan import _compare, _device, _ragged_start, _same_record, _set, _state, lp  # noqa: F401  (lp: the module's fixture)

pytestmark = pytest.mark.gpu
F32 = np.float32


def _assert_records(got, exp, what):
    assert len(got) == len(exp)
    for k in range(len(exp)):
        assert _same_record(got[k], exp[k]), (what, k, got[k], exp[k])


@pytest.mark.parametrize("name", lc.SINGLE)
def test_case_equals_the_model(gpu_ctx, lp, name):
    factory, p, states = lc.get(name)
    world = factory()
    if name.startswith("shape"):
        assert all(a.tobytes() == b.tobytes() for a, b in zip(states[0][0], _ragged_start(world)))
    recs = _compare(lp, _device(world, gpu_ctx), world, p, states, samples=2)
    _assert_records(recs, lc.model_records((factory, p, states)), name)            # (the model twice: what the builder asserted on)
    print(name, lc.launch_shape(p), recs[0])


def test_sixty_six_states_at_two_workgroups_each(gpu_ctx, lp):
    """One call against the model; the second list on the same handle, straight after it, so that the slots of its flagged states
    still hold the first call's partials; each state alone gives the bytes it gave among the others."""
    first, second = lc.get("many_first"), lc.get("many_second")
    world = first[0]()
    nf = _device(world, gpu_ctx)
    _set(lp, first[1])
    dev1, dev2 = [_state(*s) for s in first[2]], [_state(*s) for s in second[2]]
    got1 = lp.commands(nf, dev1)
    got2 = lp.commands(nf, dev2)
    _assert_records(got1, lc.model_records(first), "first")
    _assert_records(got2, lc.model_records(second), "second")
    for got, dev in ((got1, dev1), (got2, dev2)):
        for k in range(66):
            one = lp.commands(nf, [dev[k]])
            assert len(one) == 1 and one[0].tobytes() == got[k].tobytes(), k
    _compare(lp, nf, world, first[1], first[2], samples=1)


def test_one_handle_across_growing_and_shrinking_calls(gpu_ctx):
    """d_out is one buffer for results, debug costs and debug poses: 64 x 1025 costs, one result, a rollout, 66 results, 35 costs, one
    result, each against the model."""
    world = cpu.uniform_world()
    nf = _device(world, gpu_ctx)
    many = lc.get("many_first")
    free = many[2][63]
    big = lpm.Params(**dict(lc.SHAPE, n_v=64, n_w=1025, n_steps=1))
    small = lpm.Params(**dict(lc.SHAPE, n_v=5, n_w=7, n_steps=10))
    h = bl.LocalPlanner(gpu_ctx)
    try:
        def costs(p):
            _set(h, p)
            got = h.costs(nf, _state(*free)).ravel()
            assert np.array_equal(got, lpm.costs(world, p, *free)), (p.n_v, p.n_w)

        def one(p):
            _set(h, p)
            got = h.commands(nf, [_state(*free)])
            exp, _ = lpm.command(world, p, *free)
            assert len(got) == 1 and _same_record(got[0], exp) and int(exp["flags"]) == 0, (got, exp)
            return int(exp["index"])

        costs(big)
        c = one(big)
        r = h.rollout(nf, _state(*free), c)
        vt, wt = lpm.tables(big, free[1], free[2])
        e = lpm.rollout(free[0], vt[c % 64], wt[c // 64], big)
        assert len(r) == 1 and (r["x"][0], r["y"][0], r["theta"][0]) == e[0]
        _set(h, many[1])
        _assert_records(h.commands(nf, [_state(*s) for s in many[2]]), lc.model_records(many), "66 states")
        costs(small)
        one(small)
    finally:
        h.close()


def test_the_field_changes_under_the_planner(gpu_ctx, lp):
    """One NavigationField handle: goal A, goal B, a refused compute (the handle keeps no field), a recompute, then the distance
    grid transformed to another size."""
    a = cpu.uniform_world()
    b = cpu.make_world(cpu.uniform_cells(61, 47), cpu.ORIGIN, cpu.MPC, [(10, 23)], 0, cpu.SMALL_NAV)[0]
    p = lpm.Params(**dict(lc.SHAPE, v_min=0.0, n_v=5, n_w=9, n_steps=10))
    states = [(lc.on_cell(a, 30.5, 23.5, 0.0), F32(0.2), F32(0.0)), (lc.on_cell(a, 10.5, 23.5, 1.0), F32(0.1), F32(0.3)),
              (lc.on_cell(a, 50.5, 23.5, -1.0), F32(0.0), F32(0.0)), (lc.on_cell(a, 40.25, 5.75, 2.0), F32(0.3), F32(-1.0))]
    g = bl.OccupancyGrid.from_cells(a.cells, a.origin, a.mpc, cellsPerMeter=lc.CPM, ctx=gpu_ctx)
    d = bl.ObstacleDistanceGrid(ctx=gpu_ctx)
    d.setDistances(g)
    nf = bl.NavigationField(gpu_ctx)
    try:
        def compute(world):
            n = world.nav
            nf.compute(d, _capi.NavFieldParams(n.minDistanceToObstacle, n.maxDistanceWithCost, n.distanceCostExponent, n.obstacle_gain, n.reach_cells),
                       world.goals)
            assert np.array_equal(nf.cells(), world.field)

        def refused(status):
            st = _state(*states[0])
            for call in (lambda: lp.commands(nf, [st]), lambda: lp.costs(nf, st), lambda: lp.rollout(nf, st, 0)):
                with pytest.raises(bl.BotlabHipError, match="status %d" % status):
                    call()

        compute(a)
        ra = _compare(lp, nf, a, p, states, samples=1)
        compute(b)
        rb = _compare(lp, nf, b, p, states, samples=1)
        assert any(not _same_record(x, y) for x, y in zip(ra, rb))
        assert int(ra[2]["flags"]) == lpm.REACHED and int(rb[1]["flags"]) == lpm.REACHED and int(rb[2]["flags"]) == 0
        # a compute refused by a bad parameter leaves the handle without a field
        bad = _capi.NavFieldParams(b.nav.minDistanceToObstacle, b.nav.maxDistanceWithCost, b.nav.distanceCostExponent, b.nav.obstacle_gain, 1025)
        g32 = np.array(b.goals, np.int32)
        assert gpu_ctx.lib.bl_navfield_compute(nf.h, d.h, C.byref(bad), g32.ctypes.data, len(g32)) == _capi.BL_ERR_ARG
        _set(lp, p)
        refused(_capi.BL_ERR_STATE)
        assert _capi.BL_ERR_STATE == 4
        compute(a)
        _assert_records(lp.commands(nf, [_state(*s) for s in states]), ra, "recomputed")
        # the distance grid transformed to another size (as tests/test_gpu_nav_field_edges.py resizes it)
        w2 = nc.world("small_33x33")
        g2 = bl.OccupancyGrid.from_cells(w2.cells, a.origin, nc.MPC, cellsPerMeter=nc.CPM, ctx=gpu_ctx)
        d.setDistances(g2)
        refused(_capi.BL_ERR_STATE)
        g2.close()
    finally:
        nf.close()
        d.close()
        g.close()


def test_heading_limit(gpu_ctx, lp):
    """BL_LOCALPLAN_MAX_THETA is accepted (test_case_equals_the_model[heading_max] compares it); the next float is refused by every
    call that takes a state.  By the error return alone: no larger heading goes to the device."""
    world = cpu.uniform_world()
    nf = _device(world, gpu_ctx)
    factory, p, states = lc.get("heading_max")
    _set(lp, p)
    (pose, v, w), = states
    assert pose[2] == F32(65536.0) and len(lp.commands(nf, [_state(pose, v, w)])) == 1
    for over in (np.nextafter(F32(65536.0), F32(np.inf)), np.nextafter(F32(-65536.0), F32(-np.inf))):
        assert not lpm.state_ok((pose[0], pose[1], over), v, w)
        st = _state((pose[0], pose[1], over), v, w)
        for call in (lambda: lp.commands(nf, [st]), lambda: lp.costs(nf, st), lambda: lp.rollout(nf, st, 0), lambda: lp.tables(st),
                     lambda: lp.commands(nf, [_state(pose, v, w), st])):
            with pytest.raises(bl.BotlabHipError, match="status 2"):
                call()
