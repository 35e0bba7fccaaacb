"""The local planner's moving rule on the GPU (bl_localplan_commands_moving, bl_localplan_debug_costs_moving,
bl_obstracks_compose_static) against its model (tests/local_plan_moving_model.py) on the cases of
tests/local_plan_moving_cases.py: results, the cost and the first hit of every candidate, byte for byte and with nothing left out;
the device's paths (the boxes' table, the boxes per step, nothing kept; the window staged or not) asserted through the debug calls.
Tracks are placed by bl_obstracks_upload."""
import ctypes as C

import numpy as np
import pytest

import botlab_amd as bl
from botlab_amd import _capi, host
import local_plan_model as lpm
import local_plan_moving_cases as mc
import local_plan_moving_model as lmm
import obstacle_tracks_model as tm
from test_gpu_local_plan import _device, _same_record, _set, _state

pytestmark = pytest.mark.gpu
F32 = np.float32
CPM = mc.CPM


class _Env:
    def __init__(self, ctx):
        self.ctx, self.lp, self.trackers = ctx, bl.LocalPlanner(ctx), {}

    def tracker(self, w, h):
        if (w, h) not in self.trackers:
            layer = bl.ObstacleLayer(w, h, ttl_scans=3, min_hits=1, ctx=self.ctx)
            self.trackers[(w, h)] = (bl.ObstacleTracker(layer, **dict(tm.BASE, max_cells=9)), layer)
        return self.trackers[(w, h)][0]

    def close(self):
        self.lp.close()
        for t, l in self.trackers.values():
            t.close()
            l.close()


@pytest.fixture(scope="module")
def env(gpu_ctx):
    e = _Env(gpu_ctx)
    yield e
    e.close()


def _upload(tr, slots):
    tr.upload(slots, 0, int(slots["id"].max()) + 1, 1)


def _run(env, name):
    """Everything the device hands back for a case against the model.  Returns (the device's records, the moving path of the call)."""
    case = mc.get(name)
    world = case.world()
    nf, tr, lp, m = _device(world, env.ctx), env.tracker(world.w, world.h), env.lp, case.m
    _upload(tr, case.slots)
    _set(lp, case.p)
    dev = [_state(*s) for s in case.states]
    got = lp.commands_moving(nf, tr, dev, m.q, m.margin, m.lead)
    path = lp.debugMovingPath()
    assert lp.debugPath() == (0 if case.p.staged(CPM) else 1)
    rolled = [s for s, (rec, _, _) in zip(case.states, mc.model(name)) if int(rec["flags"]) in (0, lpm.BLOCKED)]
    assert path == (lmm.moving_path(world, case.p, case.slots, m, rolled[0][0]) if rolled else lmm.PATH_NONE), (name, path)
    for k, (exp, ecs, efh) in enumerate(mc.model(name)):
        assert _same_record(got[k], exp), (name, k, got[k], exp)
        cs, fh = lp.costs_moving(nf, tr, dev[k], m.q, m.margin, m.lead)
        assert lp.debugMovingPath() == lmm.moving_path(world, case.p, case.slots, m, case.states[k][0]), (name, k)
        bad = np.flatnonzero(cs.ravel() != ecs)
        assert len(bad) == 0, (name, k, len(bad), int(bad[0]), int(cs.ravel()[bad[0]]), int(ecs[bad[0]]))
        bad = np.flatnonzero(fh.ravel() != efh)
        assert len(bad) == 0, (name, k, len(bad), int(bad[0]), int(fh.ravel()[bad[0]]), int(efh[bad[0]]))
    return got, path


CONDITIONS = [n for n in mc.BUILDERS if not n.startswith(("edge_", "table_")) and n not in ("reach_cull", "seven_states", "partial_last_workgroup")]


@pytest.mark.parametrize("name", CONDITIONS)
def test_conditions_equal_the_model(env, name):
    _run(env, name)


def test_edges_equal_the_model(env):
    for mg, side, on in mc.EDGES:
        got, _ = _run(env, "edge_%d_%s_%s" % (mg, side, "on" if on else "beyond"))
        assert int(got[0]["flags"]) == (lpm.BLOCKED if on else 0)


@pytest.mark.parametrize("name", ["no_used", "unused_kinds"])
def test_no_used_slot_is_the_plain_call_byte_for_byte(env, name):
    got, path = _run(env, name)
    case = mc.get(name)
    plain = env.lp.commands(_device(case.world(), env.ctx), [_state(*s) for s in case.states])
    assert got.tobytes() == plain.tobytes() and path == lmm.PATH_NONE
    world = case.world()
    cs, fh = env.lp.costs_moving(_device(world, env.ctx), env.tracker(world.w, world.h), _state(*case.states[0]), case.m.q, case.m.margin, case.m.lead)
    assert np.array_equal(cs, env.lp.costs(_device(world, env.ctx), _state(*case.states[0]))) and not fh.any()


@pytest.mark.parametrize("kept,v_max", mc.TABLE_SIDES)
def test_both_sides_of_the_table_rule_under_both_window_paths(env, kept, v_max):
    """BL_LOCALPLAN_MOVING_BYTES: kept * n_steps * 8 bytes; at 255 steps TABLE_FITS boxes fit and one more does not."""
    assert mc.TABLE_FITS * 255 * 8 <= lmm.MOVING_BYTES < (mc.TABLE_FITS + 1) * 255 * 8
    _, path = _run(env, "table_%d_%s" % (kept, "staged" if v_max == 0.1 else "grids"))
    assert path == (2 if kept == 0 else 0 if kept == mc.TABLE_FITS else 1)
    assert env.lp.debugPath() == (0 if v_max == 0.1 else 1)


def test_the_reach_cull_decides_no_result(env):
    _, path = _run(env, "reach_cull")
    assert path == lmm.PATH_TABLE


def test_seven_states_in_one_call(env):
    got, _ = _run(env, "seven_states")
    assert {0, lpm.REACHED, lpm.OFF_FIELD, lpm.BLOCKED} <= {int(f) for f in got["flags"]}
    case = mc.get("seven_states")
    world = case.world()
    nf, tr = _device(world, env.ctx), env.tracker(world.w, world.h)
    for k, s in enumerate(case.states):                                   # and each alone is what it was among the seven
        one = env.lp.commands_moving(nf, tr, [_state(*s)], case.m.q, case.m.margin, case.m.lead)
        assert one[0].tobytes() == got[k].tobytes(), k
    assert len(env.lp.commands_moving(nf, tr, [], 2)) == 0
    tv, av, fl = env.lp.command_moving(nf, tr, *_state(*case.states[0]), case.m.q, case.m.margin, case.m.lead)
    assert (F32(tv).tobytes(), F32(av).tobytes(), fl) == (got[0]["trans_v"].tobytes(), got[0]["angular_v"].tobytes(), int(got[0]["flags"]))


def test_a_partial_last_workgroup(env):
    _run(env, "partial_last_workgroup")


def test_refusals(env, gpu_ctx):
    world = mc.small_world()
    nf, lp, lib = _device(world, gpu_ctx), env.lp, gpu_ctx.lib
    out = np.zeros(1, host.LOCALPLAN_RESULT_DTYPE)
    for name, (p, m, shape, states) in mc.refusals().items():
        assert lmm.refusal(world, p, m, shape, states)
        tr = env.tracker(*shape)
        _set(lp, p)
        mv = _capi.LocalPlanMoving(m.q, m.margin, m.lead, m.reserved)
        s = (_capi.LocalPlanState * 1)(lp._state(_state(*states[0])))
        assert lib.bl_localplan_commands_moving(lp.h, nf.h, tr.h, C.byref(mv), s, 1, out.ctypes.data) == 2, name
        assert lib.bl_localplan_debug_costs_moving(lp.h, nf.h, tr.h, C.byref(mv), C.byref(s[0]), None, None) == 2, name
    # a tracker without parameters: BL_ERR_STATE; a planner that has made no moving call: path -1
    good = mc.get("no_used")
    _set(lp, good.p)
    h = C.c_void_p()
    assert lib.bl_obstracks_create(gpu_ctx.h, world.w, world.h, C.byref(h)) == 0
    try:
        mv = _capi.LocalPlanMoving(2, 0, 0, 0)
        s = (_capi.LocalPlanState * 1)(lp._state(_state(*good.states[0])))
        assert lib.bl_localplan_commands_moving(lp.h, nf.h, h, C.byref(mv), s, 1, out.ctypes.data) == 4
    finally:
        lib.bl_obstracks_destroy(h)
    fresh = bl.LocalPlanner(gpu_ctx)
    try:
        assert fresh.debugMovingPath() == -1
    finally:
        fresh.close()


@pytest.mark.parametrize("w,h", [(37, 23), (64, 64)])
def test_compose_static(env, gpu_ctx, w, h):
    """After real updates with a moving 3 x 3 blob and a standing one (the layer's state placed by its upload), and after an upload
    of the tracker."""
    rng = np.random.default_rng(w)
    cells = rng.integers(-100, 100, (h, w)).astype(np.int8)
    live_at = mc.blob_scene(w, h)
    grid = bl.OccupancyGrid.from_cells(cells, mc.cpu.ORIGIN, mc.cpu.MPC, cellsPerMeter=CPM, ctx=gpu_ctx)
    tr = env.tracker(w, h)
    layer = tr.layer
    model = tm.Tracker(w, h, **dict(tm.BASE, max_cells=9))
    out = None
    try:
        tr.reset()

        def place(live, n):
            layer.upload(live.astype(np.uint8), np.where(live, n, 0).astype(np.uint32), n)

        place(live_at(1), 1)
        out = tr.composeStatic(grid)                                          # fresh, no blobs: the layer's compose
        assert np.array_equal(out.cells(), layer.compose(grid, None).cells())
        left_out = 0
        for n in range(1, 7):
            live = live_at(n)
            place(live, n)
            tr.update()
            model.update(live, n)
            exp = lmm.compose_static(model, live, n, cells)
            tr.composeStatic(grid, out)
            assert np.array_equal(out.cells(), exp), n
            left_out += int(np.count_nonzero(exp != np.where(live, 127, cells)))
        assert left_out > 0 and np.count_nonzero(exp == 127) >= 9
        big = live.copy()
        big[1:5, 15:20] = True                                                # 20 cells: no track
        place(big, 7)
        tr.update()
        model.update(big, 7)
        assert np.array_equal(tr.composeStatic(grid, out).cells(), lmm.compose_static(model, big, 7, cells))
        place(big, 9)                                                         # the layer ahead of the tracks
        with pytest.raises(bl.BotlabHipError, match="status 4"):
            tr.composeStatic(grid, out)
        place(big, 7)
        slots, st = tr.download()
        tr.upload(slots, st["n"], st["next_id"], 0)                           # after an upload: no blobs
        assert np.array_equal(tr.composeStatic(grid, out).cells(), np.where(big, 127, cells))
        planner = bl.MotionPlanner(ctx=gpu_ctx)
        try:
            planner.setMapWithStaticObstacles(grid, layer, tr)
            assert np.array_equal(planner.composed_.cells(), np.where(big, 127, cells))
        finally:
            if planner.composed_ is not None:
                planner.composed_.close()
            planner.distances_.close()
    finally:
        if out is not None:
            out.close()
        grid.close()
        tr.reset()
