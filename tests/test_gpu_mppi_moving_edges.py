"""The sampling local planner's moving rule on the GPU against tests/mppi_model.py, byte for byte, on the cases of
tests/mppi_moving_cases.py: used slots in every wave of the table, the grids read directly with the rule on, a fall-back caused by a
box alone, first hits after the map has refused, the ends of (steps_per_update, lead_steps, velocity), clamped boxes, and the mixed
batch.  tests/test_mppi_moving_cases_cpu.py proves that each case reaches its path; tracks are placed by bl_obstracks_upload."""
import numpy as np
import pytest

import botlab_amd as bl
import mppi_cases as mc
import mppi_model as mm
import mppi_moving_cases as mv
import obstacle_tracks_model as tm
from test_gpu_local_plan import _device

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(gpu_ctx):
    """The planner, and one tracker per grid shape: the tracker's shape must be the world's."""
    mp = bl.MppiPlanner(gpu_ctx)
    made = {}

    def tracker(world):
        key = (world.w, world.h)
        if key not in made:
            layer = bl.ObstacleLayer(world.w, world.h, ttl_scans=3, min_hits=1, ctx=gpu_ctx)
            made[key] = (bl.ObstacleTracker(layer, **dict(tm.BASE, max_cells=9)), layer)
        return made[key][0]

    yield mp, tracker
    mp.close()
    for tr, layer in made.values():
        tr.close()
        layer.close()


def _run(gpu_ctx, env, name, plan=True, samples=True):
    """The case's table uploaded; the debug call of its first state and the plan of all its states against the model."""
    mp, tracker = env
    case = mv.get(name)
    world = case.world()
    nf, tr = _device(world, gpu_ctx), tracker(world)
    tr.upload(case.slots, 0, int(case.slots["id"].max()) + 1, 1)
    moving = (case.m.q, case.m.margin, case.m.lead)
    out = {}
    if samples:
        u = None if case.u_in is None else case.u_in[0]
        out["samples"] = mc.compare_samples(bl, mp, nf, world, case.p, case.states[0], u, tr, moving, case.slots, case.m)
    if plan:
        out["plan"] = mc.compare_plan(bl, mp, nf, world, case.p, case.states, case.u_in, tr, moving, case.slots, case.m)
    out["path"] = mp.debugPath()
    return out


@pytest.mark.parametrize("name", ["every_wave", "full_table"])
def test_used_slots_beyond_the_first_wave(gpu_ctx, env, name):
    out = _run(gpu_ctx, env, name)
    costs, fh, _ = out["samples"]
    assert 0 < np.count_nonzero(fh) < len(fh) and (costs[fh > 0] == mm.COST_NONE).all() and out["path"] == 0


@pytest.mark.parametrize("name,path", [("direct_38", 1), ("staged_37", 0)])
def test_the_rule_with_the_grids_read_directly_and_with_the_window_staged(gpu_ctx, env, name, path):
    out = _run(gpu_ctx, env, name)
    costs, fh, _ = out["samples"]
    assert out["path"] == path and np.count_nonzero(fh) > 0 and (costs != mm.COST_NONE).any()
    assert int(out["plan"][0][0]["flags"]) in (0, mm.FELL_BACK)


def test_a_box_alone_makes_the_planner_fall_back(gpu_ctx, env):
    r, so = _run(gpu_ctx, env, "box_pillar")["plan"][0]
    assert int(r["flags"]) == mm.FELL_BACK and int(r["index_best"]) > 1 and int(r["cost_out"]) == int(r["cost_best"]) and so.any()
    mp, _ = env
    case = mv.get("box_pillar")
    plain, _ = mc.compare_plan(bl, mp, _device(case.world(), gpu_ctx), case.world(), case.p, case.states, case.u_in)[0]
    assert int(plain["flags"]) == 0
    r, _ = _run(gpu_ctx, env, "box_aside")["plan"][0]
    assert int(r["flags"]) == 0


@pytest.mark.parametrize("name", ["after_the_pillar", "out_and_back"])
def test_first_hits_of_samples_the_map_has_already_refused(gpu_ctx, env, name):
    """The debug call alone: the plan stops a rollout at its first refusal."""
    costs, fh, _ = _run(gpu_ctx, env, name, plan=False)["samples"]
    late = mv.refused_before_hit(mv.get(name))
    assert late.any() and (fh[late] > 0).all() and (costs[late] == mm.COST_NONE).all()


@pytest.mark.parametrize("name", ["timing_q%d_lead%d_v%d" % t for t in mv.TIMINGS] + ["floor_step"])
def test_time_divisor_and_sign(gpu_ctx, env, name):
    out = _run(gpu_ctx, env, name)
    fh = out["samples"][1]
    assert np.count_nonzero(fh) > 0 and len(set(fh.tolist())) > 2 and out["path"] == 0


def test_clamped_boxes_and_the_widest_margin(gpu_ctx, env):
    out = _run(gpu_ctx, env, "everywhere")
    r, so = out["plan"][0]
    assert int(r["flags"]) == mm.BLOCKED and (out["samples"][1] == 1).all() and not so.any()
    for name in ("corner_max", "corner_min"):
        out = _run(gpu_ctx, env, name)
        assert not out["samples"][1].any() and int(out["plan"][0][0]["flags"]) in (0, mm.FELL_BACK)


@pytest.mark.parametrize("name", ["batch", "batch_speeds"])
def test_the_mixed_batch_under_the_rule(gpu_ctx, env, name):
    """compare_plan plans the six states in one call and each alone; the debug call is of the normal state."""
    out = _run(gpu_ctx, env, name)
    assert [int(r["flags"]) & ~mm.FELL_BACK for r, _ in out["plan"]] == mc.BATCH_FLAGS
    assert np.count_nonzero(out["samples"][1]) > 0
