"""The closed loop of tests/test_obstacle_layer_model_cpu.py wholly on the device: every tick the obstacle layer's update and compose,
ObstacleDistanceGrid.setDistances of the composed grid, NavigationField.compute and LocalPlanner's command.  The composed grid, the
field, the commands and so the poses equal the model's tick by tick; the robot goes round a box its map does not know."""
import numpy as np
import pytest

import botlab_amd as bl
from botlab_amd import _capi
import local_plan_model as lpm
import test_obstacle_layer_model_cpu as cpu

pytestmark = pytest.mark.gpu
F32 = np.float32


def test_closed_loop_on_the_device_equals_the_model(gpu_ctx):
    cells, truth = cpu.scene_cells()
    p = lpm.Params(**cpu.LOOP_PARAMS)
    grid = bl.OccupancyGrid.from_cells(cells, cpu.ORIGIN, cpu.MPC, cellsPerMeter=cpu.CPM, ctx=gpu_ctx)
    layer = bl.ObstacleLayer(cpu.SCENE_W, cpu.SCENE_H, ctx=gpu_ctx, **cpu.SCENE_LAYER)
    dist = bl.ObstacleDistanceGrid(ctx=gpu_ctx)
    nf = bl.NavigationField(gpu_ctx)
    lp = bl.LocalPlanner(gpu_ctx)
    lp.set_params(p.v_min, p.v_max, p.w_max, p.acc_v, p.acc_w, p.dt_control, p.dt_sim, p.n_v, p.n_w, p.n_steps, p.w_field, p.w_heading, p.w_clear,
                  p.w_speed)
    n = cpu.SCENE_NAV
    navp = _capi.NavFieldParams(n["minDistanceToObstacle"], n["maxDistanceWithCost"], n["distanceCostExponent"], n["obstacle_gain"], cpu.SCENE_REACH)
    composed = None
    seen = dict(ticks=0, fields=set())
    try:
        def on_tick(tick, model, scan, pose, exp_composed, world):
            nonlocal composed
            layer.update(grid, scan, bl.make_pose(pose[0], pose[1], pose[2], utime=scan.utime))
            composed = layer.compose(grid, composed)
            dist.setDistances(composed)
            nf.compute(dist, navp, [cpu.SCENE_GOAL])
            assert np.array_equal(layer.classes(), model.classes), tick
            assert np.array_equal(composed.cells(), exp_composed), tick
            assert np.array_equal(nf.cells(), world.field), tick
            seen["ticks"] += 1
            seen["fields"].add(exp_composed.tobytes())

        def step(world, pose, v, w):
            exp, _ = lpm.command(world, p, pose, v, w)
            got = lp.commands(nf, [(bl.make_pose(pose[0], pose[1], pose[2], utime=99), F32(v), F32(w))])[0]
            for k in ("trans_v", "angular_v", "index", "n_admissible", "cost", "flags"):
                assert got[k].tobytes() == exp[k].tobytes(), (len(seen["fields"]), k, got, exp)
            return got

        recs, poses, steps, model, totals, ever = cpu.run_scene(True, step=step, on_tick=on_tick)
        count, last, nn = layer.download()
        assert nn == model.n and np.array_equal(count, model.count) and np.array_equal(last, model.last)
        assert layer.stats() == model.stats()
    finally:
        for x in (lp, nf, dist, layer, grid) + ((composed,) if composed is not None else ()):
            x.close()
    inside = sum(1 for c in steps if c is None or truth[c[1], c[0]] > 0)
    print(f"on the device: flags {int(recs[-1]['flags'])} at tick {len(recs) - 1}, {inside} integration steps inside the box, "
          f"{len(seen['fields'])} distinct composed grids over {seen['ticks']} ticks, rays by class {totals.tolist()}")
    assert int(recs[-1]["flags"]) == lpm.REACHED and inside == 0 and len(seen["fields"]) > 3
    assert ever and all(46 <= x < 52 and 26 <= y < 34 for x, y in ever)
