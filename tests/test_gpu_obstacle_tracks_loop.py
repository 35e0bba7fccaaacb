"""The closed loop of tests/obstacle_tracks_loop.py wholly on the device: every tick the obstacle layer's update, the tracks' update,
MotionPlanner.setMapWithTracks (the tracks' compose and the distance grid), NavigationField.compute and LocalPlanner's command.  The
tracks, the composed grid, the field, the commands and so the poses equal the model's tick by tick, from the start to the goal, and the
box keeps one id while it is seen."""
import numpy as np
import pytest

import botlab_amd as bl
from botlab_amd import _capi
import local_plan_model as lpm
import obstacle_tracks_loop as loop
import test_obstacle_layer_model_cpu as lc
from test_gpu_obstacle_tracks import same_records
from test_obstacle_tracks_loop_cpu import one_id_while_seen

pytestmark = pytest.mark.gpu
F32 = np.float32


def test_closed_loop_on_the_device_equals_the_model(gpu_ctx):
    cells, _ = lc.scene_cells()
    p = lpm.Params(**lc.LOOP_PARAMS)
    grid = bl.OccupancyGrid.from_cells(cells, lc.ORIGIN, lc.MPC, cellsPerMeter=lc.CPM, ctx=gpu_ctx)
    layer = bl.ObstacleLayer(lc.SCENE_W, lc.SCENE_H, ctx=gpu_ctx, **loop.LAYER)
    tracker = bl.ObstacleTracker(layer, **loop.TRACKS)
    planner = bl.MotionPlanner(ctx=gpu_ctx)
    nf = bl.NavigationField(gpu_ctx)
    lp = bl.LocalPlanner(gpu_ctx)
    lp.set_params(p.v_min, p.v_max, p.w_max, p.acc_v, p.acc_w, p.dt_control, p.dt_sim, p.n_v, p.n_w, p.n_steps, p.w_field, p.w_heading, p.w_clear,
                  p.w_speed)
    n = lc.SCENE_NAV
    navp = _capi.NavFieldParams(n["minDistanceToObstacle"], n["maxDistanceWithCost"], n["distanceCostExponent"], n["obstacle_gain"], lc.SCENE_REACH)
    seen = dict(ticks=0, stamped=0, deleted=0)
    try:
        def on_tick(tick, mlayer, mtracker, scan, pose, exp_composed, world):
            dpose = bl.make_pose(pose[0], pose[1], pose[2], utime=scan.utime)
            layer.update(grid, scan, dpose)
            tracker.update()
            planner.setMapWithTracks(grid, layer, tracker, loop.HORIZON, dpose, keep_clear=loop.KEEP_CLEAR)
            nf.compute(planner.distances_, navp, [lc.SCENE_GOAL])
            same_records(tracker.tracks(), mtracker.tracks(), (tick, "tracks"))
            assert tracker.stats() == mtracker.stats(), (tick, tracker.stats(), mtracker.stats())
            got = planner.composed_.cells()
            assert np.array_equal(got, exp_composed), tick
            assert np.array_equal(nf.cells(), world.field), tick
            seen["ticks"] += 1
            seen["deleted"] += mtracker.stats()["deleted"]
            seen["stamped"] += int(np.count_nonzero(exp_composed == 127) > np.count_nonzero(mlayer.compose(cells) == 127))

        def step(world, pose, v, w):
            exp, _ = lpm.command(world, p, pose, v, w)
            got = lp.commands(nf, [(bl.make_pose(pose[0], pose[1], pose[2], utime=99), F32(v), F32(w))])[0]
            for k in ("trans_v", "angular_v", "index", "n_admissible", "cost", "flags"):
                assert got[k].tobytes() == exp[k].tobytes(), (seen["ticks"], k, got, exp)
            return got

        r = loop.run_loop("tracks", step=step, on_tick=on_tick)
        same_records(tracker.blobs(), r["tracker"].blobs, "blobs at the end")
        assert np.array_equal(tracker.labels(), r["tracker"].labels)
    finally:
        for x in (lp, nf, tracker, layer, grid):
            x.close()
        if planner.composed_ is not None:
            planner.composed_.close()
        planner.distances_.close()
    kept = one_id_while_seen(r["ids"])
    print(f"on the device: flags {int(r['recs'][-1]['flags'])} at tick {len(r['recs']) - 1}, {seen['ticks']} ticks, {seen['stamped']} of them with cells stamped ahead of the box, {r['inside']} integration steps inside "
          f"the box, {r['blocked']} ticks stood still, the box keeps id {kept}, largest velocity error {r['verr']:.3f} cell per tick")
    assert int(r["recs"][-1]["flags"]) == lpm.REACHED and seen["ticks"] == len(r["recs"]) and seen["stamped"] > 0
    assert seen["deleted"] >= 1                                       # the ticks on which the last track coasts and goes are among them
