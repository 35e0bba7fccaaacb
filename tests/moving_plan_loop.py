"""The closed loop of the local planner's moving rule: the room, the parameters and the crossing box of tests/obstacle_tracks_loop.py
(DESIGN.md 4.24), but the field is computed over the static composition -- the layer's compose without the confirmed moving tracks'
cells -- and the commands come from command_moving, which meets the box where it will be at each step of the rollout.  The CPU test
runs the model; tests/test_gpu_moving_plan_loop.py runs the device beside it through step / on_tick."""
import functools

import numpy as np

import local_plan_model as lpm
import local_plan_moving_model as lmm
import obstacle_layer_model as om
import obstacle_tracks_loop as tl
import obstacle_tracks_model as tm
import test_obstacle_layer_model_cpu as lc
from test_local_plan_model_cpu import LOOP_PARAMS, cell_centre

F32 = np.float32
STEPS_PER_UPDATE = 2       # a tick (one scan, one tracker update) is dt_control = 0.1 s: two rollout steps of dt_sim = 0.05 s
LEAD_STEPS = 0             # the command is formed right after the tracker's update of the same tick, from that tick's scan
MARGIN_CELLS = 2           # the track's box is that of the cells the scan saw -- the side of the box facing the robot, often a
#                            fragment --, its velocity lags the truth by up to a quarter cell per tick, and the planner's clearance
#                            knows nothing of it (the static composition leaves it out): two cells, KEEP_CLEAR's figure in 4.24


def run_loop(speed=tl.BOX_SPEED, margin=MARGIN_CELLS, lead=LEAD_STEPS, step=None, on_tick=None, ticks=tl.TICKS, tracks=None):
    """step(world, slots, m, pose, v, w) -> (RESULT record, first_hit or None) (default: the model's command_moving);
    on_tick(tick, layer, tracker, scan, pose, composed, world) sees what a device copy must reproduce.  Returns the records, the
    integration steps inside the true box, the ticks stood still, per tick the number of candidates a moving box refused, and the
    side on which the robot crossed the box's column (the sign of robot row - box row when it passes x = BOX_X + BOX_SIZE / 2)."""
    cells, _ = lc.scene_cells()
    p = lpm.Params(**LOOP_PARAMS)
    m = lmm.Moving(STEPS_PER_UPDATE, margin, lead)
    static = lc.scene_world(cells)
    x, y = cell_centre(static, *lc.SCENE_START)
    pose = (x, y, F32(0.0))
    layer = om.Layer(lc.SCENE_W, lc.SCENE_H, **tl.LAYER)
    tracker = tm.Tracker(lc.SCENE_W, lc.SCENE_H, **(tracks or tl.TRACKS))
    v, w = F32(0), F32(0)
    recs, inside, blocked, refused, crossed = [], 0, 0, [], None
    for tick in range(ticks):
        truth = tl.truth_at(cells, tick, speed)
        scan = lc.scene_scan(truth, pose, tick)
        layer.update(cells, lc.ORIGIN, lc.CPM, scan.ranges, scan.thetas, pose)
        live = layer.live()
        tracker.update(live, layer.n)
        composed = lmm.compose_static(tracker, live, layer.n, cells)
        world = lc.scene_world(composed)
        if on_tick:
            on_tick(tick, layer, tracker, scan, pose, composed, world)
        if step:
            r, fh = step(world, tracker.slots, m, pose, v, w)
        else:
            r, _, fh = lmm.command_moving(world, p, tracker.slots, m, pose, v, w)
        recs.append(r)
        refused.append(0 if fh is None else int(np.count_nonzero(fh)))
        if int(r["flags"]) == lpm.BLOCKED:
            blocked += 1
            v, w = F32(0), F32(0)
            continue
        if int(r["flags"]):
            break
        v, w = F32(r["trans_v"]), F32(r["angular_v"])
        for q in lpm.drive(pose, v, w, p):
            c = static.cell(q[0], q[1])
            inside += int(c is None or truth[c[1], c[0]] > 0)
            if crossed is None and c is not None and c[0] >= tl.BOX_X + tl.BOX_SIZE // 2:
                by = tl.box_row(tick, speed)
                crossed = "behind" if c[1] < by else "in front" if c[1] >= by + tl.BOX_SIZE else "through"
            pose = q
    return dict(recs=recs, inside=inside, blocked=blocked, refused=refused, crossed=crossed, layer=layer, tracker=tracker)


@functools.lru_cache(maxsize=None)
def layer_run(speed=tl.BOX_SPEED):
    """run_loop("layer") of tests/obstacle_tracks_loop.py, once per process: the yardstick of the comparisons."""
    return tl.run_loop("layer", speed=speed)
