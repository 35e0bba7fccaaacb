"""The closed loop of the obstacle tracks: the 100 x 60 room and the local-planner parameters of the obstacle layer's loop
(tests/test_obstacle_layer_model_cpu.py), but the box that the map does not know now CROSSES the robot's straight route at a constant
speed.  Three ways: the map alone, the layer's composed grid, the tracks' composed grid with a horizon.  The CPU test runs the model;
tests/test_gpu_obstacle_tracks_loop.py runs the device beside it through step / on_tick."""
import math

import numpy as np

import local_plan_model as lpm
import obstacle_layer_model as om
import obstacle_tracks_model as tm
import test_obstacle_layer_model_cpu as lc
from test_local_plan_model_cpu import LOOP_PARAMS, cell_centre

F32 = np.float32
BOX_X, BOX_SIZE = 46, 6                # the box covers x 46 .. 51 and six rows
BOX_SPEED = 0.7                        # cells per tick, towards +y: chosen in the prototype so that with the plain layer
#                                        the robot's integration enters the box (at 0.6 and below the layer alone keeps it out)
BOX_Y0 = 27 - BOX_SPEED * 34           # its lowest row at tick 0: the box reaches the route when the robot does
LAYER = dict(occ_min=1, tol_cells=1, ttl_scans=3, min_hits=1, max_range=5.0)
TRACKS = dict(min_cells=3, max_cells=400, gate_cells=4, alpha=128, beta=64, confirm_hits=3, max_missed=3, min_speed=16)
# min_cells 3: the first sighting of the box is two fragments of 2 and 3 cells; a fragment of two cells is not taken for an object
HORIZON, KEEP_CLEAR = 10, 2            # the rollout looks 20 steps of 0.05 s ahead: ten ticks
TICKS = 400


def box_row(tick, speed=BOX_SPEED):
    return int(math.floor(BOX_Y0 + speed * tick))


def truth_at(cells, tick, speed=BOX_SPEED):
    t = cells.copy()
    y = box_row(tick, speed)
    t[max(y, 1):min(y + BOX_SIZE, lc.SCENE_H - 1), BOX_X:BOX_X + BOX_SIZE] = 100
    return t


def robot_cell(pose):
    return (int(math.floor((float(pose[0]) - float(lc.ORIGIN[0])) * float(lc.CPM))), int(math.floor((float(pose[1]) - float(lc.ORIGIN[1])) * float(lc.CPM))))


def box_whole(tick, speed=BOX_SPEED):
    """The whole box is inside the room (later it runs into the far wall and shrinks)."""
    return 1 <= box_row(tick, speed) and box_row(tick, speed) + BOX_SIZE <= lc.SCENE_H - 1


def run_loop(mode, step=None, on_tick=None, speed=BOX_SPEED, horizon=HORIZON, ticks=TICKS):
    """mode "map", "layer" or "tracks".  step(world, pose, v, w) -> RESULT record (default: the model's command);
    on_tick(tick, layer, tracker, scan, pose, composed, world) sees what a device copy must reproduce.  Returns a dict of the records,
    the integration steps inside the box, the ticks stood still (BLOCKED), per tick with blobs the ids of the tracks that hold one, the
    largest velocity error (cells per tick) of a confirmed matched track while the whole box is in the room, and the models."""
    cells, _ = lc.scene_cells()
    p = lpm.Params(**LOOP_PARAMS)
    static = lc.scene_world(cells)
    x, y = cell_centre(static, *lc.SCENE_START)
    pose = (x, y, F32(0.0))
    layer = om.Layer(lc.SCENE_W, lc.SCENE_H, **LAYER)
    tracker = tm.Tracker(lc.SCENE_W, lc.SCENE_H, **TRACKS)
    v, w = F32(0), F32(0)
    recs, inside, blocked, ids_per_tick, verr, world = [], 0, 0, [], 0.0, static
    for tick in range(ticks):
        truth = truth_at(cells, tick, speed)
        if mode != "map":
            scan = lc.scene_scan(truth, pose, tick)
            layer.update(cells, lc.ORIGIN, lc.CPM, scan.ranges, scan.thetas, pose)
            live = layer.live()
            if mode == "tracks":
                tracker.update(live, layer.n)
                composed = tracker.compose(live, layer.n, cells, horizon, robot_cell(pose), KEEP_CLEAR)
                if len(tracker.blobs):
                    ids_per_tick.append((tick, bool(np.any(tracker.slots["flags"] & tm.CONFIRMED)), sorted(int(tracker.slots["id"][b["track"]]) for b in tracker.blobs if b["track"] >= 0)))
                for t in tracker.tracks():
                    if t["flags"] & tm.CONFIRMED and t["flags"] & tm.MATCHED and box_whole(tick, speed):
                        verr = max(verr, math.hypot(int(t["vx"]) / 256.0, int(t["vy"]) / 256.0 - speed))
            else:
                composed = layer.compose(cells)
            world = lc.scene_world(composed)
            if on_tick:
                on_tick(tick, layer, tracker, scan, pose, composed, world)
        r = step(world, pose, v, w) if step else lpm.command(world, p, pose, v, w)[0]
        recs.append(r)
        if int(r["flags"]) == lpm.BLOCKED:               # no admissible command: stand still for this tick and look again
            blocked += 1
            v, w = F32(0), F32(0)
            continue
        if int(r["flags"]):
            break
        v, w = F32(r["trans_v"]), F32(r["angular_v"])
        for q in lpm.drive(pose, v, w, p):
            c = static.cell(q[0], q[1])
            inside += int(c is None or truth[c[1], c[0]] > 0)
            pose = q
    return dict(recs=recs, inside=inside, blocked=blocked, ids=ids_per_tick, verr=verr, layer=layer, tracker=tracker)
