"""Device time of path shortcutting (bl_shortcut_cells), from the library's own HIP events: warm, 200 repetitions, median and spread,
for all kernels of a call and for k_sc_visible alone (the rest is k_sc_dp).  Cases: one model field path on the 200 x 200 obstacle
map, 300 short paths in one call, the 8192-cell serpentine at max_span 64.  Writes shortcut_timing.json (argv[1], or the current
directory).  Needs a GPU; bench.py calls nothing of this."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import botlab_amd as bl  # noqa: E402
import helpers  # noqa: E402
import path_shortcut_model as psm  # noqa: E402
import test_path_shortcut_model_cpu as cpu  # noqa: E402

REPS = 200


def measure(sc, dist, paths, params):
    sc.set_params(*params)
    for _ in range(5):
        sc.cells(dist, paths)
    tot, vis = [], []
    for _ in range(REPS):
        sc.cells(dist, paths)
        a, b = sc.lastDeviceMs()
        tot.append(a)
        vis.append(b)
    q = lambda v, p: float(np.percentile(v, p))  # noqa: E731
    return dict(paths=len(paths), cells=int(sum(len(p) for p in paths)), clearance=params[0], max_span=params[1], waypoint_cost=params[2], reps=REPS,
                path=sc.debugPath(), total_ms=dict(median=q(tot, 50), p10=q(tot, 10), p90=q(tot, 90), min=min(tot), max=max(tot)),
                visible_ms=dict(median=q(vis, 50), p10=q(vis, 10), p90=q(vis, 90)), dp_ms_median=q(np.array(tot) - np.array(vis), 50))


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else "."
    ctx = bl.default_context()
    sc = bl.PathShortcut(ctx)
    res = {}

    def dist_of(world):
        g = bl.OccupancyGrid.from_cells(world.cells, world.origin, world.mpc, cellsPerMeter=helpers.CPM_DEFAULT, ctx=ctx)
        d = bl.ObstacleDistanceGrid(ctx=ctx)
        d.setDistances(g)
        return d, g

    world, poses = cpu.map_case(helpers.load_reference_maps())
    d, g = dist_of(world)
    q = psm.pose_cells(poses, world.origin, helpers.CPM_DEFAULT, world.w, world.h)
    res["field_path_200x200"] = measure(sc, d, [q], (0.2, 64, 1024))
    rng = np.random.default_rng(1)
    res["300_paths"] = measure(sc, d, [cpu.walk(rng, world.w, world.h, int(n), start=(100, 120)) for n in rng.integers(20, 120, 300)], (0.2, 64, 1024))
    room = cpu.room_world()
    d2, g2 = dist_of(room)
    res["serpentine_8192"] = measure(sc, d2, [cpu.serpentine(room.w, room.h, 8192)], (0.2, 64, 1024))
    sc.close()
    with open(os.path.join(out_dir, "shortcut_timing.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
