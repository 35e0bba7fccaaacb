"""Device time of ObstacleLayer.update and .compose (bl_obslayer_*, botlab_amd/csrc/bl_obslayer.hip) beside Mapping.updateMap of the
same scan on a copy of the same map, in the same process -- that kernel walks the same rays, so it is the yardstick.  Not a test.
The layer's times are the library's own HIP events around the launches (bl_obslayer_last_device_ms); the map update's is the context's
BL_K_MAP timer.  Warm (10 untimed repetitions of each), then 200 repetitions in which the three alternate; median and spread.

    python tests/tools/obslayer_measure.py [--reps 200] [--out profiles/obslayer_timing.json]

Sizes: the shipped 200 x 200 obstacle map with a 290-ray scan cut at 5 m, and that map's occupied cells tiled to 2000 x 2000 with a
290-ray scan cut at 8 m; in both a box the map does not know stands in front of the robot."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import botlab_amd as bl  # noqa: E402
from botlab_amd import synth  # noqa: E402
import helpers  # noqa: E402

BL_K_MAP = 2


def _stats(ms):
    a = np.sort(np.asarray(ms, dtype=np.float64))
    return dict(median_us=float(np.median(a)) * 1e3, min_us=float(a[0]) * 1e3, p10_us=float(a[len(a) // 10]) * 1e3,
                p90_us=float(a[(len(a) * 9) // 10]) * 1e3, max_us=float(a[-1]) * 1e3, n=int(len(a)))


def measure(ctx, name, cells, origin, pose, max_range, reps, warm=10):
    h, w = cells.shape
    truth = np.where(cells > 0, 127, -127).astype(np.int8)
    bx = int((pose[0] + 0.6 - origin[0]) / 0.05)
    by = int((pose[1] - origin[1]) / 0.05)
    truth[by - 3:by + 4, bx:bx + 6] = 127                              # the box
    scan = synth.raycast_scan(truth, origin, 0.05, pose, pose, 1000, max_range=max_range)
    g = bl.OccupancyGrid.from_cells(cells, origin, 0.05, cellsPerMeter=helpers.CPM_DEFAULT, ctx=ctx)
    gm = bl.OccupancyGrid.from_cells(cells, origin, 0.05, cellsPerMeter=helpers.CPM_DEFAULT, ctx=ctx)     # the map update's own copy
    layer = bl.ObstacleLayer(w, h, max_range=max_range, ctx=ctx)
    mapper = bl.Mapping(max_range, 4, 1, ctx=ctx)
    p = bl.make_pose(pose[0], pose[1], pose[2], utime=1000)
    out = None
    upd, com, mp = [], [], []
    ctx.timing_enable(True, kernels=[BL_K_MAP])
    for k in range(warm + reps):
        layer.update(g, scan, p)
        out = layer.compose(g, out)
        u, c = layer.lastDeviceMs()
        ctx.timing_reset()
        mapper.updateMap(scan, p, gm)
        ctx.sync()
        ms, n = ctx.timing_get(BL_K_MAP)
        assert n == 1
        if k >= warm:
            upd.append(u); com.append(c); mp.append(ms)
    ctx.timing_enable(False)
    st = layer.stats()
    for x in (layer, mapper, out, g, gm):
        x.close()
    a, b, c = _stats(upd), _stats(com), _stats(mp)
    return dict(map=name, shape=[w, h], rays=int(scan.num_ranges), max_range=float(max_range), valid_rays=st["valid"], rays_by_class=st["classes"],
                cleared_cells=st["clr"], hit_cells=st["hs"], update=a, compose=b, map_update=c,
                update_over_map_update=a["median_us"] / c["median_us"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "obslayer_timing.json"))
    args = ap.parse_args()
    ctx = bl.default_context()
    m = helpers.load_reference_maps()["obstacle_slam_10mx10m_5cm"]
    big = synth.tile_world(m["cells"], 2000)
    big = np.where(big > 0, 100, -100).astype(np.int8)
    rows = []
    for name, cells, origin, pose, rng in (("obstacle_slam_10mx10m_5cm", m["cells"], (float(m["origin"][0]), float(m["origin"][1])), (-0.75, 0.2, 0.3), 5.0),
                                           ("tiled_2000", big, (-50.0, -50.0), (-0.75 + 0.025, 0.2, 0.3), 8.0)):
        r = measure(ctx, name, cells, origin, pose, rng, args.reps)
        rows.append(r)
        print("%-28s update %7.1f us (p10 %.1f, p90 %.1f), compose %7.1f us (p10 %.1f, p90 %.1f), map update %7.1f us (p10 %.1f, p90 %.1f), "
              "update / map update %.2f" % (name, r["update"]["median_us"], r["update"]["p10_us"], r["update"]["p90_us"], r["compose"]["median_us"],
                                            r["compose"]["p10_us"], r["compose"]["p90_us"], r["map_update"]["median_us"], r["map_update"]["p10_us"],
                                            r["map_update"]["p90_us"], r["update_over_map_update"]), flush=True)
    with open(args.out, "w") as f:
        json.dump(dict(what="device time of bl_obslayer_update and bl_obslayer_compose (HIP events around the launches) and of bl_mapping_update "
                            "(BL_K_MAP timer) on the same scan and map in one process, warm, %d repetitions each, alternating" % args.reps,
                       rows=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
