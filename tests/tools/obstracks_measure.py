"""Device time of ObstacleTracker.update and .compose (bl_obstracks_*, botlab_amd/csrc/bl_obstracks.hip) beside ObstacleLayer.update and
.compose of the same scans on the same map, in the same process -- the layer's kernels are the yardstick.  Not a test.
All four times are the library's own HIP events around the launches (bl_obslayer_last_device_ms, bl_obstracks_last_device_ms).  Warm
(10 untimed repetitions), then 200 repetitions in which the four alternate; median and 10th / 90th percentile.  The tracker's update
holds the layer's three list launches; its compose holds the layer's whole compose.

    python tests/tools/obstracks_measure.py [--reps 200] [--out profiles/obstracks_timing.json]

Scenes: the shipped 200 x 200 obstacle map (290 rays cut at 5 m) and that map's occupied cells tiled to 2000 x 2000 (cut at 8 m), each
with one and with twenty 4 x 4 boxes that the map does not know, every box moving 0.3 cell per repetition, to and fro over 4 cells; and the worst case, live
cells at every even x and even y of a 131 x 67 grid (2244 blobs, 1024 kept, 256 tracks), reached through the layer's upload, for which
there is no scan and so no layer update to hold it against."""
import argparse
import ctypes as C
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import botlab_amd as bl  # noqa: E402
from botlab_amd import _capi, synth  # noqa: E402
import helpers  # noqa: E402

HORIZON = 10
PATH = 4                               # cells a box moves before it turns back: short, so that the 200 x 200 map has room for twenty


def _stats(ms):
    a = np.sort(np.asarray(ms, dtype=np.float64))
    return dict(median_us=float(np.median(a)) * 1e3, min_us=float(a[0]) * 1e3, p10_us=float(a[len(a) // 10]) * 1e3,
                p90_us=float(a[(len(a) * 9) // 10]) * 1e3, max_us=float(a[-1]) * 1e3, n=int(len(a)))


def box_places(cells, origin, pose, boxes, reach_cells):
    """Corners (cells) of `boxes` boxes on rings around the robot, where a 4 x 4 box and its path of PATH cells to the right are free."""
    h, w = cells.shape
    cx, cy = (pose[0] - origin[0]) / 0.05, (pose[1] - origin[1]) / 0.05
    out = []
    for ring in range(1, 160):
        r = 8.0 + 0.75 * ring
        if r > reach_cells:
            break
        for k in range(24):
            a = 2 * math.pi * (k + 0.37 * ring) / 24
            x, y = int(cx + r * math.cos(a)), int(cy + r * math.sin(a))
            if 3 <= y < h - 3 and 3 <= x < w - 12 and np.all(cells[y - 3:y + 4, x - 2:x + PATH + 6] < 0) and all(abs(y - q) > 4 or abs(x - p_) > PATH + 6 for p_, q in out):
                out.append((x, y))
                if len(out) == boxes:
                    return out
    return out


def measure(ctx, name, cells, origin, pose, max_range, boxes, reps, warm=10):
    h, w = cells.shape
    base = np.where(cells > 0, 127, -127).astype(np.int8)
    places = box_places(cells, origin, pose, boxes, max_range / 0.05 - 6)
    scans = []
    for k in range(warm + reps):
        truth = base.copy()
        for x, y in places:
            xx = x + int(math.floor(abs((0.3 * k) % (2.0 * PATH) - PATH)))   # to and fro over PATH cells
            truth[y - 2:y + 2, xx:xx + 4] = 127
        scans.append(synth.raycast_scan(truth, origin, 0.05, pose, pose, 1000 * (k + 1), max_range=max_range))
    g = bl.OccupancyGrid.from_cells(cells, origin, 0.05, cellsPerMeter=helpers.CPM_DEFAULT, ctx=ctx)
    layer = bl.ObstacleLayer(w, h, max_range=max_range, ttl_scans=3, ctx=ctx)
    tracker = bl.ObstacleTracker(layer, min_cells=2, max_cells=400)
    p = bl.make_pose(pose[0], pose[1], pose[2], utime=1000)
    rc = (int((pose[0] - origin[0]) / 0.05), int((pose[1] - origin[1]) / 0.05))
    out = out2 = None
    t = dict(layer_update=[], layer_compose=[], tracks_update=[], tracks_compose=[])
    for k in range(warm + reps):
        layer.update(g, scans[k], p)
        out = layer.compose(g, out)
        lu, lc = layer.lastDeviceMs()
        tracker.update()
        out2 = tracker.compose(g, out2, horizon=HORIZON, robot_cell=rc, keep_clear=2)
        tu, tc = tracker.lastDeviceMs()
        if k >= warm:
            t["layer_update"].append(lu); t["layer_compose"].append(lc); t["tracks_update"].append(tu); t["tracks_compose"].append(tc)
    st = tracker.stats()
    stamped = int(np.count_nonzero(out2.cells() == 127) - np.count_nonzero(out.cells() == 127))
    for x in (tracker, layer, out, out2, g):
        x.close()
    row = dict(scene=name, shape=[w, h], boxes=len(places), rays=int(scans[0].num_ranges), max_range=float(max_range), horizon=HORIZON,
               live_cells=st["live_cells"], blobs=st["blobs"], tracks=st["tracks"], confirmed=st["confirmed"], rounds=st["rounds"], stamped_cells=stamped)
    row.update({k: _stats(v) for k, v in t.items()})
    row["tracks_update_over_layer_update"] = row["tracks_update"]["median_us"] / row["layer_update"]["median_us"]
    row["tracks_compose_over_layer_compose"] = row["tracks_compose"]["median_us"] / row["layer_compose"]["median_us"]
    return row


def measure_pattern(ctx, reps, warm=10):
    w, h = 131, 67
    cells = np.full((h, w), -100, np.int8)
    m = np.zeros((h, w), bool)
    m[0::2, 0::2] = True
    g = bl.OccupancyGrid.from_cells(cells, (-1.0, -2.0), 0.05, cellsPerMeter=helpers.CPM_DEFAULT, ctx=ctx)
    layer = bl.ObstacleLayer(w, h, ctx=ctx)
    tracker = bl.ObstacleTracker(layer)
    out = out2 = None
    t = dict(layer_compose=[], tracks_update=[], tracks_compose=[])
    for k in range(warm + reps):
        layer.upload(m.astype(np.uint8), np.where(m, k + 1, 0).astype(np.uint32), k + 1)
        out = layer.compose(g, out)
        c = C.c_float()
        _capi.check(ctx.lib.bl_obslayer_last_device_ms(layer.h, None, C.byref(c)))     # (the layer has made no update: compose alone)
        lc = c.value
        tracker.update()
        out2 = tracker.compose(g, out2, horizon=HORIZON, robot_cell=(0, 0), keep_clear=-1)
        tu, tc = tracker.lastDeviceMs()
        if k >= warm:
            t["layer_compose"].append(lc); t["tracks_update"].append(tu); t["tracks_compose"].append(tc)
    st = tracker.stats()
    for x in (tracker, layer, out, out2, g):
        x.close()
    row = dict(scene="even cells of 131 x 67 (worst case: 2244 blobs)", shape=[w, h], boxes=0, rays=0, horizon=HORIZON, live_cells=st["live_cells"],
               blobs=st["blobs"], dropped=st["dropped"], tracks=st["tracks"], confirmed=st["confirmed"], rounds=st["rounds"], matched=st["matched"])
    row.update({k: _stats(v) for k, v in t.items()})
    row["tracks_compose_over_layer_compose"] = row["tracks_compose"]["median_us"] / row["layer_compose"]["median_us"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "obstracks_timing.json"))
    args = ap.parse_args()
    ctx = bl.default_context()
    m = helpers.load_reference_maps()["obstacle_slam_10mx10m_5cm"]
    big = synth.tile_world(m["cells"], 2000)
    big = np.where(big > 0, 100, -100).astype(np.int8)
    rows = []
    for name, cells, origin, pose, rng in (("obstacle_slam_10mx10m_5cm", m["cells"], (float(m["origin"][0]), float(m["origin"][1])), (-0.75, 0.2, 0.3), 5.0),
                                           ("tiled_2000", big, (-50.0, -50.0), (-0.75 + 0.025, 0.2, 0.3), 8.0)):
        for boxes in (1, 20):
            r = measure(ctx, name, cells, origin, pose, rng, boxes, args.reps)
            rows.append(r)
            print("%-28s %2d boxes (%4d live cells, %3d blobs, %3d tracks): layer update %7.1f us, tracks update %7.1f us (p10 %.1f, p90 %.1f), ratio %.2f; "
                  "layer compose %7.1f us, tracks compose %7.1f us (p10 %.1f, p90 %.1f), ratio %.2f"
                  % (name, r["boxes"], r["live_cells"], r["blobs"], r["tracks"], r["layer_update"]["median_us"], r["tracks_update"]["median_us"],
                     r["tracks_update"]["p10_us"], r["tracks_update"]["p90_us"], r["tracks_update_over_layer_update"], r["layer_compose"]["median_us"],
                     r["tracks_compose"]["median_us"], r["tracks_compose"]["p10_us"], r["tracks_compose"]["p90_us"],
                     r["tracks_compose_over_layer_compose"]), flush=True)
    r = measure_pattern(ctx, args.reps)
    rows.append(r)
    print("%s: %d live cells, %d blobs, %d tracks, %d rounds: tracks update %7.1f us (p10 %.1f, p90 %.1f); layer compose %7.1f us, tracks compose %7.1f us"
          % (r["scene"], r["live_cells"], r["blobs"], r["tracks"], r["rounds"], r["tracks_update"]["median_us"], r["tracks_update"]["p10_us"],
             r["tracks_update"]["p90_us"], r["layer_compose"]["median_us"], r["tracks_compose"]["median_us"]), flush=True)
    with open(args.out, "w") as f:
        json.dump(dict(what="device time of bl_obstracks_update and bl_obstracks_compose beside bl_obslayer_update and bl_obslayer_compose of the same "
                            "scans on the same map (HIP events around the launches), one process, warm, %d repetitions each, alternating; the tracks' "
                            "update holds the layer's three list launches, the tracks' compose the layer's whole compose" % args.reps,
                       rows=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
