"""Time of a map from `count` scans, two ways, in one process:

    python tests/tools/map_rebuild_probe.py [--out profiles/map_rebuild_times.json] [--reps 7]

  (a) `count` sequential bl_mapping_update calls on an empty grid (one single-workgroup launch per scan);
  (b) one bl_scanlog_rebuild of a log that holds the same scans and poses.

Shapes: the shipped 200 x 200 map at 5 cm, 290 rays, a drive-square trajectory, count in {64, 1024, 4096}; and the map tiled to
2000 x 2000 with count 1024.  Every shape is warmed up once, then repeated; per shape the tool reports the median and the least of the
host clock around the work and a stream synchronise, the device time -- for (a) the sum of the map kernels' HIP events (a repetition of
its own, since the events slow the host), for (b) the events round the rebuild's three phases (bl_scanlog_last_stats; the geometry
phase contains the one read-back) -- and whether the two maps are equal.  A measuring tool: it asserts nothing."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import botlab_amd as bl  # noqa: E402
from botlab_amd import synth  # noqa: E402
import helpers  # noqa: E402

BL_K_MAP = 2
MAX_LASER, HIT, MISS = 5.0, 4, 1


def measure(ctx, m, size, count, reps):
    if size == m["cells"].shape[0]:
        truth = np.where(m["cells"] > 0, 127, -127).astype(np.int8)
    else:
        truth = synth.tile_world(m["cells"], size)
    origin = m["origin"]
    poses = synth.square_trajectory((-0.75, 0.2, 0.0), count + 1, step_len=0.02, side=0.8)
    t0, dt = 1_000_000, 100_000
    scans = [synth.raycast_scan(truth, origin, 0.05, poses[0], poses[0], t0)] + synth.raycast_scans_gpu(truth, origin, 0.05, poses, t0, dt, ctx)
    scans, poses = scans[:count + 1], [bl.make_pose(p[0], p[1], p[2], utime=t0 + k * dt) for k, p in enumerate(poses[:count + 1])]
    zeros = np.zeros(truth.shape, np.int8)
    grid_a = bl.OccupancyGrid.from_cells(zeros, origin, m["mpc"], cellsPerMeter=helpers.CPM_DEFAULT, ctx=ctx)
    grid_b = bl.OccupancyGrid.from_cells(zeros, origin, m["mpc"], cellsPerMeter=helpers.CPM_DEFAULT, ctx=ctx)
    log = bl.ScanHistory(count + 1, 512, ctx=ctx)
    for s, p in zip(scans, poses):
        log.append(s, p)
    ctx.sync()

    def sequential():
        grid_a.reset()
        mapper = bl.Mapping(MAX_LASER, HIT, MISS, ctx=ctx)
        mapper.updateMap(scans[0], poses[0], grid_a)             # latches the pose
        ctx.sync()
        t = time.perf_counter()
        for s, p in zip(scans[1:], poses[1:]):
            mapper.updateMap(s, p, grid_a)
        ctx.sync()
        t = (time.perf_counter() - t) * 1e3
        mapper.close()
        return t

    def rebuild():
        ctx.sync()
        t = time.perf_counter()
        log.rebuild(grid_b, MAX_LASER, HIT, MISS)
        ctx.sync()
        return (time.perf_counter() - t) * 1e3

    sequential(); rebuild(); rebuild()                           # warm-up of both, this shape
    a_host, b_host, b_dev = [], [], []
    for _ in range(reps):                                        # alternating
        a_host.append(sequential())
        b_host.append(rebuild())
        st = log.stats()
        b_dev.append((st.ms_total, st.ms_geometry, st.ms_fold, st.ms_apply))
    ctx.timing_reset(); ctx.timing_enable(True, kernels=[BL_K_MAP])
    sequential()
    a_dev, launches = ctx.timing_get(BL_K_MAP)
    ctx.timing_enable(False)
    equal = bool(np.array_equal(grid_a.cells(), grid_b.cells()))
    st = log.stats()
    med = [statistics.median(v[i] for v in b_dev) for i in range(4)]
    out = dict(grid=size, rays=int(scans[1].num_ranges), count=count, reps=reps, maps_equal=equal,
               sequential_host_ms_median=statistics.median(a_host), sequential_host_ms_min=min(a_host),
               sequential_device_ms=a_dev, sequential_launches=int(launches) - 1,
               rebuild_host_ms_median=statistics.median(b_host), rebuild_host_ms_min=min(b_host),
               rebuild_device_ms_median=med[0], rebuild_geometry_ms_median=med[1], rebuild_fold_ms_median=med[2], rebuild_apply_ms_median=med[3],
               tiles=int(st.tiles), chunks=int(st.chunks), pairs=int(st.pairs), scratch_bytes=int(st.scratch_bytes), chunk_scans=int(st.chunk_scans),
               tile_cells=int(st.tile_cells))
    out["host_ratio"] = out["sequential_host_ms_median"] / out["rebuild_host_ms_median"]
    log.close(); grid_a.close(); grid_b.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="200:64,200:1024,200:4096,2000:1024")
    a = ap.parse_args()
    ctx = bl.default_context()
    m = helpers.load_reference_maps()["obstacle_slam_10mx10m_5cm"]
    results = []
    for shape in a.shapes.split(","):
        size, count = (int(v) for v in shape.split(":"))
        r = measure(ctx, m, size, count, a.reps)
        print(json.dumps(r), flush=True)
        results.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(tool="tests/tools/map_rebuild_probe.py", max_laser=MAX_LASER, hit=HIT, miss=MISS, results=results), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
