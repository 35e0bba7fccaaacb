"""Device time of the beam model (bl_beam_*), one case per process so that a kernel trace of the process is a trace of the case:

    python tests/tools/beam_probe.py reweigh --grid 200 --particles 100000 [--staged] [--reps 20]
    python tests/tools/beam_probe.py scores  --grid 200 --poses 1000

reweigh: a filter seeded at a pose of the shipped map (tiled to --grid), one moved sensor update, then bl_beam_reweigh_pf `reps` times
on the same record (the units change, the poses do not: every repetition does the same casts).  scores: bl_beam_scores for poses
scattered over the map's free cells.  Prints one JSON line: the case, the path bl_beam_debug_path reports, the least and the median of
bl_beam_last_device_ms (HIP events round the three launches), and for reweigh the same of the whole call on the host clock (the
rescan, the finish and the pose's read-back included).  A measuring tool: it asserts nothing."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("case", choices=["reweigh", "scores"])
    ap.add_argument("--grid", type=int, default=200)
    ap.add_argument("--particles", type=int, default=100_000)
    ap.add_argument("--poses", type=int, default=1000)
    ap.add_argument("--staged", action="store_true", help="stage the workgroups' windows in LDS when they fit (default: the grid read through L2)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--max-range", type=float, default=5.0)
    a = ap.parse_args()
    ctx = bl.default_context()
    m = helpers.load_reference_maps()["obstacle_slam_10mx10m_5cm"]
    if a.grid == m["cells"].shape[0]:
        cells, truth = m["cells"], np.where(m["cells"] > 0, 127, -127).astype(np.int8)
    else:
        truth = synth.tile_world(m["cells"], a.grid)
        cells = truth
    origin = m["origin"]
    g = bl.OccupancyGrid.from_cells(cells, origin, m["mpc"], cellsPerMeter=helpers.CPM_DEFAULT, ctx=ctx)
    start = (-0.75, 0.2, 0.0)
    poses = synth.square_trajectory(start, 2, step_len=0.04, side=0.8)
    scans = [synth.raycast_scan(truth, origin, 0.05, poses[max(k - 1, 0)], poses[k], 1000 + 100000 * k) for k in range(3)]
    beam = bl.BeamModel(max_range=a.max_range, ctx=ctx)
    if a.staged:
        beam.debugSet(stage_windows=True)
    dev, host = [], []
    out = dict(case=a.case, grid=a.grid, rays=int(scans[2].num_ranges), max_range=a.max_range, staging=bool(a.staged))
    if a.case == "reweigh":
        pf = bl.ParticleFilter(a.particles, ctx=ctx)
        pf.initializeFilterAtPose(bl.make_pose(*poses[0], utime=scans[0].utime), seed=7)
        for k in range(3):
            pf.updateFilter(bl.make_pose(*poses[k], utime=scans[k].utime), scans[k], g, rand_value=12345 + k)
        for _ in range(a.reps + 3):
            ctx.sync()
            t0 = time.perf_counter()
            pf.reweigh_beam(beam, g, scans[2])
            host.append((time.perf_counter() - t0) * 1e3)
            dev.append(beam.lastDeviceMs())
        dev, host = dev[3:], host[3:]
        out.update(particles=a.particles, host_ms_min=min(host), host_ms_median=statistics.median(host))
    else:
        rng = np.random.default_rng(1)
        free = np.argwhere(cells < 0)
        pick = free[rng.integers(0, len(free), a.poses)]
        q = np.stack([origin[0] + (pick[:, 1] + 0.5) * 0.05, origin[1] + (pick[:, 0] + 0.5) * 0.05, rng.uniform(-3.1, 3.1, a.poses)], axis=1)
        for _ in range(a.reps + 3):
            beam.scores(g, scans[2], q.astype(np.float32))
            dev.append(beam.lastDeviceMs())
        dev = dev[3:]
        out.update(poses=a.poses)
    out.update(path=beam.debugPath(), device_ms_min=min(dev), device_ms_median=statistics.median(dev), reps=a.reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
