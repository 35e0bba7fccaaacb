"""Device time of the clearance grid (bl_clearance_*) and of the beam model scored by leaps over it, one case per process so that a
kernel trace of the process is a trace of the case:

    python tests/tools/clearance_probe.py grid    --grid 200 --cap 64 [--reps 20]
    python tests/tools/clearance_probe.py reweigh --grid 200 --particles 100000 --cap 64

grid: the shipped map (tiled to --grid), bl_clearance_build `reps` times and bl_clearance_update of the driver's box `reps` times -- the
bounding box of the cells of two consecutive poses of the drive widened by ceil(max_range * cells_per_meter) + 2 -- with the device
time of each (HIP events round the two launches).  reweigh: beam_probe.py's filter and scan; bl_beam_reweigh_pf (the cast) and
bl_clearance_reweigh_pf alternated `reps` times on the same record in one process: device time and whole-call time on the host clock
of each form, the mean rounds per ray of the filter's pose, and whether the two forms left the same units.  Prints one JSON line:
least, median and spread (largest less least) of every series.  A measuring tool: it asserts nothing."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import botlab_amd as bl  # noqa: E402
import helpers  # noqa: E402
from range_table_probe import series, world  # noqa: E402


def driver_box(m, poses, max_range, cpm, size):
    """The box OccupancyGridSLAMT would hand to update() after a map update between poses[1] and poses[2], before clipping."""
    cx = [int((p[0] - float(m["origin"][0])) * cpm) for p in poses[1:3]]
    cy = [int((p[1] - float(m["origin"][1])) * cpm) for p in poses[1:3]]
    pad = int(math.ceil(max_range * cpm)) + 2
    return min(cx) - pad, min(cy) - pad, max(cx) + pad, max(cy) + pad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("case", choices=["grid", "reweigh"])
    ap.add_argument("--grid", type=int, default=200)
    ap.add_argument("--cap", type=int, default=64)
    ap.add_argument("--particles", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--max-range", type=float, default=5.0)
    a = ap.parse_args()
    ctx = bl.default_context()
    out = dict(case=a.case, grid=a.grid, cap=a.cap, reps=a.reps)
    m, cells, g, poses, scans = world(ctx, a.grid)
    beam = bl.BeamModel(max_range=a.max_range, ctx=ctx)
    cl = bl.ClearanceGrid(ctx, a.cap)
    out.update(max_range=a.max_range, rays=int(scans[2].num_ranges))
    box = driver_box(m, poses, a.max_range, float(helpers.CPM_DEFAULT), a.grid)
    if a.case == "grid":
        build, upd = [], []
        for _ in range(a.reps + 3):
            cl.build(g, 1)
            build.append(cl.lastDeviceMs())
        for _ in range(a.reps + 3):
            cl.update(g, *box)
            upd.append(cl.lastDeviceMs())
        out.update(bytes=cl.info()["bytes"], box=list(box), **series("build_ms", build[3:]), **series("update_ms", upd[3:]))
    else:
        cl.build(g, 1)
        pf = bl.ParticleFilter(a.particles, ctx=ctx)
        pf.initializeFilterAtPose(bl.make_pose(*poses[0], utime=scans[0].utime), seed=7)
        for k in range(3):
            pf.updateFilter(bl.make_pose(*poses[k], utime=scans[k].utime), scans[k], g, rand_value=12345 + k)
        dev, host, units = {"cast": [], "leap": []}, {"cast": [], "leap": []}, {}
        for _ in range(a.reps + 3):
            for form in ("cast", "leap"):
                ctx.sync()
                t0 = time.perf_counter()
                if form == "cast":
                    pf.reweigh_beam(beam, g, scans[2])
                else:
                    pf.reweigh_beam_leap(beam, cl, scans[2])
                host[form].append((time.perf_counter() - t0) * 1e3)
                dev[form].append(beam.lastDeviceMs())
                units[form] = beam.units(a.particles)
        for form in ("cast", "leap"):
            out.update(**series(form + "_device_ms", dev[form][3:]), **series(form + "_host_ms", host[form][3:]))
        est = pf.poseEstimate()
        d = beam.debug_leap(cl, scans[2], (est.x, est.y, est.theta))
        on = d["rounds"] >= 0
        upd = []
        for _ in range(a.reps + 3):
            cl.update(g, *box)
            upd.append(cl.lastDeviceMs())
        out.update(particles=a.particles, same_units=bool(np.array_equal(units["cast"], units["leap"])),
                   rounds_per_ray=float(d["rounds"][on].mean()), cells_per_ray_loop=float(np.minimum(d["first"][on] + 1, d["K"][on]).mean()),
                   **series("update_ms", upd[3:]))
        cast, leap = out["cast_device_ms_median"], out["leap_device_ms_median"] + out["update_ms_median"]
        out.update(leap_plus_update_ms=leap, margin_ms=cast - leap,
                   spreads_ms=out["cast_device_ms_spread"] + out["leap_device_ms_spread"] + out["update_ms_spread"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
