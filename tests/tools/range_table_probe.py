"""Device time of the range table (bl_rangetable_*) and of the beam model scored through it, one case per process so that a kernel
trace of the process is a trace of the case:

    python tests/tools/range_table_probe.py build   --grid 200 --headings 256 [--box 40] [--reps 20]
    python tests/tools/range_table_probe.py reweigh --grid 200 --particles 100000 --headings 256
    python tests/tools/range_table_probe.py agree   --grid 200 --poses 1000 --headings 256
    python tests/tools/range_table_probe.py agree   --conditions --headings 256

build: the shipped map (tiled to --grid), bl_rangetable_build `reps` times and bl_rangetable_update of a --box x --box box in the middle
`reps` times; the device time of each (HIP events round the launch) and the table's bytes.  reweigh: beam_probe.py's filter and scan;
bl_beam_reweigh_pf (the cast) and bl_rangetable_reweigh_pf alternated `reps` times on the same record in one process: device time and
whole-call time on the host clock of each form, the build time, and the number of reweighs at which the build is paid back.  agree: the
share of rays whose expected range by table lies within 4 quarter cells of the exact cast's (both without an expected hit counts as
agreeing), over poses scattered on the map's free cells or over beam_cases.conditions(64, 48).  Prints one JSON line: least, median and
spread (largest less least) of every series.  A measuring tool: it asserts nothing."""
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


def series(name, v):
    return {name + "_min": min(v), name + "_median": statistics.median(v), name + "_spread": max(v) - min(v)}


def world(ctx, grid):
    m = helpers.load_reference_maps()["obstacle_slam_10mx10m_5cm"]
    if grid == m["cells"].shape[0]:
        cells, truth = m["cells"], np.where(m["cells"] > 0, 127, -127).astype(np.int8)
    else:
        truth = synth.tile_world(m["cells"], grid)
        cells = truth
    g = bl.OccupancyGrid.from_cells(cells, m["origin"], m["mpc"], cellsPerMeter=helpers.CPM_DEFAULT, ctx=ctx)
    poses = synth.square_trajectory((-0.75, 0.2, 0.0), 2, step_len=0.04, side=0.8)
    scans = [synth.raycast_scan(truth, m["origin"], 0.05, poses[max(k - 1, 0)], poses[k], 1000 + 100000 * k) for k in range(3)]
    return m, cells, g, poses, scans


def agreement(beam, rt, g, scan, poses):
    within = total = 0
    worst = 0
    for q in poses:
        c, t = beam.debug_cast(g, scan, q), beam.debug_lookup(rt, scan, q)
        on = (c["p"] > 0) & (t["p"] > 0)
        both, none = on & (c["zstar"] >= 0) & (t["zstar"] >= 0), on & (c["zstar"] < 0) & (t["zstar"] < 0)
        d = np.abs(c["zstar"] - t["zstar"])[both]
        within += int((d <= 4).sum()) + int(none.sum())
        total += int(on.sum())
        worst = max(worst, int(d.max(initial=0)))
    return dict(rays=total, within_4=within, share=within / max(total, 1), largest_difference_both_hit=worst)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("case", choices=["build", "reweigh", "agree"])
    ap.add_argument("--grid", type=int, default=200)
    ap.add_argument("--headings", type=int, default=256)
    ap.add_argument("--particles", type=int, default=100_000)
    ap.add_argument("--poses", type=int, default=1000)
    ap.add_argument("--box", type=int, default=40)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--max-range", type=float, default=5.0)
    ap.add_argument("--conditions", action="store_true", help="agree: beam_cases.conditions(64, 48) in place of the map")
    a = ap.parse_args()
    ctx = bl.default_context()
    out = dict(case=a.case, grid=a.grid, headings=a.headings, reps=a.reps)
    if a.case == "agree" and a.conditions:
        import beam_cases as bc
        from test_gpu_beam import KEYS
        c = bc.conditions(64, 48)
        g = bl.OccupancyGrid.from_cells(c["cells"], c["origin"], c["mpc"], cellsPerMeter=c["cpm"], ctx=ctx)
        beam = bl.BeamModel(ctx=ctx, **{k: c["params"][k] for k in KEYS})
        rt = bl.RangeTable(ctx, a.headings)
        rt.build(beam, g)
        scan = bl.LidarScan(c["ranges"], c["thetas"], np.zeros(len(c["ranges"]), np.int64))
        out.update(grid="conditions(64, 48)", max_range=c["params"]["max_range"], **agreement(beam, rt, g, scan, c["poses"]))
        print(json.dumps(out))
        return
    m, cells, g, poses, scans = world(ctx, a.grid)
    beam = bl.BeamModel(max_range=a.max_range, ctx=ctx)
    rt = bl.RangeTable(ctx, a.headings)
    out.update(max_range=a.max_range, rays=int(scans[2].num_ranges))
    if a.case == "build":
        build, upd = [], []
        for _ in range(a.reps + 3):
            rt.build(beam, g)
            build.append(rt.lastDeviceMs())
        x0, y0 = a.grid // 2 - a.box // 2, a.grid // 2 - a.box // 2
        for _ in range(a.reps + 3):
            rt.update(g, x0, y0, x0 + a.box - 1, y0 + a.box - 1)
            upd.append(rt.lastDeviceMs())
        i = rt.info()
        out.update(bytes=i["bytes"], reach=i["reach"], box=a.box, **series("build_ms", build[3:]), **series("update_ms", upd[3:]))
    elif a.case == "reweigh":
        rt.build(beam, g)
        rt.build(beam, g)
        build_ms = rt.lastDeviceMs()
        pf = bl.ParticleFilter(a.particles, ctx=ctx)
        pf.initializeFilterAtPose(bl.make_pose(*poses[0], utime=scans[0].utime), seed=7)
        for k in range(3):
            pf.updateFilter(bl.make_pose(*poses[k], utime=scans[k].utime), scans[k], g, rand_value=12345 + k)
        dev, host = {"cast": [], "table": []}, {"cast": [], "table": []}
        for _ in range(a.reps + 3):
            for form in ("cast", "table"):
                ctx.sync()
                t0 = time.perf_counter()
                if form == "cast":
                    pf.reweigh_beam(beam, g, scans[2])
                else:
                    pf.reweigh_beam_table(beam, rt, scans[2])
                host[form].append((time.perf_counter() - t0) * 1e3)
                dev[form].append(beam.lastDeviceMs())
        for form in ("cast", "table"):
            out.update(**series(form + "_device_ms", dev[form][3:]), **series(form + "_host_ms", host[form][3:]))
        saved = out["cast_device_ms_median"] - out["table_device_ms_median"]
        out.update(particles=a.particles, build_ms=build_ms, bytes=rt.info()["bytes"],
                   reweighs_to_amortise=(build_ms / saved if saved > 0 else None))
    else:
        rt.build(beam, g)
        rng = np.random.default_rng(1)
        free = np.argwhere(cells < 0)
        pick = free[rng.integers(0, len(free), a.poses)]
        q = np.stack([m["origin"][0] + (pick[:, 1] + 0.5) * 0.05, m["origin"][1] + (pick[:, 0] + 0.5) * 0.05, rng.uniform(-3.1, 3.1, a.poses)], axis=1)
        out.update(poses=a.poses, **agreement(beam, rt, g, scans[2], q.astype(np.float32)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
