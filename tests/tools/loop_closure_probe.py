"""Measurement (recorded, not asserted): botlab_amd.find_loop_closures, one candidate after the other from Python, against
botlab_amd.LoopCloser.find, every candidate in one sequence of launches, on the same history in the same process.

Two histories of the world of tests/test_gpu_loop_closure.py: its 160 scans (two laps), and 1024 scans (the same circle, more laps),
both at stride 4.  Warmed up, then 7 alternating repetitions; the host clock round each call, lastDeviceMs and its split from events
for the new one.  Medians.  Writes a JSON file (default profiles/loop_closure_times.json).

    python tests/tools/loop_closure_probe.py [output.json]"""
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

import botlab_amd as bl                       # noqa: E402
from botlab_amd import synth                  # noqa: E402
import test_gpu_loop_closure as lc            # noqa: E402

REPS = 7
PARAMS = dict(stride=4, min_gap=40, radius=0.5, w=5, submap_cells=200, nx=8, ny=8, ntheta=12, dtheta=lc.DTHETA, max_range=8.0, half_life=64,
              maxLaserDistance=lc.MAX_LASER, hitOdds=lc.HIT, missOdds=lc.MISS)


def _history(ctx, n):
    world = lc._world()
    t = np.arange(n) / lc.LAP * 2 * math.pi
    truth = np.stack([lc.RADIUS * np.cos(t), lc.RADIUS * np.sin(t), np.arctan2(np.sin(t + math.pi / 2), np.cos(t + math.pi / 2))], 1)
    rec = truth.copy()
    drift = lc.BIAS * (np.arange(n) % (2 * lc.LAP))             # the recorded heading drifts for two laps, then starts again
    rec[:, 2] = np.arctan2(np.sin(truth[:, 2] + drift), np.cos(truth[:, 2] + drift))
    history = bl.ScanHistory(n, synth.RAYS, ctx=ctx)
    lap = {}
    for k in range(n):
        if k % lc.LAP not in lap:
            lap[k % lc.LAP] = synth.raycast_scan(world, lc.ORIGIN, lc.MPC, truth[k], truth[k], 0)
        s, ut = lap[k % lc.LAP], 100000 * (k + 1)
        history.append(bl.LidarScan(s.ranges, s.thetas, np.full(s.num_ranges, ut, np.int64), utime=ut), bl.make_pose(rec[k, 0], rec[k, 1], rec[k, 2], utime=ut))
    return history


def _measure(ctx, n):
    history = _history(ctx, n)
    like = bl.OccupancyGrid(lc.SIZE * lc.MPC, lc.SIZE * lc.MPC, lc.MPC, ctx=ctx)
    matcher, closer = bl.ScanMatcher(ctx=ctx), bl.LoopCloser(1024, ctx=ctx)
    try:
        for _ in range(2):
            old = bl.find_loop_closures(history, matcher, like, **PARAMS)
            new = closer.find(history, like, **PARAMS)
        assert list(zip(old["i"].tolist(), old["j"].tolist())) == list(zip(new["i"].tolist(), new["j"].tolist()))
        t_old, t_new, dev, split = [], [], [], []
        for _ in range(REPS):
            ctx.sync()
            t0 = time.perf_counter()
            bl.find_loop_closures(history, matcher, like, **PARAMS)
            t1 = time.perf_counter()
            closer.find(history, like, **PARAMS)
            t2 = time.perf_counter()
            t_old.append((t1 - t0) * 1e3)
            t_new.append((t2 - t1) * 1e3)
            ms, ms4 = closer.lastDeviceMs(split=True)
            dev.append(ms)
            split.append(ms4)
        med = statistics.median
        return dict(scans=n, candidates=len(closer.candidates()), kept=len(new), repetitions=REPS,
                    find_loop_closures_host_ms=med(t_old), loop_closer_host_ms=med(t_new), loop_closer_device_ms=med(dev),
                    device_ms_pairs=med(s[0] for s in split), device_ms_rays_fold=med(s[1] for s in split),
                    device_ms_match=med(s[2] for s in split), device_ms_records=med(s[3] for s in split),
                    host_ratio=med(t_old) / med(t_new), all_find_loop_closures_host_ms=t_old, all_loop_closer_host_ms=t_new)
    finally:
        closer.close(); matcher.close(); like.close(); history.close()


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "loop_closure_times.json")
    ctx = bl.default_context()
    rows = [_measure(ctx, 160), _measure(ctx, 1024)]
    for r in rows:
        print(json.dumps({k: v for k, v in r.items() if not k.startswith("all_")}))
    with open(out, "w") as f:
        json.dump(dict(params={k: (float(v) if isinstance(v, float) else v) for k, v in PARAMS.items()}, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
