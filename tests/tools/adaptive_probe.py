"""The adaptive particle count measured, for a run under
`rocprofv3 --kernel-trace --stats -- python3 tests/tools/adaptive_probe.py MODE`:
  cal   the calibration scenario (tests/global_init_model.py) at capacity 100 000 from a uniform cloud, through convergence
  1m    a uniform cloud on 2000^2 at capacity 1 000 000, 60 moved updates: the map-wide search and then tracking
  fixed both at their capacity without adaptive mode (what the same updates cost the fixed filter)
  kidnap the kidnap scenario of tests/recovery_model.py at capacity 100 000 with adaptive mode and recovery (defaults) both on
Prints one line per update: the count it drew, its host wall time (updateFilter to a synchronised stream, ms), and the host time of
reading the last count back (bl_pf_adaptive_state before the update: the wait the update itself would otherwise make).
Per-kernel times come from rocprofv3's trace.  Load another build of the library with BOTLAB_HIP_LIB."""
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import global_init_model as gm  # noqa: E402
import helpers  # noqa: E402
import botlab_amd as bl  # noqa: E402
from botlab_amd import synth  # noqa: E402


def world(maps, size):
    w = synth.tile_world(maps["astar_maze"]["cells"], size)
    half = size * 0.05 / 2.0
    return np.where(w > 0, 100, -60).astype(np.int8), (np.float32(-half), np.float32(-half))


def run(ctx, cells, origin, n, poses, adaptive, label):
    g = bl.OccupancyGrid.from_cells(cells, origin, np.float32(0.05), cellsPerMeter=helpers.CPM_DEFAULT, ctx=ctx)
    truth = np.where(cells > 0, 127, -127).astype(np.int8)
    odo = synth.odometry_from_truth(poses, np.random.default_rng(3))
    scans = [synth.raycast_scan(truth, origin, 0.05, poses[max(k - 1, 0)], poses[k], 1000 + 100000 * k) for k in range(len(poses))]
    pf = bl.ParticleFilter(n, ctx=ctx)
    pf.setNoiseSeed(17)
    pf.initializeFilterUniformly(g, utime=1000, seed=gm.CAL_SEED)
    if adaptive:
        pf.setAdaptive()
    ctx.sync()
    for k in range(len(poses)):
        tw = time.perf_counter()
        active = pf.adaptiveState()["next"] if adaptive else n         # (resolves the last count: the wait pf_launch_main would make)
        wait_ms = 1e3 * (time.perf_counter() - tw)
        t0 = time.perf_counter()
        pose = pf.updateFilter(bl.make_pose(*odo[k], utime=scans[k].utime), scans[k], g, rand_value=1000 + k)
        ctx.sync()
        t1 = time.perf_counter()
        if k > 0:
            err = math.hypot(pose.x - poses[k][0], pose.y - poses[k][1])
            print(f"{label} update {k} drew {active} wall_ms {1e3 * (t1 - t0):.3f} count_wait_ms {wait_ms:.4f} err {err:.3f}", flush=True)
    pf.close()
    g.close()


def kidnap(ctx, maps):
    import recovery_model as rm
    m = maps[rm.KID_MAP]
    cells, origin = m["cells"], m["origin"]
    g = bl.OccupancyGrid.from_cells(cells, origin, np.float32(0.05), cellsPerMeter=helpers.CPM_DEFAULT, ctx=ctx)
    truthmap = np.where(cells > 0, 127, -127).astype(np.int8)
    motion, truth, begin = rm.kidnap_truth()
    odo = synth.odometry_from_truth(motion, np.random.default_rng(3))
    pf = bl.ParticleFilter(100_000, ctx=ctx)
    pf.setNoiseSeed(17)
    pf.initializeFilterAtPose(bl.make_pose(*rm.KID_START, utime=1000), seed=5)
    pf.setRecovery(g, seed=rm.KID_SEED)
    pf.setAdaptive()
    for k in range(len(truth)):
        scan = synth.raycast_scan(truthmap, origin, 0.05, begin[k] if k else truth[0], truth[k], 1000 + 100000 * k)
        pose = pf.updateFilter(bl.make_pose(*odo[k], utime=scan.utime), scan, g, rand_value=(1000 + 7919 * k) % rm.RAND_MAX)
        if k:
            st, rc = pf.adaptiveState(), pf.recoveryState()
            err = math.hypot(pose.x - truth[k][0], pose.y - truth[k][1])
            print(f"kidnap update {k} active {st['active']} p_inject {rc['p_inject']:.3f} err {err:.3f}", flush=True)
    pf.close()
    g.close()


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "cal"
    maps = helpers.load_reference_maps()
    ctx = bl.default_context()
    m = maps[gm.CAL_MAP]
    cal_poses = synth.square_trajectory(gm.CAL_START, gm.CAL_STEPS, **gm.CAL_TRAJ)
    c, o = world(maps, 2000)
    big_poses = synth.square_trajectory((0.3, 0.3, 0.0), 61, step_len=0.03, turn=0.05, side=0.8)
    if mode in ("cal", "fixed"):
        run(ctx, m["cells"], m["origin"], 100_000, cal_poses, mode == "cal", f"{mode}-100k")
    if mode in ("1m", "fixed"):
        run(ctx, c, o, 1_000_000, big_poses, mode == "1m", f"{mode}-1m")
    if mode == "kidnap":
        kidnap(ctx, maps)


if __name__ == "__main__":
    main()
