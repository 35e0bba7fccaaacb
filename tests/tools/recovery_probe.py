"""k_mcl_main with and without kidnapped-robot recovery, for a run under
`rocprofv3 --kernel-trace --stats -- python3 tests/tools/recovery_probe.py MODE`: 40 moved tracking updates at 200^2 / 100 000 and at
2000^2 / 1 000 000 particles.  MODE: off (no recovery; the only mode a library without bl_pf_set_recovery runs), p0 (recovery on,
ratio 1e-9: p stays 0), p25 (ratio 1e9, max_fraction 0.25: a quarter injected once the tracker is primed).  Load another build of
the library with BOTLAB_HIP_LIB."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import helpers  # noqa: E402
import botlab_amd as bl  # noqa: E402
from botlab_amd import synth  # noqa: E402


def world(maps, size):
    w = synth.tile_world(maps["astar_maze"]["cells"], size)
    half = size * 0.05 / 2.0
    return np.where(w > 0, 100, -60).astype(np.int8), (np.float32(-half), np.float32(-half))


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "off"
    maps = helpers.load_reference_maps()
    ctx = bl.default_context()
    m = maps["obstacle_slam_10mx10m_5cm"]
    cases = [(m["cells"], m["origin"], 100_000, (-0.75, 0.2, 0.0))]
    c, o = world(maps, 2000)
    cases.append((c, o, 1_000_000, (0.3, 0.3, 0.0)))
    for cells, origin, n, start in cases:
        g = bl.OccupancyGrid.from_cells(cells, origin, np.float32(0.05), cellsPerMeter=helpers.CPM_DEFAULT, ctx=ctx)
        truth = np.where(cells > 0, 127, -127).astype(np.int8)
        poses = synth.square_trajectory(start, 41, step_len=0.02, turn=0.05, side=0.2)
        odo = synth.odometry_from_truth(poses, np.random.default_rng(3))
        scans = [synth.raycast_scan(truth, origin, 0.05, poses[max(k - 1, 0)], poses[k], 1000 + 100000 * k) for k in range(len(poses))]
        pf = bl.ParticleFilter(n, ctx=ctx)
        pf.setNoiseSeed(17)
        pf.initializeFilterAtPose(bl.make_pose(*start, utime=1000), seed=5)
        if mode != "off":
            pf.setRecovery(g, ratio=1e-9 if mode == "p0" else 1e9, maxFraction=0.25, seed=9)
        for k in range(len(poses)):
            pf.updateFilter(bl.make_pose(*odo[k], utime=scans[k].utime), scans[k], g, rand_value=1000 + k, want_pose=False)
        ctx.sync()
        if mode != "off":
            st = pf.recoveryState()
            print(n, mode, "p", st["p_inject"], "injected", st["injected_total"])
        pf.close()
        g.close()


if __name__ == "__main__":
    main()
