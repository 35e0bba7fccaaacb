"""Global localization costs on the GPU, for a run under `rocprofv3 --kernel-trace --stats -- python3 tests/tools/global_init_probe.py`:
bl_pf_init_uniform at 200^2 / 100 000, 2000^2 / 1 000 000 and 4096^2 / 1 000 000 particles (three calls each: the first allocates the
cell list), bl_pf_spread at 1 000 000, and the first five updates after a global init at 2000^2 / 1 000 000.  Prints host wall times
of the same calls (after one warm-up) as JSON."""
import json
import os
import sys
import time

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
    maps = helpers.load_reference_maps()
    ctx = bl.default_context()
    out = {}
    m = maps["obstacle_slam_10mx10m_5cm"]
    cases = [("200", m["cells"], m["origin"], 100_000)]
    for size in (2000, 4096):
        c, o = world(maps, size)
        cases.append((str(size), c, o, 1_000_000))
    for tag, cells, origin, n in cases:
        g = bl.OccupancyGrid.from_cells(cells, origin, np.float32(0.05), cellsPerMeter=helpers.CPM_DEFAULT, ctx=ctx)
        pf = bl.ParticleFilter(n, ctx=ctx)
        ts = []
        for k in range(3):
            ctx.sync()
            t0 = time.perf_counter()
            pf.initializeFilterUniformly(g, utime=1000, seed=k)
            ctx.sync()
            ts.append((time.perf_counter() - t0) * 1e3)
        out[f"init_{tag}_{n}_ms"] = ts
        if n == 1_000_000 and tag == "2000":
            ts = []
            for k in range(3):
                t0 = time.perf_counter()
                s = pf.spread()
                ts.append((time.perf_counter() - t0) * 1e3)
            out["spread_1000000_ms"] = ts
            truth = np.where(cells > 0, 127, -127).astype(np.int8)
            poses = synth.square_trajectory((0.3, 0.3, 0.0), 5, step_len=0.05, turn=0.1, side=0.2)
            pf.initializeFilterUniformly(g, utime=1000, seed=5)
            ts = []
            for k in range(1, 6):
                scan = synth.raycast_scan(truth, origin, 0.05, poses[k - 1], poses[k], 1000 + 100000 * k)
                ctx.sync()
                t0 = time.perf_counter()
                pf.updateFilter(bl.make_pose(*poses[k], utime=scan.utime), scan, g, rand_value=100 + k)
                ctx.sync()
                ts.append((time.perf_counter() - t0) * 1e3)
            out["first5_updates_2000_1000000_ms"] = ts
            out["spread_after_5"] = {k: v for k, v in pf.spread().items()}
        pf.close()
        g.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
