"""bl_pf_clusters on the GPU, for a run under `rocprofv3 --kernel-trace --stats -- python3 tests/tools/pf_cluster_probe.py`: a converged
cloud (bl_pf_init_at_pose: a handful of bins) and a uniform one (bl_pf_init_uniform over the 200^2 map at 100 000 particles, over a
2000^2 world at 1 000 000: as many bins as the map allows) at both sizes, bins of 0.5 m and 10 degrees, 8 clusters.  Prints host wall
times of the call in milliseconds (five calls after one warm-up that allocates; the call synchronises), without and with labels,
the number of clusters, and bl_pf_spread's time beside them, as JSON."""
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


def timed(f, reps=5):
    f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append(round((time.perf_counter() - t0) * 1e3, 4))
    return ts


def main():
    maps = helpers.load_reference_maps()
    ctx = bl.default_context()
    m = maps["obstacle_slam_10mx10m_5cm"]
    w = synth.tile_world(maps["astar_maze"]["cells"], 2000)
    big = (np.where(w > 0, 100, -60).astype(np.int8), (np.float32(-50.0), np.float32(-50.0)))
    out = {}
    for n, (cells, origin) in ((100_000, (m["cells"], m["origin"])), (1_000_000, big)):
        g = bl.OccupancyGrid.from_cells(cells, origin, np.float32(0.05), cellsPerMeter=helpers.CPM_DEFAULT, ctx=ctx)
        pf = bl.ParticleFilter(n, ctx=ctx)
        for cloud in ("converged", "uniform"):
            if cloud == "converged":
                pf.initializeFilterAtPose(bl.make_pose(0.3, 0.3, 0.0, utime=1000), seed=5)
            else:
                pf.initializeFilterUniformly(g, utime=1000, seed=5)
            ctx.sync()
            tag = f"{cloud}_{n}"
            out[tag + "_ms"] = timed(lambda: pf.clusters(0.5, 36, 8))
            out[tag + "_labels_ms"] = timed(lambda: pf.clusters(0.5, 36, 8, labels=True))
            r = pf.clusters(0.5, 36, 8)
            out[tag + "_clusters"] = r["num_clusters"]
            out[tag + "_heaviest_count"] = r["clusters"][0]["count"]
            out[tag + "_spread_ms"] = timed(pf.spread)
        pf.close()
        g.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
