"""Device time of LikelihoodField.compute (bl_lfield_compute, botlab_amd/csrc/bl_lfield.hip) beside the Euclidean distance grid's
transform of the same map -- the same two passes with a word store where the field has a byte store and a table look-up.  Not a
test.  Times are the library's own HIP events around the launches: bl_lfield_last_device_ms, and the context's BL_K_DIST timer around
ObstacleDistanceGrid(metric="euclidean").setDistances.  Warm (10 untimed repetitions), then the median and the spread of 200.

    python tests/tools/lfield_measure.py [--reps 200] [--out profiles/lfield_timing.json]

Maps: the shipped 200 x 200 obstacle map and a sparse 4096 x 4096 map (sources at 2e-4), at R = 6 and R = 64."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import botlab_amd as bl  # noqa: E402
import helpers  # noqa: E402

BL_K_DIST = 3


def _stats(ms):
    a = np.sort(np.asarray(ms, dtype=np.float64))
    return dict(median_us=float(np.median(a)) * 1e3, min_us=float(a[0]) * 1e3, p10_us=float(a[len(a) // 10]) * 1e3,
                p90_us=float(a[(len(a) * 9) // 10]) * 1e3, max_us=float(a[-1]) * 1e3, n=int(len(a)))


def measure(ctx, cells, R, reps, warm=10):
    g = bl.OccupancyGrid.from_cells(cells, (-5.0, -5.0), 0.05, cellsPerMeter=helpers.CPM_DEFAULT, ctx=ctx)
    lf = bl.LikelihoodField(sigma=0.1, max_cells=R, ctx=ctx)
    d = bl.ObstacleDistanceGrid(ctx=ctx, metric="euclidean", max_cells=R)
    field_ms, edt_ms = [], []
    for k in range(warm + reps):
        lf.compute(g)
        ms = lf.lastDeviceMs()
        if k >= warm:
            field_ms.append(ms)
    ctx.timing_enable(True, kernels=[BL_K_DIST])
    for k in range(warm + reps):
        ctx.timing_reset()
        d.setDistances(g)
        ctx.sync()
        ms, n = ctx.timing_get(BL_K_DIST)
        assert n == 1
        if k >= warm:
            edt_ms.append(ms)
    ctx.timing_enable(False)
    for x in (lf, d, g):
        x.close()
    f, e = _stats(field_ms), _stats(edt_ms)
    return dict(shape=[int(cells.shape[1]), int(cells.shape[0])], R=int(R), sources=int((cells >= 1).sum()), field=f, euclidean=e,
                ratio_of_medians=f["median_us"] / e["median_us"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lfield_timing.json"))
    args = ap.parse_args()
    ctx = bl.default_context()
    maps = helpers.load_reference_maps()
    rng = np.random.default_rng(11)
    sparse = np.where(rng.random((4096, 4096)) < 2e-4, 100, -50).astype(np.int8)
    rows = []
    for name, cells in (("obstacle_slam_10mx10m_5cm", maps["obstacle_slam_10mx10m_5cm"]["cells"]), ("sparse_4096", sparse)):
        for R in (6, 64):
            r = measure(ctx, cells, R, args.reps)
            r["map"] = name
            rows.append(r)
            print("%-28s R = %2d: field %8.1f us (p10 %.1f, p90 %.1f), euclidean grid %8.1f us (p10 %.1f, p90 %.1f), ratio %.3f"
                  % (name, R, r["field"]["median_us"], r["field"]["p10_us"], r["field"]["p90_us"], r["euclidean"]["median_us"],
                     r["euclidean"]["p10_us"], r["euclidean"]["p90_us"], r["ratio_of_medians"]), flush=True)
    with open(args.out, "w") as f:
        json.dump(dict(what="device time of bl_lfield_compute and of the Euclidean bl_dist_set_distances on the same maps, HIP events, "
                            "warm, %d repetitions each" % args.reps, rows=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
