"""Times bl_mppi_plan on the 200 x 200 obstacle map: device time by the HIP events the library records around its
launches, warm, `reps` repetitions, median and 10th - 90th percentile, for K = 1024 and 4096 samples at T = 30 periods of n_sub = 4
steps (120 integration steps a sample), for 1 state and 64 states.  The yardstick, alternating with it within each repetition in the
same process, is bl_localplan_commands with a comparable number of rollout steps: n_v * n_w = K candidates of 120 steps.  Writes
mppi_timing.json.  For counters run the same script under the profiler's counter collection, in a run of its own.
    python tests/tools/mppi_measure.py <out dir> [reps]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import botlab_amd as bl  # noqa: E402
from botlab_amd import _capi  # noqa: E402
import helpers  # noqa: E402

T, N_SUB = 30, 4
SHAPES = ((1024, 8, 128), (4096, 16, 256))                   # K, and the yardstick's n_v x n_w = K


def main():
    out_dir = sys.argv[1]
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    os.makedirs(out_dir, exist_ok=True)
    m = helpers.load_reference_maps()["obstacle_slam_10mx10m_5cm"]
    ctx = bl.default_context()
    g = bl.OccupancyGrid.from_cells(m["cells"], m["origin"], m["mpc"], cellsPerMeter=helpers.CPM_DEFAULT, ctx=ctx)
    d = bl.ObstacleDistanceGrid(ctx=ctx)
    d.setDistances(g)
    nf = bl.NavigationField(ctx)
    nf.compute(d, _capi.NavFieldParams(0.2, 2.0, 1.0, 50, 2), [(98, 124)])
    field = nf.cells()
    ys, xs = np.nonzero((field != 0xFFFFFFFF) & (field != 0))
    rng = np.random.default_rng(2)
    pick = rng.choice(len(xs), 64, replace=False)
    lp_states, mp_states = [], []
    for i, k in enumerate(pick):
        x = float(m["origin"][0]) + (xs[k] + 0.5) * float(m["mpc"])
        y = float(m["origin"][1]) + (ys[k] + 0.5) * float(m["mpc"])
        pose, v, w = bl.make_pose(x, y, rng.uniform(-3, 3), utime=int(k)), np.float32(rng.uniform(0, 0.5)), np.float32(rng.uniform(-1, 1))
        lp_states.append((pose, v, w))
        mp_states.append((pose, v, w, 7, i))
    base = dict(v_min=0.0, v_max=0.5, w_max=2.5, acc_v=2.0, acc_w=12.0, dt_sim=0.05)
    report = dict(reps=reps, map="obstacle_slam_10mx10m_5cm", horizon=T, n_sub=N_SUB, steps=T * N_SUB)
    mp, lp = bl.MppiPlanner(ctx), bl.LocalPlanner(ctx)
    for K, n_v, n_w in SHAPES:
        mp.set_params(noise_v=0.25, noise_w=1.5, n_samples=K, horizon=T, n_sub=N_SUB, lam=64, w_field=16, w_heading=1, w_clear=1, seed=1, **base)
        lp.set_params(dt_control=0.1, n_v=n_v, n_w=n_w, n_steps=T * N_SUB, w_field=16, w_heading=1, w_clear=1, w_speed=8, **base)
        for n_states in (1, 64):
            sub_mp, sub_lp = mp_states[:n_states], lp_states[:n_states]
            seq = np.zeros((n_states, T, 2), np.int32)
            for _ in range(20):
                _, seq = mp.plan(nf, sub_mp, seq)
                lp.commands(nf, sub_lp)
            ms = dict(mppi=[], localplan=[])
            for _ in range(reps):
                res, seq = mp.plan(nf, sub_mp, seq)                          # warm-started from its own last sequence, as a loop would
                ms["mppi"].append(mp.lastDeviceMs())
                lres = lp.commands(nf, sub_lp)
                ms["localplan"].append(lp.lastDeviceMs())
            row = dict(mppi_admissible=int(res["n_admissible"].sum()), mppi_fell_back=int((res["flags"] == bl.MPPI_FELL_BACK).sum()),
                       localplan_admissible=int(lres["n_admissible"].sum()), mppi_window_path=mp.debugPath(), localplan_window_path=lp.debugPath())
            for k, v in ms.items():
                v = np.array(v)
                row[k] = dict(median_ms=float(np.median(v)), p10_ms=float(np.percentile(v, 10)), p90_ms=float(np.percentile(v, 90)))
            row["ratio_to_localplan"] = row["mppi"]["median_ms"] / row["localplan"]["median_ms"]
            print(K, n_states, row, flush=True)
            report["K_%d_states_%d" % (K, n_states)] = row
    with open(os.path.join(out_dir, "mppi_timing.json"), "w") as f:
        json.dump(report, f, indent=1)
    mp.close()
    lp.close()


if __name__ == "__main__":
    main()
