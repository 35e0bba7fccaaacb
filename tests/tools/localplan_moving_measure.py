"""Times bl_localplan_commands_moving against bl_localplan_commands on the 200 x 200 obstacle map: device time by the
HIP events the library records around its launches, warm, the variants alternating within each repetition in one process, `reps`
repetitions, median and 10th - 90th percentile, for 1 state and 64 states at n_v = 32, n_w = 513, n_steps = 100.  The yardstick is the
plain call on the same states in the same run; the moving call runs with 0, 1, 12, 13, 16 and 256 used slots placed around the first
state's cell, inside its reach (at 100 steps 12 boxes fit the table of BL_LOCALPLAN_MOVING_BYTES and 13 do not).  Writes
localplan_moving_timing.json.
    python tests/tools/localplan_moving_measure.py <out dir> [reps]
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
import local_plan_moving_model as lmm  # noqa: E402

SLOTS = (0, 1, 12, 13, 16, 256)
Q, MARGIN, LEAD = 2, 1, 0


def main():
    out_dir = sys.argv[1]
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    os.makedirs(out_dir, exist_ok=True)
    m = helpers.load_reference_maps()["obstacle_slam_10mx10m_5cm"]
    cpm = helpers.CPM_DEFAULT
    ctx = bl.default_context()
    g = bl.OccupancyGrid.from_cells(m["cells"], m["origin"], m["mpc"], cellsPerMeter=cpm, ctx=ctx)
    d = bl.ObstacleDistanceGrid(ctx=ctx)
    d.setDistances(g)
    nf = bl.NavigationField(ctx)
    nf.compute(d, _capi.NavFieldParams(0.2, 2.0, 1.0, 50, 2), [(98, 124)])
    field = nf.cells()
    par = dict(v_min=0.0, v_max=0.5, w_max=2.5, acc_v=2.0, acc_w=12.0, dt_control=0.1, dt_sim=0.05, n_v=32, n_w=513, n_steps=100,
               w_field=16, w_heading=1, w_clear=1, w_speed=8)
    lp = bl.LocalPlanner(ctx, **par)
    ys, xs = np.nonzero((field != 0xFFFFFFFF) & (field != 0))
    rng = np.random.default_rng(2)
    pick = rng.choice(len(xs), 64, replace=False)
    states = []
    for k in pick:
        x = float(m["origin"][0]) + (xs[k] + 0.5) * float(m["mpc"])
        y = float(m["origin"][1]) + (ys[k] + 0.5) * float(m["mpc"])
        states.append((bl.make_pose(x, y, rng.uniform(-3, 3), utime=int(k)), np.float32(rng.uniform(0, 0.5)), np.float32(rng.uniform(-1, 1))))
    cx, cy = int(xs[pick[0]]), int(ys[pick[0]])
    h, w = field.shape
    trackers, layers = {}, []
    for n in SLOTS:
        recs = []
        for i in range(n):                                  # 2 x 2 boxes on a 16 x 16 lattice around the first state's cell, drifting slowly
            x0, y0 = cx - 24 + 3 * (i % 16), cy - 24 + 3 * (i // 16)
            recs.append(lmm.make_slot(i + 1, x0, y0, x0 + 1, y0 + 1, int(rng.integers(-40, 41)), int(rng.integers(-40, 41))))
        layer = bl.ObstacleLayer(w, h, ctx=ctx)
        t = bl.ObstacleTracker(layer)
        t.upload(lmm.slot_table(recs), 0, n + 1, 1)
        trackers[n] = t
        layers.append(layer)
    report = dict(params=par, reps=reps, map="obstacle_slam_10mx10m_5cm", candidates=par["n_v"] * par["n_w"], moving=dict(steps_per_update=Q, margin_cells=MARGIN, lead_steps=LEAD),
                  moving_bytes=lmm.MOVING_BYTES, first_state_cell=[cx, cy])
    for n_states in (1, 64):
        sub = states[:n_states]
        for _ in range(20):
            lp.commands(nf, sub)
            for n in SLOTS:
                lp.commands_moving(nf, trackers[n], sub, Q, MARGIN, LEAD)
        ms = {k: [] for k in ("plain",) + SLOTS}
        paths, adm = {}, {}
        for _ in range(reps):
            res = lp.commands(nf, sub)
            ms["plain"].append(lp.lastDeviceMs())
            adm["plain"] = int(res["n_admissible"].sum())
            for n in SLOTS:
                res = lp.commands_moving(nf, trackers[n], sub, Q, MARGIN, LEAD)
                ms[n].append(lp.lastDeviceMs())
                paths[n] = lp.debugMovingPath()
                adm[n] = int(res["n_admissible"].sum())
        base = float(np.median(ms["plain"]))
        rows = {}
        for k, v in ms.items():
            v = np.array(v)
            rows[str(k)] = dict(median_ms=float(np.median(v)), p10_ms=float(np.percentile(v, 10)), p90_ms=float(np.percentile(v, 90)),
                                ratio_to_plain=float(np.median(v)) / base, admissible=adm[k], moving_path_of_first_state=paths.get(k), window_path=lp.debugPath())
            print(n_states, k, rows[str(k)], flush=True)
        report[f"states_{n_states}"] = rows
    with open(os.path.join(out_dir, "localplan_moving_timing.json"), "w") as f:
        json.dump(report, f, indent=1)
    lp.close()
    for t in trackers.values():
        t.close()
    for layer in layers:
        layer.close()


if __name__ == "__main__":
    main()
