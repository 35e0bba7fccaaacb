"""Times bl_localplan_commands on the 200 x 200 obstacle map: device time by the HIP events the library records around
its launches, warm, `reps` repetitions, median and spread, for 1 state and 64 states at n_v = 32, n_w = 513, n_steps = 100; writes
the same inputs for tests/tools/localplan_cpu_ref (a single-thread restatement) and runs it when it has been built.
    python tests/tools/localplan_measure.py <out dir> [reps]
"""
import json
import os
import struct
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import botlab_amd as bl  # noqa: E402
from botlab_amd import _capi  # noqa: E402
import helpers  # noqa: E402
import nav_field_model as nm  # noqa: E402


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
    trav, pen = nf.tables()
    l1 = nm.l1_distances(m["cells"])
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
    report = dict(params=par, reps=reps, map="obstacle_slam_10mx10m_5cm", candidates=par["n_v"] * par["n_w"], steps_per_evaluation=par["n_v"] * par["n_w"] * par["n_steps"])
    results = {}
    for n in (1, 64):
        for _ in range(20):
            res = lp.commands(nf, states[:n])
        ms = []
        for _ in range(reps):
            res = lp.commands(nf, states[:n])
            ms.append(lp.lastDeviceMs())
        ms = np.array(ms)
        results[n] = res
        report[f"states_{n}"] = dict(median_ms=float(np.median(ms)), min_ms=float(ms.min()), p10_ms=float(np.percentile(ms, 10)),
                                     p90_ms=float(np.percentile(ms, 90)), max_ms=float(ms.max()),
                                     evaluations_per_second=float(n / (np.median(ms) * 1e-3)), path=lp.debugPath())
        print(n, report[f"states_{n}"], flush=True)
    # the dump for the CPU restatement
    dump = os.path.join(out_dir, "localplan_inputs.bin")
    table = np.where(trav != 0, pen, -1).astype(np.int32)
    with open(dump, "wb") as f:
        f.write(struct.pack("<11i5f", 200, 200, len(table), 64, par["n_v"], par["n_w"], par["n_steps"], par["w_field"], par["w_heading"], par["w_clear"],
                            par["w_speed"], float(m["mpc"]), float(cpm), float(m["origin"][0]), float(m["origin"][1]), par["dt_sim"]))
        f.write(field.astype(np.uint32).tobytes() + l1.astype(np.uint16).tobytes() + table.tobytes())
        for pose, v, w in states:
            f.write(struct.pack("<q4f2f", pose.utime, pose.x, pose.y, pose.theta, 0.0, float(v), float(w)))
        vts, wts = zip(*[lp.tables(s) for s in states])
        f.write(np.concatenate(vts).tobytes() + np.concatenate(wts).tobytes())
    report["device_winners"] = [int(r["index"]) for r in results[64]]
    exe = os.path.join(ROOT, "tests", "tools", "localplan_cpu_ref")
    if os.path.exists(exe):
        r = subprocess.run([exe, dump, "3"], stdout=subprocess.PIPE, timeout=600)
        text = r.stdout.decode()
        cpu_win = [int(line.split()[3]) for line in text.splitlines() if line.startswith("state ")]
        report["cpu_ref"] = text.splitlines()[-1]
        report["cpu_ref_winners_equal_device"] = cpu_win == report["device_winners"]
        print(report["cpu_ref"], report["cpu_ref_winners_equal_device"], flush=True)
    os.remove(dump)
    with open(os.path.join(out_dir, "localplan_timing.json"), "w") as f:
        json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
