"""Measures the view gain (bl_viewgain_*) and plan_path_to_frontier_by_gain on a GPU.  There is no earlier code path that computes a
gain, so the only figure beside the kernel's is the CPU model's time on (a sample of) the same candidates -- labelled as such.

  python tests/tools/view_gain_probe.py run <case> [out.json]   one case in this process: every near-frontier candidate of the map,
                                                                 10 warm-up calls of bl_viewgain_compute, then 100 timed ones (host wall
                                                                 time per call), 5 whole plan_path_to_frontier_by_gain calls, and the
                                                                 model on up to 50 of the candidates
  python tests/tools/view_gain_probe.py profile [outdir]        every case without the profiler, then under `rocprofv3 --kernel-trace
                                                                 --stats -- python ... run <case>` (the program after `--`, no counters);
                                                                 writes view_gain_per_call.csv and view_gain_kernel_stats.txt

Cases: <map>_r<R>, map one of slam200 (obstacle_slam, known within 30 cells of a free spot), disc2000 and disc4096 (the tiled maze,
known inside a disc of 0.35 x side cells), R one of 60, 100; K = 360."""
import glob
import json
import os
import sqlite3
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
CASES = [f"{m}_r{r}" for m in ("slam200", "disc2000", "disc4096") for r in (60, 100)]
WARM, REPS, K = 10, 100, 360


def _pcts(v):
    v = np.sort(np.asarray(v, float))
    return dict(median=float(np.median(v)), p10=float(np.percentile(v, 10)), p90=float(np.percentile(v, 90)), n=len(v))


def _world(name, maps, synth, vm):
    if name == "slam200":
        cells, spot = vm.partially_explored(maps["obstacle_slam_10mx10m_5cm"]["cells"])
        return cells, spot
    side = 2000 if name == "disc2000" else 4096
    world = synth.tile_world(maps["astar_maze"]["cells"], side)
    yy, xx = np.ogrid[:side, :side]
    cells = np.where((xx - side // 2) ** 2 + (yy - side // 2) ** 2 <= (0.35 * side) ** 2, world, 0).astype(np.int8)
    return cells, (side // 2, side // 2)


def run(case, out_path=None, extras=True):
    import botlab_amd as bl
    from botlab_amd import synth
    import helpers
    import nav_field_model as nm
    import view_gain_model as vm
    name, r = case.split("_r")
    r = int(r)
    cells, spot = _world(name, helpers.load_reference_maps(), synth, vm)
    h, w = cells.shape
    origin = (-w * 0.025, -h * 0.025)
    ctx = bl.default_context()
    g = bl.OccupancyGrid.from_cells(cells, origin, 0.05, cellsPerMeter=helpers.CPM_DEFAULT, ctx=ctx)
    cands = vm.near_frontier_candidates(cells, 3).astype(np.int32)
    vg = bl.ViewGain(r, K, ctx=ctx)
    res = dict(case=case, side=w, radius_cells=r, n_rays=K, candidates=len(cands))
    for _ in range(WARM):
        gain = vg.compute(g, cands)
    wall = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        gain = vg.compute(g, cands)
        wall.append((time.perf_counter() - t0) * 1e3)
    res["compute_ms"] = _pcts(wall)
    res.update(gain_min=int(gain.min()), gain_max=int(gain.max()), gain_sum=int(gain.sum()))
    if extras:
        # the whole planner from the traversable cell nearest the spot
        planner = bl.MotionPlanner(bl.MotionPlannerParams(0.1), ctx=ctx)
        planner.setMap(g)
        trav, _ = nm.tables(nm.dist_table(w, h), nm.Params(0.1, 1.0, 1.0))
        tcell, _ = nm.cell_tables(nm.l1_distances(cells), trav, np.zeros(len(trav), np.int32))
        ys, xs = np.nonzero(tcell)
        k = int(np.argmin((xs - spot[0]) ** 2 + (ys - spot[1]) ** 2))
        s = bl.make_pose(origin[0] + (xs[k] + 0.5) * 0.05, origin[1] + (ys[k] + 0.5) * 0.05, 0.0)
        frontiers = bl.find_map_frontiers(g, s)
        planner.setNumFrontiers(len(frontiers.cells()))
        wall = []
        for _ in range(5):
            t0 = time.perf_counter()
            path, fi, cell, pg, pc = bl.plan_path_to_frontier_by_gain(frontiers, s, g, planner, view=vg)
            wall.append((time.perf_counter() - t0) * 1e3)
        res["plan_ms"] = _pcts(wall)
        res.update(frontiers=len(frontiers.cells()), plan_frontier=fi, plan_cell=cell, plan_gain=pg, plan_cost=pc, plan_path=len(path))
        # the CPU model on a sample of the same candidates (not a yardstick of the kernel: a different machine part and language)
        pick = np.sort(np.random.default_rng(1).choice(len(cands), min(50, len(cands)), replace=False))
        ends = vg.rayEnds()
        t0 = time.perf_counter()
        want = vm.gains(cells, vm.Params(r, K), cands[pick], ends)
        res["cpu_model_ms_per_candidate"] = (time.perf_counter() - t0) * 1e3 / len(pick)
        res["sample_equal"] = bool(np.array_equal(want, gain[pick]))
    line = json.dumps(res)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


def profile(outdir):
    outdir = os.path.abspath(outdir)
    os.makedirs(outdir, exist_ok=True)
    me = os.path.abspath(__file__)
    rows, stats_txt = [], []
    for case in CASES:
        plain = os.path.join(outdir, f"vg_{case}.json")
        r = subprocess.run([sys.executable, me, "run", case, plain], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=280)
        if r.returncode != 0 or not os.path.exists(plain):
            stats_txt.append(f"## {case}: NOT RUN (exit {r.returncode})\n{r.stdout.decode(errors='replace')[-800:]}\n")
            print("[view_gain_probe]", case, "failed", r.returncode, flush=True)
            break                                      # nothing more on the GPU in this run
        j = json.load(open(plain))
        d = os.path.join(outdir, "prof_" + case)
        subprocess.run(["rm", "-rf", d])
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "p", "--", sys.executable, me, "run", case, "-", "noextras"]
        r = subprocess.run(cmd, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=280)
        dbs = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)
        dev_us = ""
        if r.returncode == 0 and dbs:
            con = sqlite3.connect(dbs[0])
            q = "select name, count(*), sum(end-start), avg(end-start), min(end-start), max(end-start) from kernels group by name order by 3 desc"
            stats_txt.append(f"## {case}: rocprofv3 --kernel-trace --stats -- python tests/tools/view_gain_probe.py run {case}   ({WARM} + {REPS} calls of {j['candidates']} candidates)\n"
                             "name, calls, total ns, average ns, min ns, max ns\n")
            for name, calls, tot, avg, lo, hi in con.execute(q):
                short = name.split("(")[0]
                stats_txt.append(f"{short}, {calls}, {tot}, {avg:.1f}, {lo}, {hi}\n")
                if short == "k_view_gain":
                    dev_us = "%.2f" % (avg / 1e3)
        else:
            stats_txt.append(f"## {case}: the profiled run failed (exit {r.returncode})\n{r.stdout.decode(errors='replace')[-800:]}\n")
            print("[view_gain_probe]", case, "profiled run failed", r.returncode, flush=True)
            if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
                break
        per_cand = "%.1f" % (float(dev_us) * 1e3 / j["candidates"]) if dev_us else ""
        rows.append([case, j["side"], j["radius_cells"], j["n_rays"], j["candidates"], j["gain_min"], j["gain_max"],
                     "%.3f" % j["compute_ms"]["median"], "%.3f" % j["compute_ms"]["p10"], "%.3f" % j["compute_ms"]["p90"], dev_us, per_cand,
                     "%.2f" % j["plan_ms"]["median"], j["frontiers"], j["plan_gain"], j["plan_cost"], j["plan_path"],
                     "%.3f" % j["cpu_model_ms_per_candidate"], j["sample_equal"]])
        print("[view_gain_probe]", case, "done", flush=True)
    with open(os.path.join(outdir, "view_gain_per_call.csv"), "w") as f:
        f.write("# host wall time of bl_viewgain_compute: median, p10, p90 over %d calls after %d warm-ups; k_view_gain_us: device time per launch from the profiled run;\n"
                "# plan_ms: plan_path_to_frontier_by_gain, median of 5; cpu_model: the numpy model on up to 50 of the candidates (not the same machine part)\n" % (REPS, WARM))
        f.write("case,side,radius_cells,n_rays,candidates,gain_min,gain_max,compute_ms_median,compute_ms_p10,compute_ms_p90,k_view_gain_us,device_ns_per_candidate,"
                "plan_ms_median,frontiers,plan_gain,plan_cost,plan_path_poses,cpu_model_ms_per_candidate,sample_equals_model\n")
        for row in rows:
            f.write(",".join(str(v).replace(",", ";") for v in row) + "\n")
        for c in CASES:
            if c not in [r[0] for r in rows]:
                f.write(f"# {c}: not run\n")
    with open(os.path.join(outdir, "view_gain_kernel_stats.txt"), "w") as f:
        f.writelines(stats_txt)
    return 0


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "run":
        run(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 and sys.argv[3] != "-" else None, extras="noextras" not in sys.argv[4:])
    elif len(sys.argv) >= 2 and sys.argv[1] == "profile":
        sys.exit(profile(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles")))
    else:
        print(__doc__)
        sys.exit(2)
