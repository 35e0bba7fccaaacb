"""Measures the navigation field (bl_navfield_*) on a GPU, beside the search and the frontier planner it does not replace.

  python tests/tools/nav_field_probe.py run <case> [out.json]   one case in this process: 10 warm-up computes, then 100 timed ones
                                                                 (host wall time per compute, rounds, tile sweeps), 100 path queries,
                                                                 and the yardstick on the same inputs (bl_astar_search for the same
                                                                 start and goal, or bl_plan_path_to_frontier for the frontier case)
  python tests/tools/nav_field_probe.py profile [outdir [plain]] every case under `rocprofv3 --kernel-trace --stats -- python ... run <case>`
                                                                 (the program after `--`, no counters in that run) and once without the
                                                                 profiler; writes nav_field_per_compute.csv and nav_field_kernel_stats.txt

Cases: slam200 (obstacle_slam, the smoke query), maze2000 (the tiled maze), maze4096, frontier4096 (an explored disc of the 4096 x 4096
maze: every frontier cell a goal)."""
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
CASES = ["slam200", "maze2000", "maze4096", "frontier4096"]
WARM, REPS = 10, 100


def _pcts(v):
    v = np.sort(np.asarray(v, float))
    return dict(median=float(np.median(v)), p10=float(np.percentile(v, 10)), p90=float(np.percentile(v, 90)), n=len(v))


def _world(case, maps, synth):
    if case == "slam200":
        m = maps["obstacle_slam_10mx10m_5cm"]
        return m["cells"], (float(m["origin"][0]), float(m["origin"][1])), 0.2
    side = 2000 if case == "maze2000" else 4096
    world = synth.tile_world(maps["astar_maze"]["cells"], side)
    if case == "frontier4096":                       # explored disc around the middle, unknown (0) outside
        yy, xx = np.ogrid[:side, :side]
        world = np.where((xx - side // 2) ** 2 + (yy - side // 2) ** 2 <= 1500 ** 2, world, 0).astype(np.int8)
    return world, (-side * 0.025, -side * 0.025), 0.1


def run(case, out_path=None, yardstick=True):
    import botlab_amd as bl
    from botlab_amd import synth
    import helpers
    import nav_field_model as nm
    maps = helpers.load_reference_maps()
    cells, origin, radius = _world(case, maps, synth)
    h, w = cells.shape
    ctx = bl.default_context()
    g = bl.OccupancyGrid.from_cells(cells, origin, 0.05, cellsPerMeter=helpers.CPM_DEFAULT, ctx=ctx)
    planner = bl.MotionPlanner(bl.MotionPlannerParams(radius), ctx=ctx)
    planner.setMap(g)
    sp = planner.searchParams_
    l1 = nm.l1_distances(cells)
    trav, _ = nm.tables(nm.dist_table(w, h), nm.Params(sp.minDistanceToObstacle, sp.maxDistanceWithCost, sp.distanceCostExponent))
    tcell, _ = nm.cell_tables(l1, trav, np.zeros(len(trav), np.int32))
    ys, xs = np.nonzero(tcell)

    def pose_of(x, y):
        return bl.make_pose(origin[0] + (x + 0.5) * 0.05, origin[1] + (y + 0.5) * 0.05, 0.0)
    res = dict(case=case, width=w, height=h, traversable=int(tcell.sum()))
    nf = bl.NavigationField(ctx)
    if case == "slam200":
        start, goal = bl.make_pose(-0.75, 0.2, 0.0), bl.make_pose(-0.35, 0.2, 0.0)
    elif case == "frontier4096":
        c = int(np.argmin((xs - w // 2) ** 2 + (ys - h // 2) ** 2))          # the traversable cell nearest the middle
        start, goal = pose_of(xs[c], ys[c]), None
    else:
        start, goal = pose_of(xs[0], ys[0]), pose_of(xs[-1], ys[-1])
    if goal is not None:
        params = bl.nav_params(sp)

        def compute():
            nf.computeToPose(planner.distances_, params, goal)
    else:
        frontiers = bl.find_map_frontiers(g, start)
        fr = frontiers.cells()
        planner.setNumFrontiers(len(fr))
        reach = bl.host.nav_min_traversable_cells(planner.distances_, sp)
        mpc, cpm, ox, oy = planner.distances_.frame()
        goals = np.array([(int((float(x) - float(ox)) * float(cpm)), int((float(y) - float(oy)) * float(cpm))) for f in fr for x, y in f], np.int32).reshape(-1, 2)
        params = bl.nav_params(sp, reach_cells=reach)
        res.update(frontiers=len(fr), frontier_cells=len(goals), reach_cells=reach)

        def compute():
            nf.compute(planner.distances_, params, goals)
    for _ in range(WARM):
        compute()
    wall = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        compute()
        wall.append((time.perf_counter() - t0) * 1e3)
    res["compute_ms"] = _pcts(wall)
    res["stats"] = nf.stats()
    wall = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        paths, labels, costs = nf.paths([start], cap_each=1 << 16)
        wall.append((time.perf_counter() - t0) * 1e3)
    res["path_ms"] = _pcts(wall)
    res.update(path_length=len(paths[0]), path_cost=int(costs[0]))
    # the yardstick: the parent's code paths on the same inputs (5 calls; 1 if a call takes longer than 10 s)
    wall = []
    try:
        for _ in range(5 if yardstick else 0):
            t0 = time.perf_counter()
            if goal is not None:
                p, st = bl.search_for_path(start, goal, planner.distances_, sp, return_stats=True)
            else:
                p, _, st = bl.plan_path_to_frontier(frontiers, start, g, planner, return_info=True)
            wall.append((time.perf_counter() - t0) * 1e3)
            if wall[-1] > 10e3:
                break
        if not wall:
            pass
        elif goal is not None:
            res.update(astar_ms=_pcts(wall), astar_path_length=len(p), astar_pops=int(st[0]))
        else:
            res.update(plan_path_to_frontier_ms=_pcts(wall), plan_path_to_frontier_length=len(p), plan_path_to_frontier_pops=int(st[0]),
                       plan_path_to_frontier_searches=int(st[2]))
    except bl.BotlabHipError as e:
        res["yardstick_error"] = str(e)[:200]
    line = json.dumps(res)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


def profile(outdir, plain_dir=None):
    """plain_dir: results of earlier un-profiled runs (nav_<case>.json) to take instead of running the cases again."""
    outdir = os.path.abspath(outdir)
    os.makedirs(outdir, exist_ok=True)
    me = os.path.abspath(__file__)
    rows, stats_txt, not_run = [], [], []
    for case in CASES:
        plain = os.path.join(outdir, f"nav_{case}.json")
        if plain_dir and os.path.exists(os.path.join(plain_dir, f"nav_{case}.json")):
            plain = os.path.join(plain_dir, f"nav_{case}.json")
            r = subprocess.CompletedProcess([], 0, b"")
        else:
            r = subprocess.run([sys.executable, me, "run", case, plain], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        if r.returncode != 0 or not os.path.exists(plain):
            not_run.append(case)
            stats_txt.append(f"## {case}: NOT RUN (exit {r.returncode})\n{r.stdout.decode(errors='replace')[-800:]}\n")
            print("[nav_field_probe]", case, "failed", r.returncode, flush=True)
            if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
                break                                  # a fault or a hang: nothing more on the GPU in this run
            continue
        j = json.load(open(plain))
        d = os.path.join(outdir, "prof_" + case)
        subprocess.run(["rm", "-rf", d])
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "p", "--", sys.executable, me, "run", case, "-", "noyardstick"]
        r = subprocess.run(cmd, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=280)
        dbs = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)
        kern = {}
        if r.returncode == 0 and dbs:
            con = sqlite3.connect(dbs[0])
            q = "select name, count(*), sum(end-start), avg(end-start), min(end-start), max(end-start) from kernels group by name order by 3 desc"
            stats_txt.append(f"## {case}: rocprofv3 --kernel-trace --stats -- python tests/tools/nav_field_probe.py run {case}   ({WARM} + {REPS} computes, {REPS} path queries, no yardstick calls)\n"
                             "name, calls, total ns, average ns, min ns, max ns\n")
            for name, calls, tot, avg, lo, hi in con.execute(q):
                short = name.split("(")[0]
                stats_txt.append(f"{short}, {calls}, {tot}, {avg:.1f}, {lo}, {hi}\n")
                kern[short] = (calls, tot)
        else:
            stats_txt.append(f"## {case}: the profiled run failed (exit {r.returncode})\n")
            print("[nav_field_probe]", case, "profiled run failed", r.returncode, flush=True)
        computes = WARM + REPS

        def per_compute(k):
            return "%.1f" % (kern[k][1] / computes / 1e3) if k in kern else ""
        y = j.get("astar_ms") or j.get("plan_path_to_frontier_ms") or dict(median=float("nan"), p10=float("nan"), p90=float("nan"))
        rows.append([case, j["width"], j["traversable"], j.get("frontier_cells", 1), j["stats"]["rounds"], j["stats"]["tile_sweeps"], j["stats"]["reached"],
                     "%.3f" % j["compute_ms"]["median"], "%.3f" % j["compute_ms"]["p10"], "%.3f" % j["compute_ms"]["p90"],
                     per_compute("k_nav_init"), per_compute("k_nav_goals"), per_compute("k_nav_relax"), per_compute("k_nav_count_reached"),
                     "%.3f" % j["path_ms"]["median"], j["path_length"], j["path_cost"],
                     "bl_astar_search" if "astar_ms" in j else "bl_plan_path_to_frontier", "%.3f" % y["median"], "%.3f" % y["p10"], "%.3f" % y["p90"],
                     j.get("astar_path_length", j.get("plan_path_to_frontier_length")), j.get("astar_pops", j.get("plan_path_to_frontier_pops"))])
        print("[nav_field_probe]", case, "done", flush=True)
    with open(os.path.join(outdir, "nav_field_per_compute.csv"), "w") as f:
        f.write("# host wall time per compute: median, p10, p90 over %d computes after %d warm-ups; kernel columns: device us per compute from the profiled run\n" % (REPS, WARM))
        f.write("case,side,traversable_cells,goal_cells,rounds,tile_sweeps,reached_cells,compute_ms_median,compute_ms_p10,compute_ms_p90,"
                "k_nav_init_us,k_nav_goals_us,k_nav_relax_us,k_nav_count_reached_us,path_ms_median,path_poses,path_cost,"
                "yardstick,yardstick_ms_median,yardstick_ms_p10,yardstick_ms_p90,yardstick_path_poses,yardstick_pops\n")
        for row in rows:
            f.write(",".join(str(v) for v in row) + "\n")
        for c in CASES:
            if c not in [r[0] for r in rows]:
                f.write(f"# {c}: not run\n")
    with open(os.path.join(outdir, "nav_field_kernel_stats.txt"), "w") as f:
        f.writelines(stats_txt)
    return 0


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "run":
        run(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 and sys.argv[3] != "-" else None, yardstick="noyardstick" not in sys.argv[4:])
    elif len(sys.argv) >= 2 and sys.argv[1] == "profile":
        sys.exit(profile(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles"), sys.argv[3] if len(sys.argv) > 3 else None))
    else:
        print(__doc__)
        sys.exit(2)
