"""Measures the Rao-Blackwellized grid SLAM (bl_rbslam_*) on a GPU.

  python tests/tools/rb_slam_probe.py run <case> [out.json]   one case in this process: 5 warm-up updates, then 40 timed ones along the square
                                                               trajectory (host wall time per update, 1 / 1 schedule, device noise); beside it
                                                               the existing single-map step at the same particle count (bl_pf_update +
                                                               bl_mapping_update) and, unless "noextras" follows, the CPU model on 2 updates
  python tests/tools/rb_slam_probe.py profile [outdir]        every case without the profiler, then under `rocprofv3 --kernel-trace --stats --
                                                               python ... run <case>` (the program after `--`, no counters); every GPU step
                                                               is a child process under its own `timeout -k 10`, and the first failure ends
                                                               the run; writes rb_slam_per_update.csv and rb_slam_kernel_stats.csv

Cases: p<P>_s<side>: P particles, side x side cells at 5 cm (p64_s200, p256_s200, p1024_s200, p64_s1000)."""
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
CASES = ["p64_s200", "p256_s200", "p1024_s200", "p64_s1000"]
WARM, REPS = 5, 40
MAX_LASER, HIT, MISS = 5.0, 3, 1
STEP_TIMEOUT = 280


def _med(v):
    return float(np.median(np.asarray(v, float)))


def run(case, out_path=None, extras=True):
    import botlab_amd as bl
    from botlab_amd import synth
    import helpers
    P, side = (int(s[1:]) for s in case.split("_"))
    m = helpers.load_reference_maps()["obstacle_slam_10mx10m_5cm"]
    truth = np.where(m["cells"] > 0, 127, -127).astype(np.int8)
    cpm = helpers.CPM_DEFAULT
    origin = (np.float32(-side * 0.025), np.float32(-side * 0.025))
    poses = synth.square_trajectory((-0.75, 0.2, 0.0), WARM + REPS, step_len=0.04, turn=0.1, side=0.8)
    scans = [synth.raycast_scan(truth, m["origin"], 0.05, poses[max(k - 1, 0)], poses[k], 1000 + 100000 * k) for k in range(len(poses))]
    odo = [bl.make_pose(p[0], p[1], p[2], utime=1000 + 100000 * k) for k, p in enumerate(poses)]
    ctx = bl.default_context()
    rb = bl.RBSlam(P, side, side, 0.05, cpm, origin, MAX_LASER, HIT, MISS, ctx=ctx)
    rb.setResampling(1, 1)
    rb.setNoiseSeed(3)
    rb.initializeAtPose(odo[0], seed=5)
    wall, resampled = [], 0
    for k in range(len(poses)):
        t0 = time.perf_counter()
        r = rb.update(odo[k], scans[k], rand_value=17 + k)
        if k > WARM:
            wall.append((time.perf_counter() - t0) * 1e3)
            resampled += r["resampled"]
    res = dict(case=case, particles=P, side=side, rays=scans[0].num_ranges, updates=len(wall), resampled=resampled, update_ms=_med(wall),
               map_nonzero=int(np.count_nonzero(rb.best_map().cells())))
    # the existing single-map step at the same particle count: one shared grid, the map updated at the filter's mean
    g = bl.OccupancyGrid.from_cells(np.zeros((side, side), np.int8), origin, 0.05, cellsPerMeter=cpm, ctx=ctx)
    pf = bl.ParticleFilter(max(P, 2), ctx=ctx)
    pf.setNoiseSeed(3)
    pf.initializeFilterAtPose(odo[0], seed=5)
    mapper = bl.Mapping(MAX_LASER, HIT, MISS, ctx=ctx)
    wall = []
    for k in range(len(poses)):
        t0 = time.perf_counter()
        pose = pf.updateFilter(odo[k], scans[k], g, rand_value=17 + k)
        mapper.updateMap(scans[k], pose, g)
        ctx.sync()
        if k > WARM:
            wall.append((time.perf_counter() - t0) * 1e3)
    res["single_map_step_ms"] = _med(wall)
    if extras:
        import oracle_lib
        import rb_slam_model as rbm
        mdl = rbm.RBSlamModel(oracle_lib.load_oracle(), P, (side, side), 0.05, cpm, origin, MAX_LASER, HIT, MISS, 1, 1)
        mdl.init_at_pose(poses[0][0], poses[0][1], poses[0][2], 1000)
        rng = np.random.default_rng(0)
        t = []
        for k in range(4):
            o = (poses[k][0], poses[k][1], poses[k][2], 1000 + 100000 * k)
            nz = mdl.draw_noise(o, rng)
            t0 = time.perf_counter()
            mdl.update(o, scans[k], 17 + k, nz)
            t.append((time.perf_counter() - t0) * 1e3)
        res["cpu_model_update_ms"] = _med(t[2:])
    line = json.dumps(res)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


def profile(outdir):
    outdir = os.path.abspath(outdir)
    os.makedirs(outdir, exist_ok=True)
    me = os.path.abspath(__file__)
    rows, stats = [], []
    for case in CASES:
        plain = os.path.join(outdir, f"rb_{case}.json")
        r = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT), sys.executable, me, "run", case, plain], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        if r.returncode != 0 or not os.path.exists(plain):
            print("[rb_slam_probe]", case, "failed", r.returncode, r.stdout.decode(errors="replace")[-800:], flush=True)
            break                                          # nothing more on the GPU in this run
        j = json.load(open(plain))
        d = os.path.join(outdir, "prof_" + case)
        subprocess.run(["rm", "-rf", d])
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT), "rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "p", "--", sys.executable, me, "run", case, "-",
               "noextras"]
        r = subprocess.run(cmd, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        dbs = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)
        if r.returncode != 0 or not dbs:
            print("[rb_slam_probe]", case, "profiled run failed", r.returncode, r.stdout.decode(errors="replace")[-800:], flush=True)
            break
        con = sqlite3.connect(dbs[0])
        q = "select name, count(*), sum(end-start), avg(end-start), min(end-start), max(end-start) from kernels group by name order by 3 desc"
        for name, calls, tot, avg, lo, hi in con.execute(q):
            stats.append([case, name.split("(")[0], calls, tot, "%.1f" % avg, lo, hi])
        rows.append([case, j["particles"], j["side"], j["rays"], j["updates"], j["resampled"], "%.3f" % j["update_ms"], "%.3f" % j["single_map_step_ms"],
                     "%.1f" % j["cpu_model_update_ms"], j["map_nonzero"]])
        print("[rb_slam_probe]", case, "done", flush=True)
    with open(os.path.join(outdir, "rb_slam_per_update.csv"), "w") as f:
        f.write("# host wall time per update, median of %d moved updates after %d warm-ups (1 / 1 schedule, device noise); single_map_step: bl_pf_update +\n"
                "# bl_mapping_update + sync at the same particle count; cpu_model: tests/rb_slam_model.py on one core (not the same machine part)\n" % (REPS, WARM))
        f.write("case,particles,side,rays,updates,resampled,update_ms,single_map_step_ms,cpu_model_update_ms,best_map_nonzero_cells\n")
        for row in rows:
            f.write(",".join(str(v) for v in row) + "\n")
        for c in CASES:
            if c not in [r[0] for r in rows]:
                f.write(f"# {c}: not run\n")
    with open(os.path.join(outdir, "rb_slam_kernel_stats.csv"), "w") as f:
        f.write("# rocprofv3 --kernel-trace --stats -- python tests/tools/rb_slam_probe.py run <case> - noextras\ncase,kernel,calls,total_ns,average_ns,min_ns,max_ns\n")
        for row in stats:
            f.write(",".join(str(v) for v in row) + "\n")
    return 0 if len(rows) == len(CASES) else 1


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "run":
        run(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 and sys.argv[3] != "-" else None, extras="noextras" not in sys.argv[4:])
    elif len(sys.argv) >= 2 and sys.argv[1] == "profile":
        sys.exit(profile(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles")))
    else:
        print(__doc__)
        sys.exit(2)
