"""What the per-particle scan match of the Rao-Blackwellized SLAM costs (a tool, not a test).

  python3 tests/tools/rb_slam_match_probe.py run        matched updates: 290-ray scans, P in {64, 1024, 4096} x windows (2, 2, 4) and
                                                        (4, 4, 8) on 200 x 200 maps (path 0, the window in LDS), and P = 1024, window
                                                        (2, 2, 4) on 400 x 400 maps of 1.25 cm cells (path 1, the map read directly);
                                                        WARM + N moved updates each, every particle holding the finished map
  python3 tests/tools/rb_slam_match_probe.py profile    runs `run` under rocprofv3 --kernel-trace --stats (a run of its own, the
                                                        program after --), splits the k_rb_match launches by configuration in launch
                                                        order and prints the medians as CSV (profiles/rb_slam_match_kernel_stats.csv)

The rate is candidate-ray lookups per second, P (2 nx + 1)(2 ny + 1)(2 ntheta + 1) rays / time of k_rb_match, beside the two yardsticks
of tests/tools/scan_match_probe.py: k_sm_score's measured 2.44e12 / s and the LDS byte-gather bound of 32 lanes per clock and CU,
1.97e13 / s."""
import glob
import os
import sqlite3
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

CONFIGS = [(200, P, w) for P in (64, 1024, 4096) for w in ((2, 2, 4), (4, 4, 8))] + [(400, 1024, (2, 2, 4))]
WARM, N = 10, 100
K_SM_SCORE_PER_S = 2.44e12
LDS_LOOKUPS_PER_S = 32 * 256 * 2.4e9
PROFILE_TIMEOUT_S = 900
DTH = np.float32(np.radians(0.5))


def run():
    import helpers
    import botlab_amd as bl
    from botlab_amd import synth
    maps = helpers.load_reference_maps()
    ctx = bl.default_context()
    base = maps["obstacle_slam_10mx10m_5cm"]
    truth = np.where(base["cells"] > 0, 127, -127).astype(np.int8)
    pose = (-0.75, 0.2, 0.4)
    scan = synth.raycast_scan(truth, base["origin"], 0.05, pose, pose, 1000)
    for size, P, (nx, ny, nt) in CONFIGS:
        if size == 200:
            cells, origin, mpc, cpm = base["cells"], base["origin"], np.float32(0.05), helpers.CPM_DEFAULT
        else:                                                   # the 5 m x 5 m around the robot at four times the resolution
            x0, y0 = int((pose[0] + 5.0) / 0.05) - 50, int((pose[1] + 5.0) / 0.05) - 50
            cells = np.kron(base["cells"][y0:y0 + 100, x0:x0 + 100], np.ones((4, 4), np.int8))
            origin = (np.float32(float(base["origin"][0]) + 0.05 * x0), np.float32(float(base["origin"][1]) + 0.05 * y0))
            mpc, cpm = np.float32(0.0125), np.float32(80.0)
        rb = bl.RBSlam(P, size, size, mpc, cpm, origin, 5.0, 3, 1, ctx=ctx)
        rb.setResampling(1, 65535)                              # never due: no map copies between the matches
        rb.initializeAtPose(bl.make_pose(pose[0], pose[1], pose[2], utime=1000), seed=5)
        for p in range(P):
            rb.uploadMap(p, cells)
        rb.setScanMatching(nx, ny, nt, DTH, 8.0, 0)
        noise = np.zeros((P, 3), np.float32)                    # the sampled motion itself: the particles stay where they are
        wall, rays = [], int(np.count_nonzero((scan.ranges > 0.15) & (scan.ranges < 8.0)))
        for i in range(WARM + N + 1):                           # update 0 latches and does not move
            t0 = time.perf_counter()
            s = bl.LidarScan(scan.ranges, scan.thetas, scan.times + 100000 * i, utime=scan.utime + 100000 * i)
            r = rb.update(bl.make_pose(pose[0] + 0.02 * (i & 1), pose[1], pose[2], utime=s.utime), s, rand_value=i, noise=noise)
            wall.append(time.perf_counter() - t0)
            assert r["moved"] == (i > 0)
        mt = rb.debugMatch()
        print("CONFIG grid %d P %d window %d %d %d rays %d path %d update_wall_us %.1f off_centre %d mean_score %.0f" %
              (size, P, nx, ny, nt, rays, rb.debugMatchPath(), 1e6 * statistics.median(wall[WARM + 1:]),
               int(np.count_nonzero(mt["di"] | mt["dj"] | mt["dk"])), float(mt["score"].mean())), flush=True)
        rb.close()


def profile():
    with tempfile.TemporaryDirectory(prefix="rbm_probe_") as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "p", "--", sys.executable, os.path.abspath(__file__), "run"]
        r = subprocess.run(cmd, cwd=d, env=dict(os.environ, TMPDIR=d), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           timeout=PROFILE_TIMEOUT_S)
        text = r.stdout.decode(errors="replace")
        report(text, glob.glob(os.path.join(d, "**", "*.db"), recursive=True))


def report(text, dbs):
    lines = [l.split() for l in text.splitlines() if l.startswith("CONFIG")]
    if len(lines) != len(CONFIGS):
        print(text[-3000:])
        raise SystemExit("the run did not finish")
    if not dbs:
        print(text[-3000:])
        raise SystemExit("no rocpd database")
    con = sqlite3.connect(dbs[0])
    rows = list(con.execute("select name, start, end from kernels where name like '%k_rb_%' order by start"))
    pick = {"k_rb_match": lambda n: "k_rb_match" in n, "k_rb_weigh_matched": lambda n: "k_rb_weigh_matched" in n,
            "k_rb_map": lambda n: "k_rb_map" in n and "k_rb_map_io" not in n}
    per = {k: [r[2] - r[1] for r in rows if f(r[0])] for k, f in pick.items()}
    assert all(len(v) == len(CONFIGS) * (WARM + N) for v in per.values()), {k: len(v) for k, v in per.items()}
    print("grid,P,nx,ny,ntheta,rays,path,match_us,weigh_us,map_us,update_wall_us,candidate_rays,rate_per_s,share_of_k_sm_score,share_of_lds_bound")
    for c, (ln, (size, P, (nx, ny, nt))) in enumerate(zip(lines, CONFIGS)):
        med = {k: statistics.median(v[c * (WARM + N) + WARM:(c + 1) * (WARM + N)]) / 1e3 for k, v in per.items()}
        rays, path, wall = int(ln[10]), int(ln[12]), float(ln[14])
        work = P * (2 * nx + 1) * (2 * ny + 1) * (2 * nt + 1) * rays
        rate = work / (med["k_rb_match"] * 1e-6)
        print("%d,%d,%d,%d,%d,%d,%d,%.2f,%.2f,%.2f,%.1f,%d,%.3e,%.3f,%.3f" %
              (size, P, nx, ny, nt, rays, path, med["k_rb_match"], med["k_rb_weigh_matched"], med["k_rb_map"], wall, work, rate,
               rate / K_SM_SCORE_PER_S, rate / LDS_LOOKUPS_PER_S))
    print("# rocprofv3 --stats, all configurations together:")
    for row in con.execute("select name, count(*), sum(end-start), avg(end-start), min(end-start), max(end-start) from kernels group by name order by 3 desc"):
        print("# %-50s calls %6d total_ns %12d avg_ns %10.0f min_ns %9d max_ns %10d" % (row[0][:50], row[1], row[2], row[3], row[4], row[5]))


if __name__ == "__main__":
    {"run": run, "profile": profile}[sys.argv[1] if len(sys.argv) > 1 else "run"]()
