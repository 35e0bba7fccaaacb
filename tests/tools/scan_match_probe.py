"""What a correlative scan match costs (a tool, not a test).

  python3 tests/tools/scan_match_probe.py run        the matches themselves: 290-ray scans, windows (4, 4, 12), (20, 20, 30) and
                                                     (64, 64, 90) on a 200 x 200 and a 2000 x 2000 grid, WARM + N matches each; prints
                                                     host wall medians and the numpy model's time for the same match (one core)
  python3 tests/tools/scan_match_probe.py profile    runs `run` under rocprofv3 --kernel-trace --stats (a run of its own, the program
                                                     after --), splits the k_sm_* launches by configuration in launch order and prints
                                                     the medians as CSV (profiles/scan_match_per_match.csv), with the candidate-ray
                                                     rate against the bound of the path that ran

The bound of the path that ran.  Path 0 (window in LDS): ds_read_u8 is serviced like ds_read_b32, two LDS cycles per
wave-instruction = 32 lanes per clock and CU (MI355X: 256 CUs at 2.4 GHz) = 1.97e13 lookups / s.  Path 1 (grid read directly): a wave's
64 lookups of one ray are 64 consecutive bytes of a map row, one 64-byte request; rows served from L2 arrive at 66-73 GB/s per CU
(measured gather rate of L2-resident rows), 70e9 / 64 = 1.09e9 requests / s / CU = 7.0e10 lookups / s / CU = 1.79e13 lookups / s."""
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

WINDOWS = [(4, 4, 12), (20, 20, 30), (64, 64, 90)]
GRIDS = [200, 2000]
WARM, N = 10, 100
LDS_LOOKUPS_PER_S = 32 * 256 * 2.4e9
L2_LOOKUPS_PER_S = 70e9 / 64 * 64 * 256
PROFILE_TIMEOUT_S = 360
DTH = np.float32(np.radians(0.5))


def configs():
    return [(g, w) for g in GRIDS for w in WINDOWS]


def run():
    import helpers
    import scan_match_model as sm
    import botlab_amd as bl
    from botlab_amd import synth
    maps = helpers.load_reference_maps()
    ctx = bl.default_context()
    matcher = bl.ScanMatcher(ctx=ctx)
    base = maps["obstacle_slam_10mx10m_5cm"]
    for size in GRIDS:
        if size == 200:
            cells, origin = np.where(base["cells"] > 0, 127, -127).astype(np.int8), base["origin"]
        else:
            cells, origin = synth.tile_world(base["cells"], size), (np.float32(-size * 0.025), np.float32(-size * 0.025))
        g = bl.OccupancyGrid.from_cells(cells, origin, np.float32(0.05), cellsPerMeter=helpers.CPM_DEFAULT, ctx=ctx)
        pose = (-0.75, 0.2, 0.4)
        scan = synth.raycast_scan(cells, origin, 0.05, pose, pose, 1000)
        centre = bl.make_pose(pose[0] + 0.07, pose[1] - 0.04, pose[2] + 0.02)
        for nx, ny, nt in WINDOWS:
            wall = []
            for i in range(WARM + N):
                t0 = time.perf_counter()
                res = matcher.match(scan, centre, g, nx=nx, ny=ny, ntheta=nt, dtheta=DTH, max_range=8.0)
                wall.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            ref = sm.match(cells, origin, np.float32(0.05), helpers.CPM_DEFAULT, scan.ranges, scan.thetas, (centre.x, centre.y, centre.theta),
                           nx, ny, nt, DTH, 8.0)
            model_s = time.perf_counter() - t0
            assert (res.di, res.dj, res.dk, res.score, res.ties) == (ref["di"], ref["dj"], ref["dk"], ref["score"], ref["ties"])
            print("CONFIG grid %d window %d %d %d rays %d path %d wall_us %.1f model_ms %.1f" %
                  (size, nx, ny, nt, res.rays_used, matcher.debugPath(), 1e6 * statistics.median(wall[WARM:]), 1e3 * model_s), flush=True)
        g.close()
    matcher.close()


def profile():
    with tempfile.TemporaryDirectory(prefix="sm_probe_") as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "p", "--", sys.executable, os.path.abspath(__file__), "run"]
        r = subprocess.run(cmd, cwd=d, env=dict(os.environ, TMPDIR=d), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           timeout=PROFILE_TIMEOUT_S)
        text = r.stdout.decode(errors="replace")
        report(text, glob.glob(os.path.join(d, "**", "*.db"), recursive=True))


def report(text, dbs):
    lines = [l.split() for l in text.splitlines() if l.startswith("CONFIG")]
    if len(lines) != len(configs()):
        print(text[-3000:])
        raise SystemExit("the run did not finish")
    if not dbs:
        print(text[-3000:])
        raise SystemExit("no rocpd database")
    con = sqlite3.connect(dbs[0])
    rows = list(con.execute("select name, start, end from kernels where name like '%k_sm_%' order by start"))
    per = {k: [r[2] - r[1] for r in rows if k in r[0]] for k in ("k_sm_raster", "k_sm_score", "k_sm_final")}
    assert all(len(v) == len(configs()) * (WARM + N) for v in per.values()), {k: len(v) for k, v in per.items()}
    print("grid,nx,ny,ntheta,rays,path,raster_us,score_us,final_us,kernels_us,host_wall_us,model_ms,candidate_rays,rate_per_s,bound_per_s,share_of_bound")
    for c, (ln, (size, (nx, ny, nt))) in enumerate(zip(lines, configs())):
        med = {}
        for k, v in per.items():
            med[k] = statistics.median(v[c * (WARM + N) + WARM:(c + 1) * (WARM + N)]) / 1e3
        rays, path, wall, model = int(ln[8]), int(ln[10]), float(ln[12]), float(ln[14])
        work = (2 * nx + 1) * (2 * ny + 1) * (2 * nt + 1) * rays
        rate = work / (med["k_sm_score"] * 1e-6)
        bound = L2_LOOKUPS_PER_S if path else LDS_LOOKUPS_PER_S
        print("%d,%d,%d,%d,%d,%d,%.2f,%.2f,%.2f,%.2f,%.1f,%.1f,%d,%.3e,%.3e,%.3f" %
              (size, nx, ny, nt, rays, path, med["k_sm_raster"], med["k_sm_score"], med["k_sm_final"], sum(med.values()), wall, model, work,
               rate, bound, rate / bound))
    print("# rocprofv3 --stats, all configurations together:")
    for row in con.execute("select name, count(*), sum(end-start), avg(end-start), min(end-start), max(end-start) from kernels group by name order by 3 desc"):
        print("# %-50s calls %6d total_ns %12d avg_ns %10.0f min_ns %9d max_ns %10d" % (row[0][:50], row[1], row[2], row[3], row[4], row[5]))


if __name__ == "__main__":
    {"run": run, "profile": profile}[sys.argv[1] if len(sys.argv) > 1 else "run"]()
