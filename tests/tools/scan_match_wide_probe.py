"""What a wide (pruned) correlative scan match costs (a tool, not a test).

  python3 tests/tools/scan_match_wide_probe.py run        290-ray scans; (a) 200 x 200, +-64 / +-64 / +-90 x 0.5 deg: bl_scanmatch_match
                                                          (the yardstick), the wide match, its exhaustive form; (b) 200 x 200, the
                                                          whole map +-100 / +-100, +-180 x 1 deg; (c) 2000 x 2000 tiled world, +-1000 /
                                                          +-1000, +-180 x 1 deg; (d) 4096 x 4096, +-2048 / +-2048, +-180 x 1 deg.  WARM + N
                                                          matches each (the exhaustive forms of (b), (c): fewer, see CASES); prints
                                                          host wall medians, their spread, and the statistics of the pruning
  python3 tests/tools/scan_match_wide_probe.py profile    runs `run` under rocprofv3 --kernel-trace --stats (a run of its own, the
                                                          program after --), splits the launches by case in launch order and
                                                          prints the per-kernel medians as CSV (profiles/scan_match_wide_per_match.csv)"""
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

WARM, N = 10, 100
PROFILE_TIMEOUT_S = 420
DEG = np.float32(np.radians(1.0))
HALF = np.float32(np.radians(0.5))
# name, grid, (nx, ny, ntheta), dtheta, form, warm-up, matches
CASES = [("a", 200, (64, 64, 90), HALF, "narrow", WARM, N), ("a", 200, (64, 64, 90), HALF, "wide", WARM, N),
         ("a", 200, (64, 64, 90), HALF, "exhaustive", WARM, N),
         ("b", 200, (100, 100, 180), DEG, "wide", WARM, N), ("b", 200, (100, 100, 180), DEG, "exhaustive", 2, 10),
         ("c", 2000, (1000, 1000, 180), DEG, "wide", WARM, N), ("c", 2000, (1000, 1000, 180), DEG, "exhaustive", 1, 2),
         ("d", 4096, (2048, 2048, 180), DEG, "wide", 3, 20)]
KERNELS = {"narrow": ("k_sm_raster", "k_sm_score", "k_sm_final"),
           "wide": ("k_sm_raster", "k_smw_pool_rows", "k_smw_pool_cols", "k_smw_bounds", "k_smw_seed", "k_smw_compact", "k_smw_exact",
                    "k_smw_final"),
           "exhaustive": ("k_sm_raster", "k_smw_exact", "k_smw_final")}
ALL_KERNELS = ("k_sm_raster", "k_sm_score", "k_sm_final", "k_smw_pool_rows", "k_smw_pool_cols", "k_smw_bounds", "k_smw_seed",
               "k_smw_compact", "k_smw_exact", "k_smw_final")


def run():
    import helpers
    import botlab_amd as bl
    from botlab_amd import synth
    maps = helpers.load_reference_maps()
    ctx = bl.default_context()
    matcher = bl.ScanMatcher(ctx=ctx)
    base = maps["obstacle_slam_10mx10m_5cm"]
    grids = {}
    for name, size, (nx, ny, nt), dth, form, warm, n in CASES:
        if size not in grids:
            if size == 200:
                cells, origin = np.where(base["cells"] > 0, 127, -127).astype(np.int8), base["origin"]
            else:
                cells, origin = synth.tile_world(base["cells"], size), (np.float32(-size * 0.025), np.float32(-size * 0.025))
            g = bl.OccupancyGrid.from_cells(cells, origin, np.float32(0.05), cellsPerMeter=helpers.CPM_DEFAULT, ctx=ctx)
            pose = (-0.75, 0.2, 0.4)
            grids[size] = (g, synth.raycast_scan(cells, origin, 0.05, pose, pose, 1000))
        g, scan = grids[size]
        centre = bl.make_pose(0.07, -0.04, 0.02)
        wall = []
        for i in range(warm + n):
            t0 = time.perf_counter()
            if form == "narrow":
                res = matcher.match(scan, centre, g, nx=nx, ny=ny, ntheta=nt, dtheta=dth, max_range=8.0)
            else:
                res = matcher.match_wide(scan, centre, g, nx=nx, ny=ny, ntheta=nt, dtheta=dth, max_range=8.0, exhaustive=form == "exhaustive")
            wall.append(1e6 * (time.perf_counter() - t0))
        wall = sorted(wall[warm:])
        st = matcher.wide_stats() if form != "narrow" else None
        print("CASE %s grid %d window %d %d %d form %s result %d %d %d %d %d wall_us %.1f p10 %.1f p90 %.1f stats %s" %
              (name, size, nx, ny, nt, form, res.di, res.dj, res.dk, res.score, res.ties, statistics.median(wall), wall[len(wall) // 10],
               wall[(9 * len(wall)) // 10 - 1],
               "%d %d %d %d %d %d" % (st.candidates, st.blocks, st.blocks_kept, st.candidates_scored, st.block_log2, st.path) if st else "-"),
              flush=True)
    matcher.close()


def profile():
    with tempfile.TemporaryDirectory(prefix="smw_probe_") as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "p", "--", sys.executable, os.path.abspath(__file__), "run"]
        r = subprocess.run(cmd, cwd=d, env=dict(os.environ, TMPDIR=d), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           timeout=PROFILE_TIMEOUT_S)
        text = r.stdout.decode(errors="replace")
        report(text, glob.glob(os.path.join(d, "**", "*.db"), recursive=True))


def report(text, dbs):
    lines = [l for l in text.splitlines() if l.startswith("CASE")]
    for l in lines:
        print("# " + l)
    if len(lines) != len(CASES) or not dbs:
        print(text[-3000:])
        raise SystemExit("the run did not finish, or left no rocpd database")
    con = sqlite3.connect(dbs[0])
    rows = list(con.execute("select name, start, end from kernels where name like '%k_sm%' order by start"))
    per = {k: [r[2] - r[1] for r in rows if k in r[0]] for k in ALL_KERNELS}   # no name is part of another
    taken = {k: 0 for k in ALL_KERNELS}
    print("case,grid,nx,ny,ntheta,form," + ",".join(k + "_us" for k in ALL_KERNELS) + ",kernels_us,kernels_p10_us,kernels_p90_us")
    for name, size, (nx, ny, nt), dth, form, warm, n in CASES:
        med, totals = {}, None
        for k in ALL_KERNELS:
            if k not in KERNELS[form]:
                med[k] = 0.0
                continue
            v = per[k][taken[k] + warm:taken[k] + warm + n]
            taken[k] += warm + n
            assert len(v) == n, (name, form, k, len(v))
            med[k] = statistics.median(v) / 1e3
            totals = v if totals is None else [a + b for a, b in zip(totals, v)]
        totals = sorted(t / 1e3 for t in totals)
        print("%s,%d,%d,%d,%d,%s," % (name, size, nx, ny, nt, form) + ",".join("%.2f" % med[k] for k in ALL_KERNELS) +
              ",%.2f,%.2f,%.2f" % (statistics.median(totals), totals[len(totals) // 10], totals[(9 * len(totals)) // 10 - 1]))
    print("# rocprofv3 --stats, all cases together:")
    for row in con.execute("select name, count(*), sum(end-start), avg(end-start), min(end-start), max(end-start) from kernels group by name order by 3 desc"):
        print("# %-50s calls %6d total_ns %12d avg_ns %10.0f min_ns %9d max_ns %10d" % (row[0][:50], row[1], row[2], row[3], row[4], row[5]))


if __name__ == "__main__":
    {"run": run, "profile": profile}[sys.argv[1] if len(sys.argv) > 1 else "run"]()
