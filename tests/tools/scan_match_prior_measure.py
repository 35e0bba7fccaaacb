"""What the scan match with a prior costs, and that it costs bl_scanmatch_match nothing (a tool, not a test).

  python3 tests/tools/scan_match_prior_measure.py run plain [LIB]
      bl_scanmatch_match at the six shapes of tests/tools/scan_match_probe.py (290-ray scans, windows (4, 4, 12), (20, 20, 30),
      (64, 64, 90) on a 200 x 200 and a 2000 x 2000 grid), WARM + N matches each.  LIB: another build of the library to load
      instead of botlab_amd/libbotlab_hip.so (the parent commit's, which lacks the new symbols).
  python3 tests/tools/scan_match_prior_measure.py run prior
      bl_scanmatch_match_prior at the same shapes, want_moments 0 and then 1.
  python3 tests/tools/scan_match_prior_measure.py unchanged PARENT_LIB [ROUNDS]
      (a) `run plain` under rocprofv3 --kernel-trace --stats (a run of its own each time, the program after --), the parent's
      library and this tree's alternated ROUNDS (3) times; prints per-match kernel medians per run as CSV
      (profiles/scan_match_prior_per_match.csv) and, per shape, both libraries' ranges over the rounds.
  python3 tests/tools/scan_match_prior_measure.py added
      (b) `run prior` under rocprofv3 likewise: per shape the kernels' medians with want_moments 0 and 1, the microseconds the
      moments add, and k_sm_moments' bytes/s (4 bytes per candidate, read once) against the HBM roof: 6.3e12 B/s achievable
      (8.0e12 spec).  A volume the scoring kernel has just written may be served from L2 or the Infinity Cache instead: a rate above
      the roof says so."""
import glob
import os
import re
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
HBM_ROOF = 6.3e12
PROFILE_TIMEOUT_S = 300
DTH = np.float32(np.radians(0.5))
PRIOR, HALF_LIFE = (512, 0, 512, 128), 200
NEW_SYMBOLS = ("bl_scanmatch_match_prior", "bl_scanmatch_covariance", "bl_scanmatch_refined_pose")
PLAIN_KERNELS = ("k_sm_raster", "k_sm_score", "k_sm_final")
PRIOR_KERNELS = ("k_sm_raster", "k_sm_score_prior", "k_sm_final_prior", "k_sm_moments", "k_sm_moments_final")


def configs():
    return [(g, w) for g in GRIDS for w in WINDOWS]


def run(mode, lib=None):
    from botlab_amd import _capi
    if lib:
        _capi.LIB_PATH = os.path.abspath(lib)
        for n in NEW_SYMBOLS:
            _capi.SIGNATURES.pop(n, None)
    import helpers
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
            kw = dict(nx=nx, ny=ny, ntheta=nt, dtheta=DTH, max_range=8.0)
            for want in ((None,) if mode == "plain" else (0, 1)):
                wall = []
                for i in range(WARM + N):
                    t0 = time.perf_counter()
                    if want is None:
                        res = matcher.match(scan, centre, g, **kw)
                    else:
                        res, _ = matcher.match_prior(scan, centre, g, prior=PRIOR, half_life=HALF_LIFE if want else None, **kw)
                    wall.append(time.perf_counter() - t0)
                print("CONFIG grid %d window %d %d %d rays %d path %d want %s wall_us %.1f" %
                      (size, nx, ny, nt, res.rays_used, matcher.debugPath(), "-" if want is None else want,
                       1e6 * statistics.median(wall[WARM:])), flush=True)
        g.close()
    matcher.close()


def kernel_times(args, kernels, per_config):
    """One rocprofv3 run of this file with `args`: ({kernel: [ns per launch, in launch order]}, the CONFIG lines)."""
    with tempfile.TemporaryDirectory(prefix="smp_measure_") as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "p", "--", sys.executable, os.path.abspath(__file__), "run"] + args
        r = subprocess.run(cmd, cwd=d, env=dict(os.environ, TMPDIR=d), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           timeout=PROFILE_TIMEOUT_S)
        text = r.stdout.decode(errors="replace")
        lines = [l.split() for l in text.splitlines() if l.startswith("CONFIG")]
        dbs = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)
        if r.returncode != 0 or len(lines) != per_config * len(configs()) or not dbs:
            print(text[-3000:])
            raise SystemExit("the profiled run did not finish (exit %d)" % r.returncode)
        con = sqlite3.connect(dbs[0])
        rows = list(con.execute("select name, start, end from kernels where name like '%k_sm_%' order by start"))
    per = {k: [] for k in kernels}
    for name, start, end in rows:
        ident = re.search(r"k_sm[a-z_]*", name).group(0)
        if ident in per:
            per[ident].append(end - start)
    return per, lines


def medians(per, block, count):
    """Median in microseconds of each kernel's launches block * count + WARM .. (block + 1) * count."""
    return {k: statistics.median(v[block * count + WARM:(block + 1) * count]) / 1e3 for k, v in per.items()}


def unchanged(parent_lib, rounds=3):
    print("# tests/tools/scan_match_prior_measure.py unchanged: bl_scanmatch_match, rocprofv3 --kernel-trace --stats, medians over %d matches "
          "after %d warm-up matches per shape and run; parent commit's library and this tree's alternated %d times" % (N, WARM, rounds))
    print("round,library,grid,nx,ny,ntheta,rays,path,raster_us,score_us,final_us,kernels_us,host_wall_us")
    totals = {}
    for rnd in range(rounds):
        for label, lib in (("parent", [os.path.abspath(parent_lib)]), ("branch", [])):      # the profiled run has its own directory
            per, lines = kernel_times(["plain"] + lib, PLAIN_KERNELS, 1)
            assert all(len(v) == len(configs()) * (WARM + N) for v in per.values()), {k: len(v) for k, v in per.items()}
            for c, (ln, (size, (nx, ny, nt))) in enumerate(zip(lines, configs())):
                med = medians(per, c, WARM + N)
                total = sum(med.values())
                totals.setdefault((size, nx, ny, nt), {}).setdefault(label, []).append(total)
                print("%d,%s,%d,%d,%d,%d,%d,%d,%.2f,%.2f,%.2f,%.2f,%.1f" % (rnd, label, size, nx, ny, nt, int(ln[8]), int(ln[10]), med["k_sm_raster"],
                                                                           med["k_sm_score"], med["k_sm_final"], total, float(ln[14])))
    print("# per shape: kernels_us of the parent's runs (min .. max) and of this tree's; inside = this tree's median lies within the parent's own range")
    for (size, nx, ny, nt), t in totals.items():
        p, b = sorted(t["parent"]), sorted(t["branch"])
        print("# grid %d window %d %d %d: parent %.2f .. %.2f, branch %.2f .. %.2f, branch median %.2f, %s" %
              (size, nx, ny, nt, p[0], p[-1], b[0], b[-1], statistics.median(b),
               "inside" if p[0] <= statistics.median(b) <= p[-1] else "OUTSIDE"))


def added():
    per, lines = kernel_times(["prior"], PRIOR_KERNELS, 2)
    count = WARM + N
    # raster / score / final run in every match (2 * count per shape); the moments kernels only in the second half (count per shape)
    print("# tests/tools/scan_match_prior_measure.py added: bl_scanmatch_match_prior, prior %s, half_life %d; medians over %d matches after %d warm-up" %
          (PRIOR, HALF_LIFE, N, WARM))
    print("grid,nx,ny,ntheta,path,want_moments,raster_us,score_prior_us,final_prior_us,moments_us,moments_final_us,kernels_us,host_wall_us,"
          "volume_bytes,moments_bytes_per_s,share_of_hbm_roof")
    for c, (size, (nx, ny, nt)) in enumerate(configs()):
        vol_bytes = 4 * (2 * nx + 1) * (2 * ny + 1) * (2 * nt + 1)
        sums = []
        for want in (0, 1):
            ln = lines[2 * c + want]
            med = {k: statistics.median(per[k][(2 * c + want) * count + WARM:(2 * c + want + 1) * count]) / 1e3
                   for k in ("k_sm_raster", "k_sm_score_prior", "k_sm_final_prior")}
            mom = {k: (statistics.median(per[k][c * count + WARM:(c + 1) * count]) / 1e3 if want else 0.0)
                   for k in ("k_sm_moments", "k_sm_moments_final")}
            total = sum(med.values()) + sum(mom.values())
            sums.append(total)
            rate = vol_bytes / (mom["k_sm_moments"] * 1e-6) if want else 0.0
            print("%d,%d,%d,%d,%d,%d,%.2f,%.2f,%.2f,%.2f,%.2f,%.2f,%.1f,%d,%.3e,%.3f" %
                  (size, nx, ny, nt, int(ln[10]), want, med["k_sm_raster"], med["k_sm_score_prior"], med["k_sm_final_prior"], mom["k_sm_moments"],
                   mom["k_sm_moments_final"], total, float(ln[14]), vol_bytes, rate, rate / HBM_ROOF))
        print("# grid %d window %d %d %d: the moments add %.2f us of kernel time" % (size, nx, ny, nt, sums[1] - sums[0]))
    assert all(len(per[k]) == 2 * count * len(configs()) for k in PRIOR_KERNELS[:3]) and \
        all(len(per[k]) == count * len(configs()) for k in PRIOR_KERNELS[3:]), {k: len(v) for k, v in per.items()}


if __name__ == "__main__":
    cmd = sys.argv[1] if len(sys.argv) > 1 else ""
    if cmd == "run" and len(sys.argv) >= 3 and sys.argv[2] in ("plain", "prior"):
        run(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
    elif cmd == "unchanged" and len(sys.argv) >= 3:
        unchanged(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 3)
    elif cmd == "added":
        added()
    else:
        raise SystemExit(__doc__)
