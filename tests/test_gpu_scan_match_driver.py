"""OccupancyGridSLAMT with setScanMatching (include/botlab/slam_driver.hpp), built with g++ -std=c++11 from
tests/cpp/scan_match_driver_test.cpp.  Localization-only mode on a reference map, the start at the map frame's origin, synthetic
scans along a square trajectory that ends 0.8 m from its start, and ODOMETRY FROZEN AT THE START POSE: without the matcher the filter
never moves.

Figures of the run recorded in DESIGN.md section 4.11 (5000 particles; the driver seeds the initial cloud from the OS, as the
reference does, so they vary by a few millimetres; the action noise stream and the rand() sequence are the same in all runs)."""
import math
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import helpers
import scan_match_model as sm
from botlab_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAP = "obstacle_slam_10mx10m_5cm"
START = (-0.75, 0.2, 0.0)
STEPS = 60
TRAJ = dict(step_len=0.03, turn=0.05, side=0.8)
N = 5000
DTH = np.float32(0.5 * math.pi / 180.0)          # default_scan_match_params(): +-4 cells, +-12 steps of half a degree, 8 m
WINDOW = dict(nx=4, ny=4, ntheta=12, dtheta=DTH, max_range=8.0)
RES_FMT = "<qfff4x8i"                            # bl_scan_match_result_t: pose (24 bytes), di dj dk score score_centre ties rays_used accepted
IT_FMT = "<iiqfff"                               # matches so far, map updates so far, current pose


def _build(td):
    exe = os.path.join(td, "scan_match_driver_test")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "scan_match_driver_test.cpp"), "-L" + os.path.join(ROOT, "botlab_amd"),
                           "-lbotlab_hip", "-Wl,-rpath," + os.path.join(ROOT, "botlab_amd"), "-o", exe])
    return exe


def _write_map_file(path, cells, origin, mpc):
    """The reference's ASCII .map format (occupancy_grid.cpp:111-136)."""
    with open(path, "w") as f:
        f.write(f"{float(origin[0]):g} {float(origin[1]):g} {cells.shape[1]} {cells.shape[0]} {float(mpc):g}\n")
        for row in cells:
            f.write(" ".join(str(int(v)) for v in row) + " \n")


def _write_script(path, n, events):
    with open(path, "wb") as f:
        f.write(struct.pack("<ii", n, len(events)))
        for kind, x in events:
            f.write(kind.encode())
            if kind == "O":
                f.write(struct.pack("<qfff", int(x[0]), x[1], x[2], x[3]))
            else:
                f.write(struct.pack("<qi", x.utime, x.num_ranges) + x.ranges.tobytes() + x.thetas.tobytes() + x.times.tobytes())


def _run(exe, script, mapfile, outp, matching, dump, min_score=0):
    r = subprocess.run([exe, script, mapfile, outp, str(int(matching)), str(int(dump)), str(min_score)], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=600)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and "scan_match_driver_test ok" in out, (r.returncode, out[-500:], r.stderr.decode(errors="replace")[-2000:])
    raw = open(outp, "rb").read()
    its, grids, off = [], [], 0
    while raw[off:off + 1] in (b"I", b"M"):
        if raw[off:off + 1] == b"M":
            w, h = struct.unpack_from("<ii", raw, off + 1)
            grids.append(np.frombuffer(raw, dtype=np.int8, count=w * h, offset=off + 9).reshape(h, w).copy())
            off += 9 + w * h
        else:
            res = struct.unpack_from(RES_FMT, raw, off + 1)
            it = struct.unpack_from(IT_FMT, raw, off + 1 + 56)
            its.append((res, it))
            off += 1 + 56 + struct.calcsize(IT_FMT)
    assert struct.calcsize(RES_FMT) == 56 and raw[off:off + 1] == b"E"
    return its, grids


def _scenario(maps):
    m = maps[MAP]
    cells, mpc = m["cells"], m["mpc"]
    truthmap = np.where(cells > 0, 127, -127).astype(np.int8)
    x0, y0, t0 = START
    origin = (float(m["origin"][0]) - x0, float(m["origin"][1]) - y0)          # the start is the map frame's origin
    origin = tuple(float("%g" % v) for v in origin)                            # as the map file carries it
    poses = [(p[0] - x0, p[1] - y0, p[2]) for p in synth.square_trajectory(START, STEPS, **TRAJ)]
    assert math.hypot(poses[-1][0], poses[-1][1]) >= 0.5
    ts = 1_000_000
    scans = [synth.raycast_scan(truthmap, origin, 0.05, poses[k - 1], poses[k], ts + k * 100_000) for k in range(1, len(poses))]

    def events(odometry):
        ev = []
        for k in range(len(poses)):
            ev.append(("O", (ts + k * 100_000, *[np.float32(v) for v in odometry(k)])))
            if k >= 1:
                ev.append(("L", scans[k - 1]))
        return ev
    return truthmap, origin, mpc, poses, scans, events


def _errors(it, truth):
    _, (_, _, _, x, y, th) = it
    return math.hypot(x - truth[0], y - truth[1]), abs(math.atan2(math.sin(th - truth[2]), math.cos(th - truth[2])))


def test_driver_tracks_with_frozen_odometry(maps):
    truthmap, origin, mpc, poses, scans, events = _scenario(maps)
    frozen, true_odo = (lambda k: (0.0, 0.0, 0.0)), (lambda k: poses[k])
    with tempfile.TemporaryDirectory() as td:
        exe = _build(td)
        mapfile = os.path.join(td, "known.map")
        _write_map_file(mapfile, truthmap, origin, mpc)
        s_frozen, s_true = os.path.join(td, "frozen.bin"), os.path.join(td, "true.bin")
        _write_script(s_frozen, N, events(frozen))
        _write_script(s_true, N, events(true_odo))
        on, grids = _run(exe, s_frozen, mapfile, os.path.join(td, "a.bin"), matching=True, dump=True)
        ref, _ = _run(exe, s_true, mapfile, os.path.join(td, "b.bin"), matching=False, dump=False)       # the yardstick: today's path
        off, _ = _run(exe, s_frozen, mapfile, os.path.join(td, "c.bin"), matching=False, dump=False)
    assert len(on) == len(ref) == len(off) == len(scans) == len(grids)

    # (a) the corrected poses the driver hands to the filter are the model's chain, bit for bit
    origin32 = (np.float32(origin[0]), np.float32(origin[1]))
    last = (np.float32(0.0), np.float32(0.0), np.float32(0.0))
    for k, ((res, it), cells, scan) in enumerate(zip(on, grids, scans)):
        r = sm.match(cells, origin32, np.float32(float("%g" % float(mpc))), helpers.CPM_DEFAULT, scan.ranges, scan.thetas, last,
                     min_score=0, utime=scan.utime, **WINDOW)
        exp_pose = np.array([r["x"], r["y"], r["theta"]], np.float32)
        got_pose = np.array(res[1:4], np.float32)
        assert got_pose.tobytes() == exp_pose.tobytes(), (k, got_pose, exp_pose)
        assert res[0] == scan.utime
        assert res[4:] == (r["di"], r["dj"], r["dk"], r["score"], r["score_centre"], r["ties"], r["rays_used"], r["accepted"]), (k, res, r)
        assert it[0] == k + 1                                    # one match per iteration
        last = (r["x"], r["y"], r["theta"])

    # (b) against the yardstick (true odometry, matching off)
    e_ref, h_ref = _errors(ref[-1], poses[-1])
    e_on, h_on = _errors(on[-1], poses[-1])
    e_off, h_off = _errors(off[-1], poses[-1])
    print("final SLAM-pose error: yardstick %.4f m / %.3f deg; frozen odometry, matching on %.4f m / %.3f deg; frozen, off %.4f m / %.3f deg"
          % (e_ref, math.degrees(h_ref), e_on, math.degrees(h_on), e_off, math.degrees(h_off)))
    bound_pos, bound_heading = e_ref + 0.10, h_ref + 2.0 * float(DTH)
    assert e_on <= bound_pos and h_on <= bound_heading
    assert e_off > bound_pos                                     # without the matcher frozen odometry loses the robot


def _odometry_at_scan(odo32, k):
    """PoseTraceT::poseAt at the stamp of odometry sample k >= 1 (slam_detail::between of samples k - 1 and k at ratio 1.0: float
    differences, double steps, narrowed once)."""
    a, b = odo32[k - 1], odo32[k]
    x = np.float32(float(a[0]) + float(np.float32(b[0] - a[0])) * 1.0)
    y = np.float32(float(a[1]) + float(np.float32(b[1] - a[1])) * 1.0)

    def back(v):
        return v if abs(v) <= math.pi else (v - 2.0 * math.pi if v > 0 else v + 2.0 * math.pi)
    th = np.float32(back(float(a[2]) + back(float(b[2]) - float(a[2])) * 1.0))
    return x, y, th


def test_driver_full_slam_from_an_empty_map(maps):
    """Full SLAM from an empty map, true odometry, matching on with min_score = 1.  Every centre the driver forms -- the last
    corrected pose composed with the odometry's motion since the last scan -- and every match against the map as the run has built
    it equal the model's chain (scan_match_model.compose_delta + match), bit for bit."""
    truthmap, origin, mpc, poses, scans, events = _scenario(maps)
    with tempfile.TemporaryDirectory() as td:
        exe = _build(td)
        script = os.path.join(td, "true.bin")
        _write_script(script, N, events(lambda k: poses[k]))
        its, grids = _run(exe, script, "-", os.path.join(td, "o.bin"), matching=True, dump=True, min_score=1)
    assert len(its) == len(scans) == len(grids)
    res, it = its[0]
    # the first match meets an empty map: nothing scores, it is not accepted, the result is the centre -- the start pose
    assert not grids[0].any()
    assert res[4:8] == (0, 0, 0, 0) and res[11] == 0 and res[1:4] == (0.0, 0.0, 0.0)
    assert its[-1][1][0] == len(scans) and its[-1][1][1] == len(scans)          # a match and a map update per iteration
    assert any(r[11] == 1 for r, _ in its[1:])                  # later matches find the map the run has built
    # the chain: OccupancyGridSLAMT() makes a 10 m x 10 m grid at 5 cm about the origin
    odo32 = [tuple(np.float32(v) for v in p) for p in poses]
    origin32, mpc32 = (np.float32(-5.0), np.float32(-5.0)), np.float32(0.05)
    last, odo_prev = (np.float32(0.0), np.float32(0.0), np.float32(0.0)), None
    moved = 0
    for k, ((res, _), cells, scan) in enumerate(zip(its, grids, scans)):
        odo_now = _odometry_at_scan(odo32, k + 1)
        if odo_prev is None:
            odo_prev = odo_now
        centre = sm.compose_delta(last, odo_prev, odo_now)
        moved += int(tuple(centre) != tuple(last))
        r = sm.match(cells, origin32, mpc32, np.float32(1.0) / mpc32, scan.ranges, scan.thetas, centre, min_score=1, utime=scan.utime, **WINDOW)
        got_pose, exp_pose = np.array(res[1:4], np.float32), np.array([r["x"], r["y"], r["theta"]], np.float32)
        assert got_pose.tobytes() == exp_pose.tobytes(), (k, got_pose, exp_pose, centre)
        assert res[4:] == (r["di"], r["dj"], r["dk"], r["score"], r["score_centre"], r["ties"], r["rays_used"], r["accepted"]), (k, res, r)
        last, odo_prev = (r["x"], r["y"], r["theta"]), odo_now
    assert moved >= len(scans) - 2                              # the composition with a non-zero motion is what ran
    e, h = _errors(its[-1], poses[-1])
    print("full SLAM, true odometry, matching on: final error %.4f m / %.3f deg" % (e, math.degrees(h)))
