"""The C++ layer of the scan match with a prior, built with g++ -std=c++11 from tests/cpp/scan_match_prior_test.cpp:
ScanMatcherT::matchWithPrior and scan_match_prior_from_sigmas (include/botlab/scan_matcher.hpp), and OccupancyGridSLAMT with
setScanMatchingPrior / setScanMatchingSubCell (include/botlab/slam_driver.hpp) against the model's chain
(tests/scan_match_prior_model.py), bit for bit.  The driver runs are the size of tests/test_gpu_scan_match_driver.py's: 5000
particles, 60 steps.  Figures of the full-SLAM run are recorded in DESIGN.md section 4.19."""
import math
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import botlab_amd as bl
import helpers
import scan_match_model as sm
import scan_match_prior_cases as pc
import scan_match_prior_model as smp
import test_gpu_scan_match_driver as drv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRIOR = (512, 0, 512, 128)               # two score units per cell^2, half a unit per heading step^2
HALF_LIFE = 200
RES_FMT = drv.RES_FMT
MOM_FMT = "<10q8i"
POSE_FMT = "<qfff"
IT_SIZE = 1 + 56 + 112 + 8 + 2 * 20


def _build(td, source="scan_match_prior_test"):
    exe = os.path.join(td, source)
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", source + ".cpp"), "-L" + os.path.join(ROOT, "botlab_amd"),
                           "-lbotlab_hip", "-Wl,-rpath," + os.path.join(ROOT, "botlab_amd"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def exe():
    with tempfile.TemporaryDirectory() as td:
        yield _build(td)


def test_prior_from_sigmas_cpp_equals_python(exe):
    """No device: the C++ function and botlab_amd.prior_from_sigmas state one rule."""
    for args in [(0.1, 0.2, 0.0, 0.02, 1.0, 0.05, 0.00872665), (0.05, 0.05, 0.5, 0.0174533, 4.0, 0.05, 0.00872665),
                 (0.03, 0.11, -0.9, 0.004, 37.5, 0.05, 0.00872665), (0.001, 0.2, 0.75, 0.0001, 10.0, 0.05, 0.01),
                 (float("inf"), 0.1, 0.0, float("inf"), 1.0, 0.05, 0.01), (0.0, 0.1, 0.0, 0.1, 1.0, 0.05, 0.01), (0.1, 0.1, 1.0, 0.1, 1.0, 0.05, 0.01)]:
        out = subprocess.run([exe, "sigmas"] + [repr(float(v)) for v in args], stdout=subprocess.PIPE, timeout=60, check=True).stdout.decode().split()
        try:
            want = [str(v) for v in bl.prior_from_sigmas(*args)] + ["0", "0"]
        except ValueError:
            want = ["invalid"]
        assert out == want, (args, out, want)


def _write_case(path, case):
    nx, ny, nt = case.window
    with open(path, "wb") as f:
        f.write(struct.pack("<fff", *(float(v) for v in case.centre)))
        f.write(struct.pack("<iiiffii", nx, ny, nt, float(case.dtheta), case.max_range, case.min_score, 0))
        f.write(struct.pack("<6i", *case.prior, case.half_life, 1))
        f.write(struct.pack("<i", len(case.ranges)) + case.ranges.tobytes() + case.thetas.tobytes())


def _result_of(raw, off=0):
    return struct.unpack_from(RES_FMT, raw, off)


def _check_result(res, ref, utime):
    assert res[0] == utime
    got_pose, exp_pose = np.array(res[1:4], np.float32), np.array([ref["x"], ref["y"], ref["theta"]], np.float32)
    assert got_pose.tobytes() == exp_pose.tobytes(), (got_pose, exp_pose)
    assert res[4:] == (ref["di"], ref["dj"], ref["dk"], ref["score"], ref["score_centre"], ref["ties"], ref["rays_used"], ref["accepted"]), (res, ref["sums"])


def _check_moments(mom, ref):
    assert mom[:10] == ref["sums"] and mom[10:12] == (ref["best_obj"], ref["pen_best"]), (mom, ref["sums"])
    assert tuple(zip(mom[12:15], mom[15:18])) == ref["fractions"], (mom, ref["fractions"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["window_4_4_12", "prior_moves_winner"])
def test_match_with_prior_equals_the_model(exe, name):
    case, ref = pc.get(name), pc.evaluate(pc.get(name))
    with tempfile.TemporaryDirectory() as td:
        mapfile, casefile, outp = os.path.join(td, "m.map"), os.path.join(td, "case.bin"), os.path.join(td, "out.bin")
        drv._write_map_file(mapfile, case.cells, case.origin, case.mpc)
        _write_case(casefile, case)
        r = subprocess.run([exe, "match", mapfile, casefile, outp], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert r.returncode == 0 and b"scan_match_prior_test ok" in r.stdout, (r.returncode, r.stderr.decode(errors="replace")[-2000:])
        raw = open(outp, "rb").read()
    _check_result(_result_of(raw), ref, pc.UTIME)
    _check_moments(struct.unpack_from(MOM_FMT, raw, 56), ref)
    (nv,) = struct.unpack_from("<i", raw, 168)
    vol = np.frombuffer(raw, dtype=np.int32, count=nv, offset=172).reshape(ref["volume"].shape)
    assert np.array_equal(vol, ref["volume"])
    assert struct.unpack_from("<ii", raw, 172 + 4 * nv) == (1, 1)          # without the moments: the same result, nothing kept


def _run(exe, script, mapfile, outp, prior, subcell, dump, min_score=0):
    arg = "-" if prior is None else ",".join(str(v) for v in prior)
    r = subprocess.run([exe, "drive", script, mapfile, outp, arg, str(int(subcell)), str(int(dump)), str(min_score)], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=600)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and "scan_match_prior_test ok" in out, (r.returncode, out[-500:], r.stderr.decode(errors="replace")[-2000:])
    raw = open(outp, "rb").read()
    its, grids, off = [], [], 0
    while raw[off:off + 1] in (b"I", b"M"):
        if raw[off:off + 1] == b"M":
            w, h = struct.unpack_from("<ii", raw, off + 1)
            grids.append(np.frombuffer(raw, dtype=np.int8, count=w * h, offset=off + 9).reshape(h, w).copy())
            off += 9 + w * h
        else:
            its.append(dict(res=_result_of(raw, off + 1), mom=struct.unpack_from(MOM_FMT, raw, off + 57),
                            counts=struct.unpack_from("<ii", raw, off + 169), pose=struct.unpack_from(POSE_FMT, raw, off + 177),
                            corrected=struct.unpack_from(POSE_FMT, raw, off + 197)))
            off += IT_SIZE
    assert raw[off:off + 1] == b"E"
    return its, grids


def _chain(its, grids, scans, origin32, mpc32, cpm, centres, prior, half_life, subcell, min_score):
    """The model's chain: every match around the centre formed from the model's own last corrected pose; the driver's result,
    moments and corrected pose must be the model's, bit for bit.  centres(k, last) gives the centre of iteration k."""
    last = (np.float32(0.0), np.float32(0.0), np.float32(0.0))
    moved_by_fraction = 0
    for k, (it, cells, scan) in enumerate(zip(its, grids, scans)):
        centre = centres(k, last)
        r = smp.match(cells, origin32, mpc32, cpm, scan.ranges, scan.thetas, centre, prior=prior, half_life=half_life, min_score=min_score,
                      utime=scan.utime, **drv.WINDOW)
        _check_result(it["res"], r, scan.utime)
        if half_life is not None:
            _check_moments(it["mom"], r)
        want = smp.refined_pose(r, centre, float(mpc32), float(drv.DTH)) if subcell else (r["x"], r["y"], r["theta"])
        got = np.array(it["corrected"][1:], np.float32)
        assert got.tobytes() == np.array(want, np.float32).tobytes(), (k, got, want)
        assert it["corrected"][0] == scan.utime and it["counts"][0] == k + 1
        moved_by_fraction += int(tuple(np.array(want, np.float32)) != (r["x"], r["y"], r["theta"]))
        last = tuple(np.float32(v) for v in want)
    return moved_by_fraction


@pytest.mark.gpu
def test_driver_with_prior_and_sub_cell_on_a_known_map(maps, exe):
    """Localization on a reference map with odometry frozen at the start pose (the matcher alone moves the filter): with the prior
    set, and separately with sub-cell on, the driver's matches, moments and corrected poses are the model's chain; with the
    switches unset the driver's matches are byte-equal to those of the driver test that knows nothing of them."""
    truthmap, origin, mpc, poses, scans, events = drv._scenario(maps)
    with tempfile.TemporaryDirectory() as td:
        old = drv._build(td)
        mapfile, script = os.path.join(td, "known.map"), os.path.join(td, "frozen.bin")
        drv._write_map_file(mapfile, truthmap, origin, mpc)
        drv._write_script(script, drv.N, events(lambda k: (0.0, 0.0, 0.0)))
        with_prior, g_prior = _run(exe, script, mapfile, os.path.join(td, "a.bin"), PRIOR + (HALF_LIFE, 1), subcell=False, dump=True)
        sub_cell, g_sub = _run(exe, script, mapfile, os.path.join(td, "b.bin"), PRIOR + (HALF_LIFE, 0), subcell=True, dump=True)
        only_sub, g_only = _run(exe, script, mapfile, os.path.join(td, "c.bin"), None, subcell=True, dump=True)
        unset, g_unset = _run(exe, script, mapfile, os.path.join(td, "d.bin"), None, subcell=False, dump=True)
        today, g_today = drv._run(old, script, mapfile, os.path.join(td, "e.bin"), matching=True, dump=True)
    assert len(with_prior) == len(sub_cell) == len(only_sub) == len(unset) == len(today) == len(scans)
    origin32, mpc32 = (np.float32(origin[0]), np.float32(origin[1])), np.float32(float("%g" % float(mpc)))
    frozen = lambda k, last: last                                                                  # noqa: E731
    args = (scans, origin32, mpc32, helpers.CPM_DEFAULT, frozen)
    # the map is extended from the filter's pose in this mode too, and the filter's first cloud is seeded from the OS: every run is
    # compared on the maps it dumped itself
    _chain(with_prior, g_prior, *args, PRIOR, HALF_LIFE, False, 0)
    moved = _chain(sub_cell, g_sub, *args, PRIOR, HALF_LIFE, True, 0)
    assert moved >= len(scans) // 2                             # the fractions are what moved the chain, not zeros
    _chain(only_sub, g_only, *args, (0, 0, 0, 0), 64, True, 0)
    # switches unset: today's driver.  Both runs are the plain model's chain (scan_match_model.match) on their own maps, bit for
    # bit; and while their maps coincide -- the first iteration at least, the map of the file -- the structs are compared directly.
    last_u = last_t = (np.float32(0.0), np.float32(0.0), np.float32(0.0))
    same_maps, direct = True, 0
    for k, (a, (res, it), scan) in enumerate(zip(unset, today, scans)):
        ru = sm.match(g_unset[k], origin32, mpc32, helpers.CPM_DEFAULT, scan.ranges, scan.thetas, last_u, min_score=0, utime=scan.utime, **drv.WINDOW)
        rt = sm.match(g_today[k], origin32, mpc32, helpers.CPM_DEFAULT, scan.ranges, scan.thetas, last_t, min_score=0, utime=scan.utime, **drv.WINDOW)
        _check_result(a["res"], ru, scan.utime)
        _check_result(res, rt, scan.utime)
        assert a["counts"] == it[:2] == (k + 1, k + 1)
        assert a["mom"] == (0,) * 18 and a["corrected"][1:] == a["res"][1:4] and a["corrected"][0] == scan.utime
        same_maps = same_maps and np.array_equal(g_unset[k], g_today[k])
        if same_maps:
            assert struct.pack(RES_FMT, *a["res"]) == struct.pack(RES_FMT, *res)
            direct += 1
        last_u, last_t = (ru["x"], ru["y"], ru["theta"]), (rt["x"], rt["y"], rt["theta"])
    assert direct >= 1
    for name, its in (("prior", with_prior), ("prior + sub-cell", sub_cell), ("unset", unset)):
        e, h = drv._errors((None, (0, 0) + its[-1]["pose"]), poses[-1])
        ec = math.hypot(its[-1]["corrected"][1] - poses[-1][0], its[-1]["corrected"][2] - poses[-1][1])
        print("known map, frozen odometry, %s: final SLAM-pose error %.4f m / %.3f deg; corrected pose %.4f m" % (name, e, math.degrees(h), ec))


@pytest.mark.gpu
def test_driver_full_slam_with_prior(maps, exe):
    """Full SLAM from an empty map, true odometry, min_score = 1, the prior on (and, separately, sub-cell too): every centre -- the
    last corrected pose composed with the odometry's motion -- and every match against the map as the run has built it equal the
    model's chain.  The final errors are printed: a measurement next to DESIGN.md 4.11's 0.257 m / 4.7 deg, no threshold."""
    truthmap, origin, mpc, poses, scans, events = drv._scenario(maps)
    odo32 = [tuple(np.float32(v) for v in p) for p in poses]
    origin32, mpc32 = (np.float32(-5.0), np.float32(-5.0)), np.float32(0.05)
    with tempfile.TemporaryDirectory() as td:
        script = os.path.join(td, "true.bin")
        drv._write_script(script, drv.N, events(lambda k: poses[k]))
        runs = [("prior", _run(exe, script, "-", os.path.join(td, "a.bin"), PRIOR + (HALF_LIFE, 1), subcell=False, dump=True, min_score=1), False),
                ("prior + sub-cell", _run(exe, script, "-", os.path.join(td, "b.bin"), PRIOR + (HALF_LIFE, 1), subcell=True, dump=True, min_score=1), True)]
    for name, (its, grids), subcell in runs:
        assert len(its) == len(scans) == len(grids) and not grids[0].any()
        assert its[0]["res"][4:8] == (0, 0, 0, 0) and its[0]["res"][11] == 0                       # an empty map: the centre, not accepted
        assert any(it["res"][11] == 1 for it in its[1:])
        state = dict(prev=None)

        def centre(k, last):
            now = drv._odometry_at_scan(odo32, k + 1)
            prev = state["prev"] if state["prev"] is not None else now
            state["prev"] = now
            return sm.compose_delta(last, prev, now)
        _chain(its, grids, scans, origin32, mpc32, np.float32(1.0) / mpc32, centre, PRIOR, HALF_LIFE, subcell, 1)
        e, h = drv._errors((None, (0, 0) + its[-1]["pose"]), poses[-1])
        print("full SLAM, true odometry, matching with %s: final error %.4f m / %.3f deg" % (name, e, math.degrees(h)))
