"""bl_pfmodel.h compiled for the host (tests/cpp/pfmodel_ref.cpp), without a GPU: the one copy of the motion model, the plain sensor
model and the low-variance draw that the particle filter (bl_mcl.hip) and RB-SLAM (bl_rbslam.hip) share, against the oracle's own
entry points.

  * bl_action_update against orc_pf_action_state: rot1, trans, rot2 as doubles bit for bit and `moved`, over one odometry sequence
    with the latching first call, a step below trans < 0.0001 with a turn, a backward step (|rot1| > pi/2), steps on both sides of
    the `moved` threshold (|trans| + |rot2| < 0.00001f) and headings across +-pi;
  * bl_pf_apply_action with a noise table against orc_action_apply_noise, poses whose heading wraps among them, float bits;
  * bl_ray_pose + bl_ray_setup + bl_score_ray_half_units over bl_grid_odds, summed per particle, equal to 2 * orc_likelihood exactly:
    an 8 x 6 and a 40 x 40 grid, rays ending on every border row and column, one cell outside, far outside (negative and >= width),
    and an interpolated scan (parent utime != pose utime);
  * bl_score_units at -1, 0, 1 and BL_RBSLAM_SCORE_MAX;
  * bl_resample_offset at rand() = 0 and RAND_MAX, and the draw against orc_resample_indices on an unequal 7-particle set;
  * bl_particle_fill zeroes the padding of the exported particle."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest

import oracle_lib
import resample_rule_model as rrm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MPC, CPM = np.float32(0.05), np.float32(20.0)
SCORE_MAX = 1 << 33                          # BL_RBSLAM_SCORE_MAX
POSE_DTYPE = np.dtype([("utime", "<i8"), ("x", "<f4"), ("y", "<f4"), ("theta", "<f4"), ("_pad", "<f4")])


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("pfmodel") / "pfmodel_ref.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-shared", "-fPIC", "-o", so,
                           os.path.join(ROOT, "tests", "cpp", "pfmodel_ref.cpp")])
    lib = C.CDLL(so)
    lib.pm_likelihood_half_units.restype = C.c_longlong
    lib.pm_likelihood_half_units.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int,
                                             C.c_void_p, C.c_void_p, C.c_void_p]
    lib.pm_score_units.restype = C.c_ulonglong
    lib.pm_score_units.argtypes = [C.c_longlong]
    lib.pm_resample_offset.restype = C.c_double
    lib.pm_resample_offset.argtypes = [C.c_int, C.c_double]
    lib.pm_particle.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_double]
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# ---------------------------------------------------------------------------------------------------------------- updateAction
T_BELOW = float(np.nextafter(np.float32(0.00001), np.float32(0)))       # the float just below 0.00001f
ODOMETRY = [
    (0.0, 0.0, 0.0),                         # the first call latches: no motion
    (0.00005, 0.0, 0.3),                     # trans < 0.0001 with a turn: rot1 = 0, all of the turn in rot2
    (0.1, 0.02, 0.35),                       # forward
    (0.0, -0.01, 0.35),                      # against the heading: |rot1| > pi/2, the backward branch
    (0.0, -0.01, 0.0),                       # a turn in place back to heading 0
    (0.0, -0.01, T_BELOW),                   # |trans| + |rot2| just below 0.00001f: not moved
    (0.0, -0.01, 0.0),                       # ... and back, the same size with the other sign: not moved
    (0.0, -0.01, 0.00001),                   # exactly 0.00001f: not below, moved
    (0.3, 0.2, 3.1),                         # towards +pi
    (0.35, 0.1, -3.1),                       # across +pi to -pi: the heading difference wraps
    (0.45, 0.12, 3.05),                      # and back across, backwards
    (0.45, 0.12, 3.05),                      # no motion at all
]


def test_action_update_is_the_oracles(ref, oracle):
    n = len(ODOMETRY)
    odo = np.zeros(n, POSE_DTYPE)
    for k, (x, y, th) in enumerate(ODOMETRY):
        odo[k] = (1000 + 10 * k, x, y, th, 0)
    rtr, moved = np.zeros((n, 3), np.float64), np.zeros(n, np.int32)
    ref.pm_action_seq(n, _p(odo), _p(rtr), _p(moved))
    probe = oracle_lib.OraclePF(oracle, 2)
    want_moved = []
    for k in range(n):
        probe.update_action_only(oracle.pose(odo["x"][k], odo["y"][k], odo["theta"][k], utime=int(odo["utime"][k])), np.zeros(6, np.float32))
        st, mv = (C.c_double * 3)(), C.c_int()
        oracle.lib.orc_pf_action_state(probe.h, st, C.byref(mv))
        assert rtr[k].tobytes() == np.array(list(st), np.float64).tobytes(), k
        assert moved[k] == mv.value, k
        want_moved.append(mv.value)
    # the sequence is what its comments say
    assert want_moved == [0, 1, 1, 1, 1, 0, 0, 1, 1, 1, 1, 0]
    assert rtr[1][0] == 0.0 and abs(rtr[1][2] - 0.3) < 1e-6                     # below the translation threshold: the turn is rot2
    assert rtr[3][1] < 0 and rtr[10][1] < 0 and rtr[2][1] > 0                   # the backward branch negates trans
    assert abs((rtr[9][0] + rtr[9][2] + np.pi) % (2 * np.pi) - np.pi) < 0.1     # across pi: the short way round
    stds = np.zeros(3)
    ref.pm_action_stds(_p(stds))
    assert stds.tolist() == [0.05, 0.005, 0.05]


# ---------------------------------------------------------------------------------------------------------------- applyAction
def test_apply_action_with_a_noise_table_is_the_oracles(ref, oracle):
    rng = np.random.default_rng(5)
    n = 64
    src = np.zeros((n, 3), np.float32)
    src[:, 0], src[:, 1] = rng.uniform(-3, 3, n), rng.uniform(-3, 3, n)
    src[:, 2] = rng.uniform(-3.14159, 3.14159, n)
    src[:8, 2] = [3.14, 3.1415925, -3.14, -3.1415925, 3.0, -3.0, 0.0, -0.0]      # headings that the noise takes across +-pi
    noise = np.stack([rng.normal(0.1, 0.05, n), rng.normal(0.1, 0.005, n), rng.normal(0.05, 0.05, n)], axis=1).astype(np.float32)
    noise[0], noise[1], noise[2] = (0.1, 0.1, 0.1), (0.2, 0.1, 0.1), (-0.2, 0.1, -0.1)
    noise[3], noise[5] = (-0.001, -0.1, -0.001), (-0.2, 0.05, -3.2)
    noise[4] = (0.3, 0.1, 6.4)                                                   # two steps of 2 pi back
    out = np.zeros((n, 3), np.float32)
    ref.pm_apply_noise(n, _p(src), _p(noise), _p(out))
    action = oracle.lib.orc_action_create()
    try:
        for o in ((0.0, 0.0, 0.0, 1000), (0.1, 0.0, 0.0, 2000)):                # the oracle applies nothing before it has moved
            op = oracle.pose(o[0], o[1], o[2], utime=o[3])
            moved = oracle.lib.orc_action_update(action, C.byref(op))
        assert moved
        parts = np.zeros(n, oracle_lib.PARTICLE_DTYPE)
        parts["x"], parts["y"], parts["theta"] = src[:, 0], src[:, 1], src[:, 2]
        oracle.lib.orc_action_apply_noise(action, parts.ctypes.data, n, noise.ctypes.data)
    finally:
        oracle.lib.orc_action_destroy(action)
    for j, f in enumerate(("x", "y", "theta")):
        assert out[:, j].tobytes() == parts[f].tobytes(), f
    wrapped = np.abs(src[:, 2].astype(np.float64) + noise[:, 0] + noise[:, 2]) > np.pi
    assert wrapped[:6].all() and np.all(np.abs(out[:, 2]) <= np.float32(np.pi))


# ---------------------------------------------------------------------------------------------------------------- sensor model
def _scan(ranges, thetas, times, utime):
    return types.SimpleNamespace(ranges=np.ascontiguousarray(ranges, np.float32), thetas=np.ascontiguousarray(thetas, np.float32),
                                 times=np.ascontiguousarray(times, np.int64), utime=int(utime), num_ranges=len(ranges))


def _targets(W, H):
    """Cells a scan must end in: every border cell, the ring one cell outside, far outside on all four sides, a few inside."""
    t = [(x, y) for x in range(W) for y in (0, H - 1)] + [(x, y) for y in range(H) for x in (0, W - 1)]
    t += [(x, y) for x in range(-1, W + 1) for y in (-1, H)] + [(x, y) for y in range(-1, H + 1) for x in (-1, W)]
    t += [(-1000, 3), (W + 1000, 2), (3, -1000), (2, H + 1000), (-700, -900), (W + 300, H + 500)]
    t += [(W // 4, H // 4), (1, 1), (W - 2, H - 2)]
    return t


def _scan_to(targets, origin, pose, utime):
    """A scan from `pose` whose ray k ends in the middle of cell targets[k]; ray angles in [0, 2 pi).  (A negative coordinate
    truncates towards zero: cell -1 is (-2, -1].)"""
    sx, sy = (pose[0] - origin[0]) * float(CPM), (pose[1] - origin[1]) * float(CPM)
    mid = lambda c: c + 0.5 if c >= 0 else c - 0.5
    d = np.array([(mid(tx) - sx, mid(ty) - sy) for tx, ty in targets], np.float64)
    ranges = np.hypot(d[:, 0], d[:, 1]) / float(CPM)
    thetas = np.mod(pose[2] - np.arctan2(d[:, 1], d[:, 0]), 2 * np.pi)
    times = utime - 1000 + np.arange(len(targets)) * (1000 // len(targets))
    return _scan(ranges, thetas, times, utime)


def _end_cells(scan, origin, pose):
    """The end cell of every ray from `pose` in float32, as sensor_model.cpp:29-38 forms it (no interpolation)."""
    sx = np.float32((np.float64(np.float32(pose[0])) - np.float64(np.float32(origin[0]))) * np.float64(CPM))
    sy = np.float32((np.float64(np.float32(pose[1])) - np.float64(np.float32(origin[1]))) * np.float64(CPM))
    th = np.float32(pose[2]) - scan.thetas
    ex = (scan.ranges * np.cos(th.astype(np.float64)).astype(np.float32) * CPM + sx).astype(np.float32)
    ey = (scan.ranges * np.sin(th.astype(np.float64)).astype(np.float32) * CPM + sy).astype(np.float32)
    return np.trunc(ex).astype(np.int64), np.trunc(ey).astype(np.int64)


def _header_likelihood(ref, cells, origin, part, scan):
    keep = scan.ranges > np.float32(0.15)                   # the host keeps these rays (moving_laser_scan.cpp:24)
    ranges, thetas, times = (np.ascontiguousarray(a[keep]) for a in (scan.ranges, scan.thetas, scan.times))
    frame = np.array([origin[0], origin[1], MPC, CPM], np.float32)
    pb = np.array([part["p_x"], part["p_y"], part["p_theta"]], np.float32)
    pe = np.array([part["x"], part["y"], part["theta"]], np.float32)
    c = np.ascontiguousarray(cells)
    return ref.pm_likelihood_half_units(c.shape[1], c.shape[0], _p(frame), _p(c), _p(pb), int(part["p_utime"]), _p(pe), int(part["utime"]),
                                        len(ranges), _p(ranges), _p(thetas), _p(times))


def _oracle_likelihood(oracle, cells, origin, part, scan):
    l, g = oracle.lidar(scan), oracle.grid(cells, MPC, CPM, origin)
    raw = np.zeros(1, np.float64)
    p = np.array([part], oracle_lib.PARTICLE_DTYPE)
    oracle.lib.orc_likelihood(p.ctypes.data, 1, C.byref(l), C.byref(g), raw.ctypes.data)
    return raw[0]


# (W, H), origin, the pose the scan is aimed from: outside the small grid (every cell is more than 0.15 m away), inside the large one
SENSOR_CASES = {"8x6": ((8, 6), (-0.3, 0.7), (-0.3 - 4.5 * 0.05, 0.7 - 4.5 * 0.05, 0.4)),
                "40x40": ((40, 40), (-1.0, -1.0), (-1.0 + 20.5 * 0.05, -1.0 + 20.5 * 0.05, 3.1))}


@pytest.mark.parametrize("name", list(SENSOR_CASES))
def test_plain_sensor_model_is_twice_the_oracles_likelihood(ref, oracle, name):
    (W, H), origin, pose = SENSOR_CASES[name]
    rng = np.random.default_rng(W)
    cells = rng.integers(-30, 40, (H, W)).astype(np.int8)
    cells[0, 0], cells[H - 1, W - 1], cells[0, W - 1], cells[H - 1, 0] = 127, -128, 5, 1
    targets = _targets(W, H)
    scan = _scan_to(targets, origin, pose, 5000)
    assert np.all(scan.ranges > np.float32(0.15))
    # the scan reaches what it is meant to reach
    ex, ey = _end_cells(scan, origin, pose)
    ends = set(zip(ex.tolist(), ey.tolist()))
    assert {(x, y) for x in range(W) for y in (0, H - 1)} <= ends and {(x, y) for y in range(H) for x in (0, W - 1)} <= ends
    assert {(-1, 2), (W, 2), (2, -1), (2, H)} <= ends
    assert ex.min() < -500 and ex.max() >= W + 500 and ey.min() < -500 and ey.max() >= H + 500
    parts = np.zeros(4, oracle_lib.PARTICLE_DTYPE)
    # 0: the pose itself, equal utimes.  1: the same with the start on the other side of a cell border.  2, 3: interpolated -- the
    # parent pose elsewhere and at another heading (3: across +-pi), the rays' stamps between the two utimes
    parts["x"], parts["y"], parts["theta"] = pose[0], pose[1], pose[2]
    parts["utime"], parts["p_utime"] = 5000, 5000
    parts["p_x"], parts["p_y"], parts["p_theta"] = parts["x"], parts["y"], parts["theta"]
    parts["x"][1] += 0.03; parts["p_x"][1] = parts["x"][1]
    parts["p_utime"][2:] = 4000
    parts["p_x"][2:], parts["p_y"][2:] = parts["x"][2:] - 0.12, parts["y"][2:] + 0.07
    parts["p_theta"][2], parts["p_theta"][3] = pose[2] - 0.5, -3.0
    total = 0
    for k in range(4):
        want = _oracle_likelihood(oracle, cells, origin, parts[k], scan)
        got = _header_likelihood(ref, cells, origin, parts[k], scan)
        assert got == 2.0 * want, (name, k, got, want)
        total += got
    assert total > 0
    # a scan with rays the host drops (range <= 0.15f) among the others: the oracle drops them too
    short = _scan(np.concatenate([scan.ranges[:5], np.float32([0.15, 0.1, 0.0])]), np.concatenate([scan.thetas[:5], np.float32([0.1, 0.2, 0.3])]),
                  np.concatenate([scan.times[:5], [4990, 4995, 5000]]), 5000)
    assert _header_likelihood(ref, cells, origin, parts[2], short) == 2.0 * _oracle_likelihood(oracle, cells, origin, parts[2], short)


def test_score_units(ref):
    assert [ref.pm_score_units(v) for v in (-1, 0, 1, SCORE_MAX)] == [2, 2, 1000, 1000 * SCORE_MAX]


# ---------------------------------------------------------------------------------------------------------------- low-variance draw
def test_resampling_offset_and_draw(ref, oracle):
    for M in (1, 7, 300):
        assert ref.pm_resample_offset(0, 1.0 / M) == 0.0
        assert ref.pm_resample_offset(rrm.RAND_MAX, 1.0 / M) == 1.0 / M
        assert ref.pm_resample_offset(12345, 1.0 / M) == (12345.0 / rrm.RAND_MAX) * (1.0 / M)
    units = np.array([2, 9000, 2, 31000, 1000, 2, 17000], np.uint64)
    for rv in (0, 1, 12345, rrm.RAND_MAX // 2, rrm.RAND_MAX - 1, rrm.RAND_MAX):
        idx = np.zeros(7, np.int32)
        ref.pm_resample(7, _p(units), rv, _p(idx))
        assert np.array_equal(idx, rrm.oracle_indices(oracle, units, rv)), rv
        assert np.array_equal(idx, rrm.integer_rule(units, rv)), rv
    assert len(set(idx.tolist())) > 2
    # four equal weights at rand() = 0: every target but the first lies ON a prefix (T_m = 2 m = prefix_(m - 1), exactly, in the
    # oracle's doubles too), which the non-strict comparison takes
    equal, idx4 = np.full(4, 2, np.uint64), np.zeros(4, np.int32)
    ref.pm_resample(4, _p(equal), 0, _p(idx4))
    assert idx4.tolist() == [0, 0, 1, 2] == rrm.oracle_indices(oracle, equal, 0).tolist() == rrm.integer_rule(equal, 0).tolist()


def test_exported_particle_has_zeroed_padding(ref):
    raw = np.full(56, 0xa5, np.uint8)
    pose, parent = np.float32([1.5, -2.5, 0.25]), np.float32([1.25, -2.0, -0.5])
    ref.pm_particle(_p(raw), _p(pose), 123456789012, _p(parent), 98765, 0.375)
    p = raw.view(oracle_lib.PARTICLE_DTYPE)[0]
    assert (p["utime"], p["x"], p["y"], p["theta"]) == (123456789012, pose[0], pose[1], pose[2])
    assert (p["p_utime"], p["p_x"], p["p_y"], p["p_theta"], p["weight"]) == (98765, parent[0], parent[1], parent[2], 0.375)
    assert raw[20:24].tolist() == [0] * 4 and raw[44:48].tolist() == [0] * 4
