"""The numpy model of the adaptive particle count (tests/adaptive_model.py): the bound and k_sat with hand-worked values, the exact bin
count on adversarial clouds, resampling with M != N against the CPU reference filter's sequential cumulative, and the calibration of
the defaults on the global-localization scenario of tests/global_init_model.py."""
import math

import numpy as np
import pytest

import adaptive_model as am
import global_init_model as gm
import helpers
from botlab_amd import synth
from botlab_amd.host import (ADAPTIVE_BIN_THETA, ADAPTIVE_BIN_XY, ADAPTIVE_EPSILON, ADAPTIVE_MIN_PARTICLES, ADAPTIVE_Z,
                             PARTICLE_DTYPE)

CAL_CAP = 100_000


def test_defaults():
    assert ADAPTIVE_EPSILON == 0.01 and ADAPTIVE_Z == 2.326 and ADAPTIVE_MIN_PARTICLES >= 200
    assert ADAPTIVE_BIN_XY < 0.5                                   # finer than AMCL's: a 10 m map of 5 cm cells
    assert ADAPTIVE_BIN_THETA == math.radians(10.0)


def test_bound_hand_worked():
    # k = 2: b = 2/9, c = 1 - 2/9 + sqrt(2/9) z;  n = ceil(1 / (2 eps) c^3)
    z, eps = 2.326, 0.01
    b = 2.0 / 9.0
    c = 1.0 - b + math.sqrt(b) * z
    assert am.bound(2, eps, z) == math.ceil(50.0 * c ** 3)
    assert am.bound(2, eps, z) == 330                              # c = 1.87426..., 50 c^3 = 329.19...
    # k = 100: b = 2/891, c = 1.10794..., n = ceil(99 / 0.02 * c^3) = 6733
    assert am.bound(100, eps, z) == 6733
    # the count floor and the capacity
    assert am.next_count(0, 200, eps, z, 100_000) == 200 and am.next_count(1, 200, eps, z, 100_000) == 200
    assert am.next_count(2, 200, eps, z, 100_000) == 330
    assert am.next_count(2, 500, eps, z, 100_000) == 500
    assert am.next_count(10 ** 6, 200, eps, z, 100_000) == 100_000
    # bounds() (the array form) agrees with bound() bit for bit
    ks = np.arange(2, 5000)
    assert np.array_equal(am.bounds(ks, eps, z), [am.bound(int(k), eps, z) for k in ks])


def test_k_sat():
    z, eps = 2.326, 0.01
    for cap in (200, 1000, 100_000, 1_000_000):
        k = am.k_sat(cap, eps, z)
        assert am.bound(k, eps, z) >= cap and (k == 2 or am.bound(k - 1, eps, z) < cap), cap
    assert am.k_sat(100_000, eps, z) == 1857
    assert 15_000 < am.k_sat(1_000_000, eps, z) < 25_000           # "roughly 2 10^4"
    assert am.k_sat(10, 1e6, z) == 11                               # no k <= cap reaches the capacity: cap + 1


def _count_ref(x, y, th, bxy, bth):
    t = set()
    for a, b, c in zip(np.float32(x).astype(float), np.float32(y).astype(float), np.float32(th).astype(float)):
        t.add((math.floor(a / bxy), math.floor(b / bxy), math.floor(c / bth)))
    return len(t)


def test_count_adversarial():
    bxy, bth = 0.1, math.radians(10.0)
    pi = np.float32(math.pi)
    # a single bin
    assert am.count_bins(np.full(1000, 0.01, np.float32), np.full(1000, 0.02, np.float32), np.zeros(1000, np.float32), bxy, bth) == 1
    # poses exactly on bin edges and just below them (as floats: 0.3 in float is not 3 * 0.1 in double)
    edges = np.float32(np.arange(-20, 21) * 0.1)
    below = np.nextafter(edges, np.float32(-np.inf))
    x = np.concatenate([edges, below]); y = np.zeros_like(x); th = np.zeros_like(x)
    assert am.count_bins(x, y, th, bxy, bth) == _count_ref(x, y, th, bxy, bth)
    assert am.count_bins(x, y, th, 0.5, bth) == _count_ref(x, y, th, 0.5, bth)
    # theta = +-pi and its neighbours: distinct bins at both ends
    th = np.array([-pi, pi, np.nextafter(-pi, 0), np.nextafter(pi, 0), 0.0, -0.0], np.float32)
    z0 = np.zeros_like(th)
    assert am.count_bins(z0, z0, th, bxy, bth) == _count_ref(z0, z0, th, bxy, bth) == 5
    # negative coordinates (floor, not truncation) and every particle in a bin of its own
    rng = np.random.default_rng(1)
    x = (rng.permutation(5000) - 2500).astype(np.float32) * np.float32(0.1) + np.float32(0.05)
    y = np.float32(-3.0) + rng.random(5000).astype(np.float32)
    th = (rng.random(5000) * 2 * math.pi - math.pi).astype(np.float32)
    assert am.count_bins(x, y, th, bxy, bth) == 5000 == _count_ref(x, y, th, bxy, bth)
    # random clouds at several scales
    for s in (0.05, 1.0, 30.0):
        x, y = (rng.normal(0, s, 20_000).astype(np.float32) for _ in range(2))
        th = (rng.random(20_000) * 2 * math.pi - math.pi).astype(np.float32)
        assert am.count_bins(x, y, th, bxy, bth) == _count_ref(x, y, th, bxy, bth)
    # the clamp: far coordinates and NaN share the end bins
    big = np.array([1e30, 2e30, -1e30, np.nan, -np.inf], np.float32)
    z0 = np.zeros_like(big)
    assert am.count_bins(big, z0, z0, bxy, bth) == 2


def test_resample_m_equals_reference(oracle):
    """resample_reference with M != N equals the reference's own loop (orc_resample_indices runs it with M = N, so compare on the
    sequential rule directly: an explicit loop of particle_filter.cpp:84-103 with M outputs)."""
    rng = np.random.default_rng(5)
    for n, M in ((2, 7), (1000, 200), (1000, 4097), (4097, 1000), (50, 50)):
        w = rng.random(n) ** 4
        w /= w.sum()
        for rv in (0, 1, 12345, am.RAND_MAX // 2, am.RAND_MAX):
            M_inv = 1.0 / M
            r = (float(rv) / float(am.RAND_MAX)) * M_inv
            c, i, want = w[0], 0, []
            for m in range(M):
                U = r + m * M_inv
                while U > c and i < n - 1:
                    i += 1
                    c += w[i]
                want.append(i)
            assert np.array_equal(am.resample_reference(w, rv, M), want), (n, M, rv)
    # with M = N it is the reference filter's resample (through the oracle)
    import oracle_lib
    parts = np.zeros(3000, dtype=PARTICLE_DTYPE)
    w = rng.random(3000) ** 3
    parts["weight"] = w / w.sum()
    idx = np.zeros(3000, np.int32)
    oracle.lib.orc_resample_indices(parts.ctypes.data, 3000, 777, idx.ctypes.data)
    assert np.array_equal(am.resample_reference(parts["weight"], 777, 3000), idx)


def test_resample_integer_rule():
    """The integer-prefix rule with M != N: T_m = U_m * S against the exact prefix."""
    units = np.array([2, 2, 6, 2, 40, 2], np.uint64)
    idx = am.resample_integer(units, 0, 3)                    # T = 0, 18, 36 of S = 54: prefix 2 4 10 12 52 54
    assert list(idx) == [0, 4, 4]
    idx = am.resample_integer(units, am.RAND_MAX, 12)         # r = 1/12: T = (1 + m) * 4.5
    assert list(idx) == [2, 2, 4, 4, 4, 4, 4, 4, 4, 4, 4, 5]


def _calibration_run(oracle, maps, cap, params, adaptive=True):
    m = maps[gm.CAL_MAP]
    cells, origin, mpc, cpm = m["cells"], m["origin"], m["mpc"], helpers.CPM_DEFAULT
    truth = np.where(cells > 0, 127, -127).astype(np.int8)
    poses = synth.square_trajectory(gm.CAL_START, gm.CAL_STEPS, **gm.CAL_TRAJ)
    odo = synth.odometry_from_truth(poses, np.random.default_rng(3))
    x, y, th = gm.model_cloud(gm.CAL_SEED, cells, origin, mpc, cap)
    f = am.AdaptiveCPUFilter(oracle, gm.as_particles(x, y, th, 1000, PARTICLE_DTYPE), params, np.random.default_rng(11),
                             adaptive=adaptive)
    out = []
    for k in range(1, len(poses)):
        scan = synth.raycast_scan(truth, origin, 0.05, poses[k - 1], poses[k], 1000 + 100000 * k)
        p = f.update(odo[k], scan, cells, mpc, cpm, origin, 1000 + k)
        if p is None:
            continue
        out.append((len(f.post), math.hypot(p.x - poses[k][0], p.y - poses[k][1]), gm.near_weight(f.post, poses[k])))
    return out


def test_calibration(oracle, maps):
    """From a uniform cloud at capacity 100 000 on the global-localization scenario, with the default parameters (0.1 m / 10 degree
    bins, epsilon 0.01, z 2.326, at least 200 particles).  Measured: the count stays at k_sat = 1857 bins (all 100 000 particles) for
    14 updates, then falls with the spread; the weight near the truth passes 0.9 at update 37 and the estimate is within 0.1 m from
    update 39 on (0.012 m at CAL_K = 50); the last updates run 2 150 - 2 500 particles (about 2 % of the capacity).  AMCL's 0.5 m
    bins end at about 1 100 particles, 5 cm / 5 degree bins at 6 500 - 7 200 and over 10 % for a few updates."""
    p = am.Params(ADAPTIVE_MIN_PARTICLES, ADAPTIVE_EPSILON, ADAPTIVE_Z, ADAPTIVE_BIN_XY, ADAPTIVE_BIN_THETA)
    out = _calibration_run(oracle, maps, CAL_CAP, p)
    assert len(out) >= gm.CAL_K
    first = next(i for i, (_, e, w) in enumerate(out) if w >= gm.CAL_NEAR_WEIGHT and e <= gm.CAL_EST_TOL)
    assert first < gm.CAL_K                                        # converges within CAL_K updates
    assert out[gm.CAL_K - 1][2] >= gm.CAL_NEAR_WEIGHT
    assert all(e <= gm.CAL_EST_TOL for _, e, _ in out[first:])     # and stays within CAL_EST_TOL to the end
    assert all(n <= CAL_CAP // 10 for n, _, _ in out[first:])      # at most 10 % of the capacity once converged
    assert out[0][0] == CAL_CAP
