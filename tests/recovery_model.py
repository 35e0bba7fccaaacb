"""numpy model of the kidnapped-robot recovery (augmented MCL, bl_pf_set_recovery), bit for bit: the tracker's fold in float64, the
injected fraction p and threshold t, the per-particle decision words, and the injected samples (global_init_model's sampler keyed by
the update number u and the recovery tag).  Also the reference's low-variance resampling (particle_filter.cpp:84-103) and the
calibrated kidnap scenario on obstacle_slam_10mx10m_5cm (tests/test_recovery_model_cpu.py measures it on the CPU filter; the GPU tests
reuse the constants)."""
import math

import numpy as np

import global_init_model as gm

RC_CTR = 0x72637679                         # Philox counter word of the recovery: (m, u, RC_CTR, 0 / 1) sample, (m, u, RC_CTR, 2) decision
RAND_MAX = 2147483647

# ---- defaults (ParticleFilter.setRecovery, botlab_hip.h): AMCL's averaging rates, ratio / max_fraction calibrated below
ALPHA_SLOW, ALPHA_FAST = 0.001, 0.1
RATIO, MAX_FRACTION = 0.9, 0.1

# ---- the calibrated kidnap scenario (measured by test_kidnap_calibration on the CPU filter)
KID_MAP = gm.CAL_MAP
KID_START = gm.CAL_START                    # truth start; the filter starts there (init_at_pose)
KID_TRAJ = gm.CAL_TRAJ
KID_K0 = 15                                 # moved updates tracked before the kidnap
KID_TO = (0.2, 2.4, 3.1)                     # where the robot is set down (x, y, theta): the truth from update K0 + 1 on is the rest of
                                            # the trajectory moved rigidly so that its pose K0 lands here; odometry carries on unaware
KID_KR = 75                                 # moved updates after the kidnap within which recovery must have re-localised
KID_SEED = 77                               # recovery seed of the calibration run
KID_N = 20_000                              # particles of the calibration run
KID_LOST = 0.5                              # without recovery the estimate is still farther than this (metres) after KID_KR updates:
                                            # relaxed from 1 m -- the trajectory carries the wrong cloud back towards the truth (0.64 m
                                            # at the end); the near-truth weight (< 0.01) is the sharper check


def kidnap_truth(k0=KID_K0, kr=KID_KR, start=KID_START, to=KID_TO, traj=KID_TRAJ):
    """(motion, truth, begin): `motion` is the trajectory the odometry sees (a square from `start`), `truth` the true poses --
    motion[k] for k <= k0, then motion[k] moved rigidly so that motion[k0] lands on `to`.  Scan k sweeps from begin[k] to truth[k]:
    begin[k] = truth[k - 1], except that the scan right after the kidnap starts at `to` (the robot is carried between two scans)."""
    from botlab_amd import synth
    motion = synth.square_trajectory(start, k0 + kr, **traj)
    a = motion[k0]
    dth = to[2] - a[2]
    c, s = math.cos(dth), math.sin(dth)
    truth = list(motion[:k0 + 1])
    for p in motion[k0 + 1:]:
        dx, dy = p[0] - a[0], p[1] - a[1]
        th = p[2] + dth
        truth.append(np.array([to[0] + c * dx - s * dy, to[1] + s * dx + c * dy, math.atan2(math.sin(th), math.cos(th))]))
    begin = [None] + [truth[k - 1] for k in range(1, len(truth))]
    begin[k0 + 1] = np.array(to, dtype=np.float64)
    return motion, truth, begin


class Tracker:
    """The device tracker (k_pf_recovery_fold): plain IEEE double, no contraction -- Python floats reproduce it."""

    def __init__(self):
        self.w_slow = self.w_fast = self.w_avg = self.p = 0.0
        self.primed = False
        self.updates = 0
        self.t = 0

    def step(self, u, S, N, fold, alpha_slow=ALPHA_SLOW, alpha_fast=ALPHA_FAST, ratio=RATIO, max_fraction=MAX_FRACTION):
        """Start of moved update u: fold the posterior of S weight units over N particles (fold: a sensor update produced it)."""
        if fold:
            w_avg = (float(S) * 0.0005) / float(N)
            self.w_avg = w_avg
            if not self.primed:
                self.w_slow = self.w_fast = w_avg
                self.primed = True
            else:
                self.w_slow = self.w_slow + alpha_slow * (w_avg - self.w_slow)
                self.w_fast = self.w_fast + alpha_fast * (w_avg - self.w_fast)
        self.p = injected_fraction(self.primed, self.w_slow, self.w_fast, ratio, max_fraction)
        self.t = threshold(self.p)
        self.updates = u
        return self.t

    def as_tuple(self):
        return (self.w_slow, self.w_fast, self.w_avg, self.p, self.updates, int(self.primed))


def folds_next(pose_utime):
    """Whether the posterior of an update is folded at the next one: only when the update did not interpolate its scan, i.e. its
    particles carried pose utime 0 (every update after the first; the first too after an initialisation or upload at utime 0)."""
    return pose_utime == 0


def injected_fraction(primed, w_slow, w_fast, ratio, max_fraction):
    if primed and w_fast < ratio * w_slow:
        return min(max_fraction, 1.0 - w_fast / (ratio * w_slow))
    return 0.0


def threshold(p):
    """t = p >= 1 ? 2^32 : floor(p * 2^32) (p * 2^32 is exact in double)."""
    return 1 << 32 if p >= 1.0 else int(math.floor(p * 4294967296.0))


def decision_words(seed, u, idx):
    """Word 0 of Philox4x32-10((m, u, RC_CTR, 2), seed) for the global particle indices idx."""
    m = np.asarray(idx, dtype=np.uint64)
    return gm.philox4x32(m, u, RC_CTR, 2, seed & gm.MASK32, (seed >> 32) & gm.MASK32)[0]


def injected_mask(seed, u, t, n):
    """Which of particles 0 .. n-1 update u injects."""
    if t == 0:
        return np.zeros(n, bool)
    return decision_words(seed, u, np.arange(n, dtype=np.uint64)) < np.uint64(t) if t < (1 << 32) else np.ones(n, bool)


def sample(seed, elig, width, origin, mpc, idx, u):
    """Injected priors (x, y, theta float32) of the particles idx at update u: k_pf_init_uniform's formula with counter words
    (m, u, RC_CTR, 0 / 1) and the recovery seed."""
    m = np.asarray(idx, dtype=np.uint64)
    k0, k1 = seed & gm.MASK32, (seed >> 32) & gm.MASK32
    a0, a1, a2, a3 = gm.philox4x32(m, u, RC_CTR, 0, k0, k1)
    b0, _, _, _ = gm.philox4x32(m, u, RC_CTR, 1, k0, k1)
    F = np.uint64(len(elig))
    r = (a0 * F + ((a1 * F) >> np.uint64(32))) >> np.uint64(32)
    cell = elig[r.astype(np.int64)]
    cx, cy = cell % np.uint64(width), cell // np.uint64(width)
    s24 = 2.0 ** -24
    fx = (a2 >> np.uint64(8)).astype(np.float64) * s24
    fy = (a3 >> np.uint64(8)).astype(np.float64) * s24
    ft = (b0 >> np.uint64(8)).astype(np.float64) * s24
    x = (np.float64(np.float32(origin[0])) + (cx.astype(np.float64) + fx) * np.float64(np.float32(mpc))).astype(np.float32)
    y = (np.float64(np.float32(origin[1])) + (cy.astype(np.float64) + fy) * np.float64(np.float32(mpc))).astype(np.float32)
    th = gm.wrap_to_pi(((2.0 * ft - 1.0) * math.pi).astype(np.float32))
    return x, y, th


def resample(weights, rand_value):
    """The reference's low-variance resampling (particle_filter.cpp:84-103): c = running sum of the weights (np.cumsum adds in
    sequence, as the loop does), U_m = r + m * M_inv, source = first i with U_m <= c_i (clamped to N - 1)."""
    w = np.asarray(weights, dtype=np.float64)
    n = len(w)
    M_inv = 1.0 / n
    r = (float(rand_value) / float(RAND_MAX)) * M_inv
    U = r + np.arange(n, dtype=np.float64) * M_inv
    c = np.cumsum(w)
    return np.minimum(np.searchsorted(c, U, side="left"), n - 1)


def units_of(raw):
    """Weight units of the reference's raw likelihoods: max(likelihood, 0.001) in units of 0.0005."""
    raw = np.asarray(raw, dtype=np.float64)
    return np.where(raw > 0, np.rint(raw * 2000.0), 2.0).astype(np.int64)
