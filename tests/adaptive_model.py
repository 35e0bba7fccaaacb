"""numpy model of the adaptive particle count (bl_pf_set_adaptive, KLD-sampling): the bin count of a resampled set, the KLD bound,
k_sat and next, bit for bit; resampling with M != N by the reference's sequential cumulative and by the library's integer prefix; and a
CPU filter with an adaptive count built from the reference's per-particle entry points (action noise, likelihood,
estimatePosteriorPose), which tests/test_adaptive_model_cpu.py calibrates the defaults on."""
import collections
import ctypes as C
import math

import numpy as np

import recovery_model as rm

RAND_MAX = rm.RAND_MAX
IDX_LIM = 1 << 20                           # bin indices are clamped to [-2^20, 2^20 - 1] (NaN: -2^20), botlab_hip.h


def bin_index(v, b):
    """clamp(floor(v / b)) + 2^20 in [0, 2^21 - 1], computed in double from the float coordinates."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        q = np.floor(np.asarray(v, dtype=np.float32).astype(np.float64) / np.float64(b))
    q = np.where(np.isnan(q), -IDX_LIM, q)
    q = np.clip(q, -IDX_LIM, IDX_LIM - 1)
    return (q + IDX_LIM).astype(np.int64)


def bin_keys(x, y, th, bin_xy, bin_theta):
    return (bin_index(x, bin_xy) << 42) | (bin_index(y, bin_xy) << 21) | bin_index(th, bin_theta)


def count_bins(x, y, th, bin_xy, bin_theta):
    """k: distinct (floor(x / bin_xy), floor(y / bin_xy), floor(theta / bin_theta)) triples."""
    if len(x) == 0:
        return 0
    return int(len(np.unique(bin_keys(x, y, th, bin_xy, bin_theta))))


def bound(k, epsilon, z):
    """n(k) for k >= 2, in plain IEEE double as the library forms it."""
    km1 = float(k - 1)
    b = 2.0 / (9.0 * km1)
    c = 1.0 - b + math.sqrt(b) * z
    return math.ceil(km1 / (2.0 * epsilon) * c * c * c)


def bounds(ks, epsilon, z):
    """bound() over an array of k >= 2 (numpy's float64 operations round as Python's)."""
    km1 = np.asarray(ks, dtype=np.float64) - 1.0
    b = 2.0 / (9.0 * km1)
    c = 1.0 - b + np.sqrt(b) * z
    return np.ceil(km1 / (2.0 * epsilon) * c * c * c)


def k_sat(cap, epsilon, z):
    """The smallest k in [2, cap] with n(k) >= cap, else cap + 1."""
    ks = np.arange(2, cap + 1, dtype=np.int64)
    hit = np.flatnonzero(bounds(ks, epsilon, z) >= cap)
    return int(ks[hit[0]]) if len(hit) else cap + 1


def next_count(k, min_particles, epsilon, z, cap):
    n = min_particles if k <= 1 else bound(k, epsilon, z)
    return int(min(cap, max(min_particles, n)))


def resample_reference(weights, rand_value, M):
    """The reference's low-variance resampling (particle_filter.cpp:84-103) with M outputs: c = sequential running sum of the
    weights, U_m = r + m / M, r = rand / RAND_MAX / M, source = first i with U_m <= c_i (clamped to N - 1)."""
    w = np.asarray(weights, dtype=np.float64)
    M_inv = 1.0 / M
    r = (float(rand_value) / float(RAND_MAX)) * M_inv
    U = r + np.arange(M, dtype=np.float64) * M_inv
    return np.minimum(np.searchsorted(np.cumsum(w), U, side="left"), len(w) - 1)


def resample_integer(units, rand_value, M):
    """The library's integer-prefix rule with M outputs: T_m = (r + m / M) * S, first i with T_m <= prefix_i (clamped)."""
    u = np.asarray(units, dtype=np.uint64)
    prefix = np.cumsum(u, dtype=np.uint64)
    S = float(prefix[-1])
    M_inv = 1.0 / M
    r = (float(rand_value) / float(RAND_MAX)) * M_inv
    T = (r + np.arange(M, dtype=np.float64) * M_inv) * S
    return np.minimum(np.searchsorted(prefix.astype(np.float64), T, side="left"), len(u) - 1)


Params = collections.namedtuple("Params", "min_particles epsilon z bin_xy bin_theta")


class CountModel:
    """active / next / bins / k_sat of a filter of capacity cap, driven by the parents of every resampling update."""

    def __init__(self, cap, p):
        self.cap, self.p = cap, p
        self.ksat = k_sat(cap, p.epsilon, p.z)
        self.active = self.next = cap
        self.bins = 0

    def counted(self, parent_x, parent_y, parent_th):
        k = count_bins(parent_x, parent_y, parent_th, self.p.bin_xy, self.p.bin_theta)
        self.active = len(parent_x)
        self.bins = min(k, self.ksat)
        self.next = next_count(self.bins, self.p.min_particles, self.p.epsilon, self.p.z, self.cap)
        return self.bins


class AdaptiveCPUFilter:
    """The reference's particle filter with an adaptive count: the reference's ActionModel (its odometry step and the noise of
    apply_with_noise, drawn here from rot1 / trans / rot2 and the model's standard deviations), its likelihood and its
    estimatePosteriorPose, with numpy's resampling of M = next particles in between (resample_reference) and the count above."""

    STDS = (0.05, 0.005, 0.05)              # ActionModel::update's rot1Std, transStd, rot2Std

    def __init__(self, oracle, parts, params, rng, adaptive=True):
        import oracle_lib
        self.o, self.rng, self.adaptive = oracle, rng, adaptive
        self.post = np.ascontiguousarray(parts).copy()
        self.cap = len(parts)
        self.model = CountModel(self.cap, params)
        self.action = oracle.lib.orc_action_create()
        self.probe = oracle_lib.OraclePF(oracle, 2)      # a twin ActionModel whose rot1 / trans / rot2 we can read
        self.pose = None

    def __del__(self):
        if getattr(self, "action", None):
            self.o.lib.orc_action_destroy(self.action)
            self.action = None

    def update(self, odom, scan, cells, mpc, cpm, origin, rand_value):
        """One updateFilter; returns the pose estimate or None when the robot did not move."""
        op = self.o.pose(odom[0], odom[1], odom[2], utime=scan.utime)
        moved = bool(self.o.lib.orc_action_update(self.action, C.byref(op)))
        self.probe.update_action_only(op, np.zeros(6, np.float32))
        if not moved:
            return None
        st = (C.c_double * 3)()
        mv = C.c_int()
        self.o.lib.orc_pf_action_state(self.probe.h, st, C.byref(mv))
        M = self.model.next if self.adaptive else self.cap
        idx = resample_reference(self.post["weight"], rand_value, M)
        prior = self.post[idx].copy()
        noise = np.empty((M, 3), np.float32)
        for j in range(3):
            noise[:, j] = (st[j] + self.STDS[j] * self.rng.standard_normal(M)).astype(np.float32)
        self.o.lib.orc_action_apply_noise(self.action, prior.ctypes.data, M, np.ascontiguousarray(noise).ctypes.data)
        raw = np.zeros(M, np.float64)
        g, l = self.o.grid(cells, mpc, cpm, origin), self.o.lidar(scan)
        self.o.lib.orc_likelihood(prior.ctypes.data, M, C.byref(l), C.byref(g), raw.ctypes.data)
        w = np.maximum(raw, 0.001)
        prior["weight"] = w / w.sum()
        self.post = prior
        out = type(op)()
        self.o.lib.orc_estimate_pose(self.post.ctypes.data, M, C.byref(out))
        self.pose = out
        if self.adaptive:
            self.model.counted(self.post["p_x"], self.post["p_y"], self.post["p_theta"])
        return out
