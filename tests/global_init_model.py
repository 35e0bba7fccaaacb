"""numpy model of bl_pf_init_uniform (the global-localization sampler, bl_mcl.hip k_pf_init_uniform) and of bl_pf_spread, bit for
bit: Philox4x32-10 vectorised over particles, the eligible-cell list in row-major order, the rank / offset / heading formulas.

Also the calibrated scenario of global localization on obstacle_slam_10mx10m_5cm (tests/test_global_init_model_cpu.py measures
it on the CPU filter; the GPU tests reuse the constants)."""
import math

import numpy as np

MASK32 = 0xFFFFFFFF
GL_CTR1 = 0xFFFFFFFE
GL_CTR2 = 0x676C6F62
PI_F = np.float32(math.pi)                  # (float)M_PI, the float just above pi

# ---- the calibrated scenario (measured by test_global_init_calibration on the CPU filter)
CAL_MAP = "obstacle_slam_10mx10m_5cm"
CAL_START = (-0.75, 0.2, 0.0)               # truth start (x, y, theta); the filter is not told
CAL_STEPS = 60                              # truth poses after the start: square_trajectory(CAL_START, CAL_STEPS, **CAL_TRAJ)
CAL_TRAJ = dict(step_len=0.03, turn=0.05, side=0.8)
CAL_N = 20_000                              # particles of the calibration run
CAL_SEED = 2024                             # sampler seed of the calibration run
CAL_K = 50                                  # moved updates within which the cloud has converged
CAL_NEAR_POS, CAL_NEAR_THETA = 0.3, 0.3     # "near the truth": within 0.3 m and 0.3 rad
CAL_NEAR_WEIGHT = 0.9                       # weight near the truth after CAL_K updates, at least
CAL_EST_TOL = 0.1                           # estimate within 0.1 m of the truth after CAL_K updates
# steady spread of a filter started AT the truth in the same scenario (bounds of what test_steady_spread_from_true_pose measures:
# at most 0.025 m / 0.100 rad over the run), and the driver's default convergence thresholds, at least twice those
CAL_STEADY_POS, CAL_STEADY_THETA = 0.03, 0.11
DRIVER_POS_TOL, DRIVER_HEADING_TOL = 0.2, 0.3  # OccupancyGridSLAMT defaults (include/botlab/slam_driver.hpp)


def philox4x32(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (bl_math.h bl_philox4x32) over arrays of counters; returns four uint64 arrays holding uint32 values."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & np.uint64(MASK32) for c in (c0, c1, c2, c3))
    c0, c1, c2, c3 = np.broadcast_arrays(c0, c1, c2, c3)
    k0, k1 = int(k0) & MASK32, int(k1) & MASK32
    m32, s32 = np.uint64(MASK32), np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        n0 = (p1 >> s32) ^ c1 ^ np.uint64(k0)
        n1 = p1 & m32
        n2 = (p0 >> s32) ^ c3 ^ np.uint64(k1)
        n3 = p0 & m32
        c0, c1, c2, c3 = n0, n1, n2, n3
        k0 = (k0 + 0x9E3779B9) & MASK32
        k1 = (k1 + 0xBB67AE85) & MASK32
    return c0, c1, c2, c3


def eligible_cells(cells, dist=None, min_dist=0.0):
    """Row-major indices of the eligible cells: log-odds < 0 and, with a distance grid, distance > min_dist (float compare)."""
    ok = np.asarray(cells).reshape(-1) < 0
    if dist is not None:
        ok &= np.asarray(dist, dtype=np.float32).reshape(-1) > np.float32(min_dist)
    return np.flatnonzero(ok).astype(np.uint64)


def wrap_to_pi(th):
    """bl_wrap_to_pi for angles within one 2 pi step of the range."""
    th = np.asarray(th, dtype=np.float32).copy()
    lo, hi = th <= -PI_F, th >= PI_F
    th[lo] = (th[lo].astype(np.float64) + 2.0 * math.pi).astype(np.float32)
    th[hi] = (th[hi].astype(np.float64) - 2.0 * math.pi).astype(np.float32)
    return th


def sample(seed, elig, width, origin, mpc, idx):
    """Poses (x, y, theta float32) of the particles with global indices idx."""
    m = np.asarray(idx, dtype=np.uint64)
    k0, k1 = seed & MASK32, (seed >> 32) & MASK32
    a0, a1, a2, a3 = philox4x32(m, GL_CTR1, GL_CTR2, 0, k0, k1)
    b0, _, _, _ = philox4x32(m, GL_CTR1, GL_CTR2, 1, k0, k1)
    F = np.uint64(len(elig))
    # hi64(((a0 << 32) | a1) * F) without 128-bit integers: (a0 F + ((a1 F) >> 32)) >> 32  (F < 2^31)
    r = (a0 * F + ((a1 * F) >> np.uint64(32))) >> np.uint64(32)
    cell = elig[r.astype(np.int64)]
    cx, cy = cell % np.uint64(width), cell // np.uint64(width)
    s24 = 2.0 ** -24
    fx = (a2 >> np.uint64(8)).astype(np.float64) * s24
    fy = (a3 >> np.uint64(8)).astype(np.float64) * s24
    ft = (b0 >> np.uint64(8)).astype(np.float64) * s24
    x = (np.float64(np.float32(origin[0])) + (cx.astype(np.float64) + fx) * np.float64(np.float32(mpc))).astype(np.float32)
    y = (np.float64(np.float32(origin[1])) + (cy.astype(np.float64) + fy) * np.float64(np.float32(mpc))).astype(np.float32)
    th = wrap_to_pi(((2.0 * ft - 1.0) * math.pi).astype(np.float32))
    return x, y, th


def model_cloud(seed, cells, origin, mpc, n, dist=None, min_dist=0.0, chunks=1):
    """The whole cloud of n particles, formed in `chunks` pieces of consecutive indices."""
    elig = eligible_cells(cells, dist, min_dist)
    assert len(elig) > 0
    w = np.asarray(cells).shape[1]
    parts = [sample(seed, elig, w, origin, mpc, ix) for ix in np.array_split(np.arange(n, dtype=np.uint64), chunks)]
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(3))


def as_particles(x, y, th, utime, dtype):
    """A PARTICLE_DTYPE array: parent = pose, weight 1 / N."""
    out = np.zeros(len(x), dtype=dtype)
    out["utime"] = utime
    out["p_utime"] = utime
    out["x"], out["y"], out["theta"] = x, y, th
    out["p_x"], out["p_y"], out["p_theta"] = x, y, th
    out["weight"] = 1.0 / len(x)
    return out


def spread_model(x, y, th, units):
    """bl_pf_spread in float64 (exact integers for the units)."""
    u = np.asarray(units, dtype=np.uint64)
    S = int(u.sum(dtype=np.uint64))
    Q = sum(int(v) * int(v) for v in u) if len(u) < 50_000 else int((u.astype(object) ** 2).sum())
    du = u.astype(np.float64)
    x, y, th = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (x, y, th))
    mx, my = (du * x).sum() / S, (du * y).sum() / S
    dx, dy = x - mx, y - my
    R = math.hypot((du * np.cos(th)).sum(), (du * np.sin(th)).sum()) / S
    return dict(units_sum=S, units_sq=Q, n_eff=(float(S) * float(S)) / float(Q), mean_x=mx, mean_y=my,
                var_x=(du * dx * dx).sum() / S, var_y=(du * dy * dy).sum() / S, cov_xy=(du * dx * dy).sum() / S, theta_resultant=R)


def spread_stds_of(parts):
    """(position std, heading circular std) of a particle array's weighted cloud, as the driver's convergence test forms them."""
    w = parts["weight"].astype(np.float64)
    w = w / w.sum()
    x, y, th = (parts[f].astype(np.float64) for f in ("x", "y", "theta"))
    mx, my = (w * x).sum(), (w * y).sum()
    a, c, b = (w * (x - mx) ** 2).sum(), (w * (y - my) ** 2).sum(), (w * (x - mx) * (y - my)).sum()
    lam = 0.5 * (a + c) + math.sqrt(0.25 * (a - c) ** 2 + b * b)
    R = math.hypot((w * np.cos(th)).sum(), (w * np.sin(th)).sum())
    return math.sqrt(lam), math.sqrt(-2.0 * math.log(R))


def near_weight(parts, truth, pos_tol=CAL_NEAR_POS, th_tol=CAL_NEAR_THETA):
    """Weight of the particles within pos_tol metres and th_tol radians of the truth pose."""
    d = np.hypot(parts["x"].astype(np.float64) - truth[0], parts["y"].astype(np.float64) - truth[1])
    dth = np.abs(np.angle(np.exp(1j * (parts["theta"].astype(np.float64) - truth[2]))))
    w = parts["weight"].astype(np.float64)
    return float(w[(d <= pos_tol) & (dth <= th_tol)].sum() / w.sum())
