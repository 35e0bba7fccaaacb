"""The numpy model of the global-localization sampler (tests/global_init_model.py): its properties on the shipped maps and on a
ragged grid, and the calibration of global localization on the CPU reference filter -- the one place the scenario constants the GPU
tests reuse (CAL_*) are measured."""
import math

import numpy as np
import pytest

import global_init_model as gm
import helpers
from botlab_amd import synth
from botlab_amd.host import PARTICLE_DTYPE


def _ragged(maps):
    c = np.tile(maps["obstacle_slam_10mx10m_5cm"]["cells"], (3, 3))[:333, :517]      # W, H no multiples of 4 or 64
    return np.ascontiguousarray(c), (np.float32(-8.3), np.float32(-4.1)), np.float32(0.05)


def _chi2_z(counts, expected):
    chi2 = float((((counts - expected) ** 2) / expected).sum())
    df = len(counts) - 1
    return (chi2 - df) / math.sqrt(2.0 * df)


def test_philox_known_answer():
    """Philox4x32-10 against the published known-answer vector (Random123 kat_vectors: counter and key all ones)."""
    out = gm.philox4x32(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)
    assert [int(v) for v in out] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    out = gm.philox4x32(0, 0, 0, 0, 0, 0)
    assert [int(v) for v in out] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]


@pytest.mark.parametrize("name", ["obstacle_slam_10mx10m_5cm", "convex_10mx10m_5cm", "drive_square_10mx10m_5cm", "narrow", "ragged"])
def test_sampler_properties(maps, name):
    if name == "ragged":
        cells, origin, mpc = _ragged(maps)
    else:
        m = maps[name]
        cells, origin, mpc = m["cells"], m["origin"], m["mpc"]
    h, w = cells.shape
    elig = gm.eligible_cells(cells)
    F = len(elig)
    n = 20 * F
    x, y, th = gm.model_cloud(99, cells, origin, mpc, n)
    # every particle on an eligible cell (the float pose maps back to the cell it was drawn in)
    cx = np.floor((x.astype(np.float64) - np.float64(origin[0])) / np.float64(mpc)).astype(np.int64)
    cy = np.floor((y.astype(np.float64) - np.float64(origin[1])) / np.float64(mpc)).astype(np.int64)
    cx, cy = np.clip(cx, 0, w - 1), np.clip(cy, 0, h - 1)
    assert np.all(cells[cy, cx] < 0)
    # uniform over the eligible cells
    counts = np.bincount(np.searchsorted(elig, (cy * w + cx).astype(np.uint64)), minlength=F)
    assert abs(_chi2_z(counts, n / F)) < 5.0
    # uniform heading in the range of wrap_to_pi
    assert np.all(th > -gm.PI_F) and np.all(th < gm.PI_F)
    hist = np.histogram(th.astype(np.float64), bins=72, range=(-math.pi, math.pi))[0]
    assert abs(_chi2_z(hist, n / 72)) < 5.0
    # sub-cell offsets uniform
    off = (x.astype(np.float64) - np.float64(origin[0])) / np.float64(mpc) - cx
    assert abs(_chi2_z(np.histogram(off, bins=20, range=(0, 1))[0], n / 20)) < 5.0
    # independent of how the particles are split into launches / ranks
    x2, y2, th2 = gm.model_cloud(99, cells, origin, mpc, n, chunks=7)
    assert x2.tobytes() == x.tobytes() and y2.tobytes() == y.tobytes() and th2.tobytes() == th.tobytes()


def test_distance_filter(maps):
    cells, origin, mpc = _ragged(maps)
    occ = cells > 0
    # a crude distance field: cells of the ring around an occupied cell get 0.05, farther cells 1.0, occupied ones 0
    near = np.zeros_like(occ)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            near |= np.roll(np.roll(occ, dy, 0), dx, 1)
    dist = np.where(occ, 0.0, np.where(near, 0.05, 1.0)).astype(np.float32)
    x, y, _ = gm.model_cloud(5, cells, origin, mpc, 50_000, dist, 0.1)
    cx = ((x.astype(np.float64) - np.float64(origin[0])) / np.float64(mpc)).astype(np.int64)
    cy = ((y.astype(np.float64) - np.float64(origin[1])) / np.float64(mpc)).astype(np.int64)
    assert np.all(dist[cy, cx] > 0.1) and np.all(cells[cy, cx] < 0)
    assert len(gm.eligible_cells(cells, dist, 0.1)) < len(gm.eligible_cells(cells))


def test_rank_without_modulo_bias():
    """hi64(x * F) of the model against Python's exact integers."""
    rng = np.random.default_rng(1)
    a0 = rng.integers(0, 2**32, 2000, dtype=np.uint64)
    a1 = rng.integers(0, 2**32, 2000, dtype=np.uint64)
    for F in (1, 2, 3, 1000, 2**31 - 1):
        r = (a0 * np.uint64(F) + ((a1 * np.uint64(F)) >> np.uint64(32))) >> np.uint64(32)
        want = [((int(p) << 32 | int(q)) * F) >> 64 for p, q in zip(a0, a1)]
        assert [int(v) for v in r] == want


def test_global_init_calibration(oracle, maps):
    """Global localization on the CPU reference filter (ParticleFilter of the reference, sensor model of linear log-odds sums):
    CAL_N particles of the model's cloud over obstacle_slam_10mx10m_5cm, lidar along the square trajectory from CAL_START.
    Measured: the weight within 0.3 m / 0.3 rad of the truth first passes 0.9 after 38 moved updates and the estimate is within
    0.1 m from then on (0.99 / 0.016 m at 50); CAL_K = 50 leaves that margin.  The cloud's spread falls below the driver's default
    thresholds (0.2 m, 0.3 rad) after about 43 moved updates (0.146 m / 0.151 rad at 45, 0.075 m / 0.113 rad at 50)."""
    import oracle_lib
    m = maps[gm.CAL_MAP]
    cells, origin, mpc, cpm = m["cells"], m["origin"], m["mpc"], helpers.CPM_DEFAULT
    truth = np.where(cells > 0, 127, -127).astype(np.int8)
    poses = synth.square_trajectory(gm.CAL_START, gm.CAL_STEPS, **gm.CAL_TRAJ)
    odo = synth.odometry_from_truth(poses, np.random.default_rng(3))
    x, y, th = gm.model_cloud(gm.CAL_SEED, cells, origin, mpc, gm.CAL_N)
    opf = oracle_lib.OraclePF(oracle, gm.CAL_N)
    opf.set_particles(gm.as_particles(x, y, th, 1000, PARTICLE_DTYPE))
    # the start is not ambiguous: the cloud holds almost no weight near the truth before the first update
    assert gm.near_weight(opf.particles(), poses[0]) < 0.01
    moved, k = 0, 0
    while moved < gm.CAL_K:
        k += 1
        scan = synth.raycast_scan(truth, origin, 0.05, poses[k - 1], poses[k], 1000 + 100000 * k)
        res = opf.update(oracle.pose(*odo[k], utime=scan.utime), scan, cells, mpc, cpm, origin, 1000 + k)
        moved += res["moved"]
    tr = poses[k]
    parts = opf.particles()
    assert gm.near_weight(parts, tr) >= gm.CAL_NEAR_WEIGHT
    assert math.hypot(res["pose"].x - tr[0], res["pose"].y - tr[1]) <= gm.CAL_EST_TOL
    pos, heading = gm.spread_stds_of(parts)
    assert pos <= gm.DRIVER_POS_TOL and heading <= gm.DRIVER_HEADING_TOL
    assert k < len(poses)


def test_steady_spread_from_true_pose(oracle, maps):
    """The spread a filter started at the true pose holds in the calibrated scenario (measured: at most 0.025 m and 0.100 rad
    over the 60 updates), the yardstick of the driver's default convergence thresholds (at least twice it)."""
    import oracle_lib
    m = maps[gm.CAL_MAP]
    cells, origin, mpc, cpm = m["cells"], m["origin"], m["mpc"], helpers.CPM_DEFAULT
    truth = np.where(cells > 0, 127, -127).astype(np.int8)
    poses = synth.square_trajectory(gm.CAL_START, gm.CAL_STEPS, **gm.CAL_TRAJ)
    odo = synth.odometry_from_truth(poses, np.random.default_rng(3))
    opf = oracle_lib.OraclePF(oracle, 5000)
    opf.init_at_pose(oracle.pose(*gm.CAL_START, utime=1000), 5)
    worst = [0.0, 0.0]
    for k in range(1, len(poses)):
        scan = synth.raycast_scan(truth, origin, 0.05, poses[k - 1], poses[k], 1000 + 100000 * k)
        opf.update(oracle.pose(*odo[k], utime=scan.utime), scan, cells, mpc, cpm, origin, 1000 + k)
        pos, heading = gm.spread_stds_of(opf.particles())
        worst = [max(worst[0], pos), max(worst[1], heading)]
    assert worst[0] <= gm.CAL_STEADY_POS and worst[1] <= gm.CAL_STEADY_THETA, worst
    assert gm.DRIVER_POS_TOL >= 2 * gm.CAL_STEADY_POS and gm.DRIVER_HEADING_TOL >= 2 * gm.CAL_STEADY_THETA
