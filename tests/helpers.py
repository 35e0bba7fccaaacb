"""Shared test helpers: golden fixtures and synthetic inputs."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")

SLAM_MAPS = ["convex_10mx10m_5cm", "convex_10mx10m_5cm_offcenter", "drive_square_10mx10m_5cm", "obstacle_slam_10mx10m_5cm"]
ASTAR_MAPS = ["astar_convex", "astar_empty", "astar_filled", "astar_maze", "astar_narrow", "astar_wide"]
GEN_MAPS = ["empty", "filled", "narrow", "wide"]
ALL_MAPS = SLAM_MAPS + GEN_MAPS + ASTAR_MAPS

CPM_DEFAULT = np.float32(1.0 / np.float64(np.float32(0.05)))    # cellsPerMeter_ after OccupancyGrid() + loadFromFile


def load_reference_maps():
    z = np.load(os.path.join(GOLDEN, "reference_maps.npz"))
    out = {}
    for name in ALL_MAPS:
        out[name] = dict(cells=z[name + "__cells"], origin=tuple(z[name + "__origin"]), mpc=z[name + "__mpc"][0])
    return out


def load_astar_cases():
    with open(os.path.join(GOLDEN, "astar_cases.json")) as f:
        return json.load(f)


def ref_math_inputs():
    """The seeded inputs test_oracle_pins.py pins wrap_to_pi / angle_diff / angle_sum / interpolate_pose_by_time on:
    20 009 float32 angles, 20 000 double pairs, 5 000 (begin, end, t) triples.  Poses are (utime, x, y, theta) with
    float32-exact coordinates."""
    import math
    rng = np.random.default_rng(7)
    angles = np.concatenate([rng.uniform(-20, 20, 20000), [0.0, math.pi, -math.pi, np.float32(math.pi), -np.float32(math.pi),
                                                           3.1415927, -3.1415927, 6.2831855, 1e-30]]).astype(np.float32)
    pairs = rng.uniform(-7, 7, (20000, 2))
    n = 5000
    b_utime, e_utime, t = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    b_xyt, e_xyt = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    for i in range(n):
        b_utime[i] = int(rng.integers(0, 10**12))
        b_xyt[i] = rng.uniform(-5, 5, 3)
        e_utime[i] = b_utime[i] + int(rng.integers(0, 200000))
        e_xyt[i] = rng.uniform(-5, 5, 3)
        t[i] = b_utime[i] + int(rng.integers(-1000, 201000))
    return dict(angles=angles, pairs=pairs, b_utime=b_utime, b_xyt=b_xyt, e_utime=e_utime, e_xyt=e_xyt, t=t)


def ref_math_inputs_digest(inp):
    import hashlib
    h = hashlib.sha256()
    for k in sorted(inp):
        h.update(k.encode())
        h.update(np.ascontiguousarray(inp[k]).tobytes())
    return h.hexdigest()


def load_ref_math_vectors():
    """tests/golden/ref_math_vectors.npz: what the reference's own angle_functions.hpp / interpolation.hpp return on
    ref_math_inputs() (written by tests/golden/make_ref_math_vectors.py)."""
    z = np.load(os.path.join(GOLDEN, "ref_math_vectors.npz"))
    return {k: z[k] for k in z.files}
