"""Inputs for the kernel paths and integer edges of the beam model that tests/beam_cases.py does not reach: many
workgroups for k_beam_final, windows inside a textured grid, walks of 4096 cells with the table clamps and the square root at its
largest arguments, other frames, the logarithm over p's range.  A case is beam_cases' dict; a builder may add members that say what
it claims (tests/test_beam_edge_cases_cpu.py proves each claim on the model, tests/test_gpu_beam_edges.py runs the case)."""
import math

import numpy as np

import beam_cases as bc
import beam_model as bm

F32 = np.float32
WG = 32                                                   # poses per workgroup of k_beam_cast
OFF_POSE = (-0.25, 0.15, 0.0)                             # off every grid here whose origin is (0, 0)


def centre(cx, cy, theta=0.0, origin=(0.0, 0.0), mpc=bc.MPC):
    """The pose at the centre of cell (cx, cy) of a grid at `origin` with cells of mpc metres."""
    return (F32(origin[0] + (cx + 0.5) * mpc), F32(origin[1] + (cy + 0.5) * mpc), F32(theta))


def case(cells, ranges, thetas, poses, origin=(0.0, 0.0), mpc=bc.MPC, cpm=bc.CPM, **prm):
    return dict(cells=np.ascontiguousarray(cells, dtype=np.int8), origin=(F32(origin[0]), F32(origin[1])), mpc=float(mpc), cpm=float(F32(cpm)),
                ranges=np.asarray(ranges, dtype=np.float32), thetas=np.asarray(thetas, dtype=np.float32),
                poses=np.asarray(poses, dtype=np.float32).reshape(-1, 3), params=bm.params(**prm))


def model_scores(c, t, chunk=256):
    """bm.scores of the case's DISTINCT poses, tiled over the poses; the rays in chunks (S is a sum over the rays), so that 4096 rays
    of 4096 cells need no 4096 x 4096 arrays."""
    rays = bm.used_rays(c["ranges"], c["thetas"], c["params"])
    uniq, inv = np.unique(c["poses"].view(np.uint32), axis=0, return_inverse=True)
    out = np.empty(len(uniq), np.int64)
    for i, bits in enumerate(uniq):
        pose, total = bits.view(np.float32), 0
        for a in range(0, max(len(rays[0]), 1), chunk):
            g = bm.cast(c["cells"], c["origin"], c["cpm"], tuple(v[a:a + chunk] for v in rays), pose, c["params"], t)
            if g is None:
                total = bm.OFF_GRID
                break
            total += int(bm.lg(g["p"][g["p"] > 0], t).sum())
        out[i] = total
    return out[np.asarray(inv).reshape(-1)]


def wg_windows(c, reach=None):
    """Per workgroup of the case's poses: None for an empty bounding box (no pose takes part), else bm.window of its start cells."""
    h, w = c["cells"].shape
    reach = bm.reach_cells(c["params"], c["cpm"]) if reach is None else reach
    out = []
    for a in range(0, len(c["poses"]), WG):
        s = [bm.pose_start(p, c["origin"], c["cpm"], w, h) for p in c["poses"][a:a + WG]]
        s = [v for v in s if v is not None]
        if not s:
            out.append(None)
            continue
        box = (min(v[0] for v in s), min(v[1] for v in s), max(v[0] for v in s), max(v[1] for v in s))
        out.append(bm.window(box, reach, w, h))
    return out


def expected_path(c, window_bytes):
    """What bl_beam_debug_path answers with staging on: 0 every workgroup staged, 1 none, 2 some of each."""
    staged = [v is not None and v[2] * v[3] <= window_bytes for v in wg_windows(c)]
    return 0 if all(staged) else 1 if not any(staged) else 2


# ---------------------------------------------------------------------------------------------- A: many workgroups
def _smax_base():
    """The 64 x 48 room of ray_count and three returns that end in its walls as seen from cell (20, 20): the best pose stands there, the
    poor one two cells off.  span is twice their score gap, so the poor pose's j is 128."""
    room = bc.ray_count(0)["cells"]
    rg = [43 * bc.MPC, 27 * bc.MPC, 20 * bc.MPC]
    th = [0.0, -math.pi / 2, math.pi]
    best, poor = centre(20, 20), centre(22, 21)
    c = case(room, rg, th, [best, poor], max_range=3.0)
    S = bm.scores(c["cells"], c["origin"], c["cpm"], c["ranges"], c["thetas"], c["poses"], c["params"], bm.make_tables(c["params"], c["cpm"]))
    return room, rg, th, best, poor, 2 * int(S[0] - S[1])


def smax_case(B, wg, off_before=False):
    """32 (B - 1) + 1 poses, B workgroups, the last of one pose: the poor pose everywhere, the best pose once, in workgroup wg.  With
    off_before every pose before the best is off the grid: whole workgroups record BL_BEAM_OFF_GRID."""
    room, rg, th, best, poor, span = _smax_base()
    n = WG * (B - 1) + 1
    at = min(WG * wg + (7 * wg + 5) % WG, n - 1)
    poses = np.tile(np.array(poor, np.float32), (n, 1))
    if off_before:
        poses[:at] = np.array(OFF_POSE, np.float32)
    poses[at] = best
    return dict(case(room, rg, th, poses, max_range=3.0, span=span), best=at, blocks=B)


def smax_cases():
    """(B, wg, off_before) of every case of group A."""
    out = []
    for B in (64, 65, 1024, 1025, 2049):
        for wg in (0, 63, 64, 1023, 1024, B - 1):
            if wg < B and (B, wg, False) not in out:
                out.append((B, wg, False))
    for B in (65, 1025):
        for wg in (0, 63, 64, 1023, 1024, B - 1):
            if 0 < wg < B and (B, wg, True) not in out:
                out.append((B, wg, True))
    return out


def path_count_case(clustered):
    """130 x 70, a reach of 10 cells: one workgroup per entry of `clustered`, its 32 poses within two cells of each other (a window of
    28 x 27, which 2 KB holds) or scattered from corner to corner (no window fits 2 KB)."""
    base = bc.conditions(130, 70, max_range=0.5)
    rng = np.random.default_rng(4)
    near = [centre(64 + k % 2, 35 + (k // 2) % 2, 0.2 * k) for k in range(WG)]
    far = [centre(int(rng.integers(1, 129)), int(rng.integers(1, 69)), float(rng.uniform(-3, 3))) for _ in range(WG)]
    far[0], far[1] = centre(1, 1), centre(128, 68)
    poses = np.concatenate([np.array(near if cl else far, np.float32) for cl in clustered])
    return dict(base, poses=poses)


def filter_cloud():
    """The poses of a cloud of 2081 particles, 66 workgroups: the best one last, three off the grid, the poor pose elsewhere."""
    c = smax_case(66, 65)
    c["poses"][[5, 17, 2079]] = np.array(OFF_POSE, np.float32)
    assert c["best"] == 2080
    return c


# ---------------------------------------------------------------------------------------------- B: windows in a textured grid
TEX_H, TEX_REACH = 96, 10


def cluster_centres(W):
    """name -> (cx, cy): the workgroups of the textured case of width W."""
    out = {"round%d" % k: (60 + k, 48) for k in range(4)}                   # the window's left edge at every residue mod 4
    out.update(left=(2, 48), right=(W - 3, 48), bottom=(61, 2), top=(61, 93))
    out.update(bottom_left=(2, 2), bottom_right=(W - 3, 2), top_left=(2, 93), top_right=(W - 3, 93))
    return out


def cluster_poses(cx, cy):
    """32 poses on the 3 x 3 block of cells round (cx, cy), every cell of it used, headings all round."""
    return [centre(cx + k % 3 - 1, cy + (k // 3) % 3 - 1, 0.2 * k) for k in range(WG)]


def texture(W, seed=11):
    """96 x W cells, about one in seven occupied, the clusters' own 3 x 3 blocks free."""
    rng = np.random.default_rng(seed + W)
    cells = np.where(rng.random((TEX_H, W)) < 1.0 / 7.0, 100, -20).astype(np.int8)
    for cx, cy in cluster_centres(W).values():
        cells[cy - 1:cy + 2, cx - 1:cx + 2] = -20
    return cells


def texture_scan():
    """16 rays all round; returns from 3 to 9.5 cells, two max readings."""
    th = [2.0 * math.pi * k / 16 for k in range(16)]
    rg = [(3.0 + 0.5 * ((5 * k) % 14)) * bc.MPC for k in range(16)]
    rg[3], rg[12] = 0.5, 0.8
    return rg, th


def textured_case(W, names=None, lead_off=False, tail=False):
    """The clusters `names` (default: all twelve), a workgroup each; lead_off: a workgroup of off-grid poses first; tail: a last
    workgroup of one pose."""
    cc = cluster_centres(W)
    names = list(cc) if names is None else list(names)
    poses = [OFF_POSE] * WG if lead_off else []
    for nm in names:
        poses += cluster_poses(*cc[nm])
    if tail:
        poses.append(centre(40, 30, 1.0))
    rg, th = texture_scan()
    cells = texture(W)
    if tail:
        cells[30, 40] = -20
    return dict(case(cells, rg, th, poses, max_range=TEX_REACH * bc.MPC), names=names, first=(WG if lead_off else 0))


# ---------------------------------------------------------------------------------------------- C: 4096 cells
LONG_RANGE = 204.79                                       # ceil(float32(204.79) * 20) = 4096; 204.8 gives 4097
TOO_FAR = 204.8
LONG = dict(max_range=LONG_RANGE, lam=0.001, sigma_cells=100.0, hit_cut=1023)
# end cells (dx, dy) from the start cell: a perfect square, its neighbours, the diagonal; then cells where sqrtf of the rounded
# 16 (dx^2 + dy^2) is the next integer and the first correction of the integer square root does the work (the nearest such cell to the
# start is (473, 913): none lies within the 130 cells of beam_cases)
ROOT_CELLS = [(2400, 3200), (2400, 3199), (2400, 3201), (2890, 2890), (2891, 2891), (2895, 2895), (42, 3528), (473, 913), (4068, 186), (4086, 163)]


def aim(dx, dy, mpc=bc.MPC):
    """(range, theta) of the ray that, from a pose with heading 0 at a cell's centre, ends at the centre of the cell (dx, dy) further."""
    return math.hypot(dx, dy) * mpc, -math.atan2(dy, dx)


def clamp_rays():
    """(dx, dy) of three end cells whose z lies 1022, 1023 and 1024 quarter cells behind a hit in a wall column ten cells ahead."""
    out = []
    for target in (1022, 1023, 1024):
        for dy in range(1, 30):
            for dx in range(250, 280):
                minor = (2 * 10 * dy + dx) // (2 * dx)
                if int(bm.quarter(dx, dy, 0, 0)) - int(bm.quarter(10, minor, 0, 0)) == target and (dx, dy) not in out:
                    out.append((dx, dy))
                    break
            else:
                continue
            break
    assert len(out) == 3
    return out


def corridor(W, wall_x=None, occupied=(), extra_poses=(), rays=None):
    """5 x W, free but for the column wall_x and the cells `occupied`; poses at both ends and in the middle on the middle row, headings
    0 and pi; returns along the heading at 1022, 1023, 1024, 4000 and 4095 cells, two max readings, the clamp_rays and the ROOT_CELLS."""
    cells = np.full((5, W), -20, np.int8)
    if wall_x is not None:
        cells[:, wall_x] = 100
    for x, y in occupied:
        cells[y, x] = 100
    if rays is None:
        rays = [(n * bc.MPC, 0.0) for n in (1022, 1023, 1024, 4000, 4095)] + [(LONG_RANGE, 0.0), (300.0, 0.0)]
        rays += [aim(dx, dy) for dx, dy in clamp_rays()] + [aim(dx, -dy) for dx, dy in clamp_rays()] + [aim(dx, dy) for dx, dy in ROOT_CELLS]
    poses = [centre(3, 2), centre(4, 2), centre(W // 2, 2), centre(W // 2, 2, math.pi), centre(W - 4, 2, math.pi), centre(W - 5, 2, math.pi)]
    poses += list(extra_poses)
    return case(cells, [r[0] for r in rays], [r[1] for r in rays], poses, **LONG)


def corridor_free(W):
    return corridor(W)


def corridor_wall(W):
    """A wall column 4090 cells from the first pose and 4089 from the second (z* = 16360 and 16356), a few cells from the poses at the far
    end, and ten cells ahead of an extra pose that the clamp_rays are made for."""
    return corridor(W, wall_x=4093, extra_poses=[centre(4083, 2), centre(4083, 1), centre(4083, 3)])


def corridor_end(W, at_far_cell):
    """One ray along the heading, as a return and as a max reading; the only occupied cell of the first pose's walk (heading 0, on row
    1) and of the second's (heading pi, on row 3) at the far cell m itself, or at the walk's last cell before it."""
    step = 0 if at_far_cell else 1
    c = corridor(W, rays=[(4000 * bc.MPC, 0.0), (LONG_RANGE, 0.0)])
    c["poses"] = np.array([centre(3, 1), centre(W - 4, 3, math.pi)], np.float32)
    rays = bm.used_rays(c["ranges"], c["thetas"], c["params"])
    ends = []
    for pose, sign in zip(c["poses"], (1, -1)):
        s = bm.pose_start(pose, c["origin"], c["cpm"], W, 5)
        g = bm.cast(c["cells"], c["origin"], c["cpm"], rays, pose, c["params"], bm.make_tables(c["params"], c["cpm"]))
        assert g["K"].tolist() == [4096, 4096]
        ends.append((s[0] + sign * (4096 - step), s[1]))
    for x, y in ends:
        c["cells"][y, x] = 100
    return dict(c, ends=ends)


def floor_p_case(max_reading=False):
    """Every return scores lg(1): z_rand = 2^-19 at a reach of 4096 cells gives Rand = lround(0.5) = 1, and z_hit = z_short = 0.  4096
    rays all round on an 8 x 8 grid with a wall: 4096 lg(1) is the most negative score there is.  With max_reading the last ray is
    one: MaxFree for the pose that looks at nothing, MaxBlocked for the one that faces the wall."""
    cells = np.full((8, 8), -20, np.int8)
    cells[:, 6] = 100
    th = [2.0 * math.pi * k / 4096 for k in range(4096)]
    rg = [0.2 + 0.04 * (k % 5000) for k in range(4096)]
    if max_reading:
        th[-1], rg[-1] = 0.0, 250.0
    poses = [centre(3, 3), centre(3, 3, math.pi), OFF_POSE]
    return case(cells, rg, th, poses, max_range=LONG_RANGE, z_rand=2.0 ** -19, z_hit=0.0, z_short=0.0)


# ---------------------------------------------------------------------------------------------- D: other frames
FRAMES = [(o, cpm) for o in ((-3.7, 12.3), (5.0, -0.85)) for cpm in (10.0, 40.0, float(F32(1 / 0.03)))]


def conditions_frame(w, h, origin, cpm, **prm):
    """beam_cases.conditions on a grid at `origin` with cpm cells per metre: poses at the same cells, ranges the same number of cells
    (the two at the 0.15 m limit and the dropped ones as they are)."""
    mpc = {10.0: 0.1, 40.0: 0.025}.get(cpm, 0.03)
    base = bc.conditions(w, h, **prm)
    scale = bc.CPM * mpc                                                     # a range of r metres at 20 cells per metre is r scale here
    mr = float(F32(base["params"]["max_range"] * scale))
    rg = base["ranges"].astype(np.float64) * scale
    rg[32], rg[33] = 0.15, np.nextafter(F32(0.15), F32(1))
    rg[34], rg[35] = mr, np.nextafter(F32(mr), F32(0))
    rg[38], rg[39] = 2 * mr, 2 * mr
    at = [(w // 2, h // 2, 0.0), (5, 5, 0.7), (1, 1, -2.0), (w - 2, h - 2, 3.1), (0, h // 2, 1.0), (-3, 4, 0.0), (w + 2, 2, 0.0), None, None,
          (w // 2, h // 2, 0.0), (w // 3, h // 3, 5.0)]
    poses = [centre(*v, origin=origin, mpc=mpc) if v else None for v in at]
    poses[7] = (F32("nan"), F32(origin[1] + 0.5), F32(0))
    poses[8] = (F32(origin[0] + 0.5), F32(origin[1] + 0.5), F32("inf"))
    return case(base["cells"], rg, base["thetas"], poses, origin=origin, mpc=mpc, cpm=cpm, **dict(dict(prm), max_range=mr))


# ---------------------------------------------------------------------------------------------- E: the logarithm, the parameter rule
def log_sweep():
    """The p of the sweep; every one is p / 2^30 exactly as a float32."""
    ps = [1, 2, 3, 255, 256, 257]
    for k in (8, 16, 23, 24, 29, 30):
        low = 2 ** max(k - 23, 0)
        ps += [2 ** k - low, 2 ** k, 2 ** k + 2 ** (k - 8) - low, 2 ** k + 2 ** (k - 8)]
    ps.append(2 ** 31 - 128)
    out = sorted(set(ps))
    assert all(float(F32(p / 2.0 ** 30)) * 2.0 ** 30 == p for p in out)
    return out


def log_case(p, blocked_factor=1.0):
    """An 8 x 8 grid, free but for a wall column; one max reading; the first pose looks away from the wall (S = lg(MaxFree)), the second
    at it (S = lg(MaxBlocked)); z_max = p / 2^30."""
    cells = np.full((8, 8), -20, np.int8)
    cells[:, 6] = 100
    return case(cells, [5.0], [0.0], [centre(3, 3, math.pi), centre(3, 3)], max_range=1.0, z_max=p / 2.0 ** 30, blocked_factor=blocked_factor)


def blocked_floor():
    """(accepted, refused): the least float32 blocked_factor for which lround(2^30 z_max blocked_factor) is 1 at the default z_max, and
    the float below it."""
    zm = bm.TWO30 * bm.params()["z_max"]
    b = F32(0.5 / zm)
    while bm._lround(zm * float(b)) < 1:
        b = np.nextafter(b, F32(1))
    while bm._lround(zm * float(np.nextafter(b, F32(0)))) >= 1:
        b = np.nextafter(b, F32(0))
    return float(b), float(np.nextafter(b, F32(0)))


def boundary_params():
    """(accepted, refused) pairs of parameter changes at bl_beam_set_params' two conditions on p."""
    one = float(np.nextafter(F32(1), F32(0)))
    ok_b, bad_b = blocked_floor()
    return [(dict(z_rand=2.0 ** -19), dict(z_rand=float(np.nextafter(F32(2.0 ** -19), F32(0))))),
            (dict(z_max=float(np.nextafter(F32(2), F32(0)))), dict(z_max=2.0)),
            (dict(z_hit=1.0, z_short=0.0, z_rand=one), dict(z_hit=1.0, z_short=0.0, z_rand=1.0)),
            (dict(blocked_factor=ok_b), dict(blocked_factor=bad_b))]
