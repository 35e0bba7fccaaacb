"""The beam model's definition (include/botlab_hip.h, "beam model") as tests/beam_model.py states it: against a plain-loop
implementation with its own walk, integer square root and logarithm; the tables' properties; the two-wall case the feature exists
for; and the symmetries of the score.  No GPU."""
import math

import numpy as np
import pytest

import botlab_amd as bl
import beam_cases as bc
import beam_model as bm
import scan_match_model as sm

F32 = np.float32


# ------------------------------------------------------------------------------------------------ the plain-loop implementation
def loop_isqrt(v):
    if v < 2:
        return v
    r = 1 << ((v.bit_length() + 1) // 2)
    while True:
        n = (r + v // r) // 2
        if n >= r:
            return r
        r = n


def loop_lg(p, t):
    e = p.bit_length() - 1
    mant = (((p << (31 - e)) & 0xFFFFFFFF) >> 23) & 255
    return (e - 30) * t["ln2"] + int(t["lt"][mant])


def loop_score(c, pose, t):
    """S of one pose, ray by ray, the walk as the reference's loop (mapping.cpp:101-127); also the per-ray values."""
    cells, p = c["cells"], c["params"]
    h, w = cells.shape
    pose = tuple(F32(v) for v in pose)
    if not all(math.isfinite(float(v)) for v in pose):
        return bm.OFF_GRID, None
    px, py = sm.grid_position(pose[0], pose[1], c["origin"], F32(c["cpm"]))
    if not (abs(float(px)) < 2.0 ** 30 and abs(float(py)) < 2.0 ** 30):
        return bm.OFF_GRID, None
    sx, sy = int(float(px)), int(float(py))
    if not (0 <= sx < w and 0 <= sy < h):
        return bm.OFF_GRID, None
    used, seen = [], 0
    for rg, th in zip(c["ranges"].tolist(), c["thetas"].tolist()):
        if not (math.isfinite(rg) and F32(rg) > sm.MIN_RANGE):
            continue
        if seen % p["ray_stride"] == 0:
            used.append((F32(rg), F32(th)))
        seen += 1
    total, rows = 0, []
    mr = F32(p["max_range"])
    for rg, th in used:
        is_max = bool(rg >= mr)
        ex, ey, has_e = sm.endpoints(np.array([rg]), np.array([th]), pose, 0, F32(0), c["origin"], c["cpm"])
        mx, my, has_m = sm.endpoints(np.array([mr]), np.array([th]), pose, 0, F32(0), c["origin"], c["cpm"])
        if not has_m[0] or not (is_max or has_e[0]):
            rows.append((-1, -1, -1, -1, 0))
            continue
        x1, y1 = int(mx[0]), int(my[0])
        dx, dy = abs(x1 - sx), abs(y1 - sy)
        stx, sty = (1 if sx < x1 else -1), (1 if sy < y1 else -1)
        err, x, y, k, first, hit_cell = dx - dy, sx, sy, 0, None, None
        while x != x1 or y != y1:
            if 0 <= x < w and 0 <= y < h and cells[y, x] >= p["occ_min"]:
                first, hit_cell = k, (x, y)
                break
            e2 = 2 * err
            if e2 >= -dy:
                err -= dy
                x += stx
            if e2 <= dx:
                err += dx
                y += sty
            k += 1
        K = max(dx, dy)
        zstar = loop_isqrt(16 * ((hit_cell[0] - sx) ** 2 + (hit_cell[1] - sy) ** 2)) if hit_cell else -1
        if is_max:
            z, pv = -1, (t["max_blocked"] if hit_cell else t["max_free"])
        else:
            z = loop_isqrt(16 * ((int(ex[0]) - sx) ** 2 + (int(ey[0]) - sy) ** 2))
            pv = t["rand"]
            if hit_cell:
                pv += int(t["hit"][min(abs(z - zstar), p["hit_cut"])])
            if not hit_cell or z < zstar:
                pv += int(t["short"][min(z >> 2, 1023)])
        total += loop_lg(pv, t)
        rows.append((K if first is None else first, K, z, zstar, pv))
    return total, rows


ALL_CASES = [("two_walls", bc.two_walls), ("conditions", lambda: bc.conditions(64, 48)), ("conditions_occ2", lambda: bc.conditions(37, 23, occ_min=2)),
             ("open_64", lambda: bc.open_field(64, 48, 64)), ("open_wall", lambda: bc.open_field(130, 70, 130, wall_x=100)),
             ("rays_stride3", lambda: bc.ray_count(65, stride=3, dropped_every=4)), ("many", lambda: bc.many_poses(40)), ("mirror", bc.mirror_case)]


@pytest.mark.parametrize("name,make", ALL_CASES, ids=[n for n, _ in ALL_CASES])
def test_model_equals_the_plain_loops(name, make):
    c = make()
    t = bm.make_tables(c["params"], c["cpm"])
    S = bm.scores(c["cells"], c["origin"], c["cpm"], c["ranges"], c["thetas"], c["poses"], c["params"], t)
    rays = bm.used_rays(c["ranges"], c["thetas"], c["params"])
    for i, pose in enumerate(c["poses"]):
        exp, rows = loop_score(c, pose, t)
        assert int(S[i]) == exp, (name, i)
        got = bm.cast(c["cells"], c["origin"], c["cpm"], rays, pose, c["params"], t)
        assert (got is None) == (rows is None)
        if rows is not None:
            assert len(rows) == len(rays[0])
            for k, col in enumerate(("first", "K", "z", "zstar", "p")):
                assert got[col].tolist() == [r[k] for r in rows], (name, i, col)


def test_the_cases_reach_what_they_are_built_for():
    c = bc.conditions(64, 48)
    t = bm.make_tables(c["params"], c["cpm"])
    rays = bm.used_rays(c["ranges"], c["thetas"], c["params"])
    assert len(rays[0]) == 32 + 5                                         # 0.15, NaN, inf, -1 and 0 dropped
    assert rays[2][-5:].tolist() == [False, True, False, True, True]     # just above 0.15; max_range; just below it; 2 max_range twice
    seen = dict(first0=False, firstK=False, max_hit=False, max_free=False, short=False, behind=False, off=0)
    for pose in c["poses"]:
        g = bm.cast(c["cells"], c["origin"], c["cpm"], rays, pose, c["params"], t)
        if g is None:
            seen["off"] += 1
            continue
        seen["first0"] |= bool((g["first"] == 0).any())
        seen["firstK"] |= bool(((g["first"] == g["K"]) & (g["K"] > 0)).any())
        seen["max_hit"] |= bool(((g["z"] < 0) & (g["zstar"] >= 0)).any())
        seen["max_free"] |= bool(((g["z"] < 0) & (g["zstar"] < 0) & (g["p"] > 0)).any())
        seen["short"] |= bool(((g["z"] >= 0) & (g["zstar"] > g["z"])).any())
        seen["behind"] |= bool(((g["zstar"] >= 0) & (g["z"] > g["zstar"])).any())
    assert seen == dict(first0=True, firstK=True, max_hit=True, max_free=True, short=True, behind=True, off=4), seen
    o = bc.open_field(64, 48, 65)
    g = bm.cast(o["cells"], o["origin"], o["cpm"], bm.used_rays(o["ranges"], o["thetas"], o["params"]), o["poses"][0], o["params"],
                bm.make_tables(o["params"], o["cpm"]))
    assert 65 in g["K"].tolist() and (g["first"] == g["K"]).all()        # the walk leaves the grid, nothing expected


def test_closed_form_walk_is_the_loop():
    import obstacle_layer_model as om
    for (x1, y1) in [(7, 3), (-7, 3), (3, -7), (-5, -5), (9, 0), (0, -9), (64, 33), (-65, 64), (1, 130)]:
        xs, ys = om.walk(2, 3, 2 + x1, 3 + y1)
        assert list(zip(xs.tolist(), ys.tolist())) == om.walk_loop(2, 3, 2 + x1, 3 + y1)


def test_table_properties():
    U = bm.unit_table()
    assert U[0] == 2 ** 20 and U[256] == 1 and (np.diff(U.astype(np.int64)) <= 0).all()
    assert np.array_equal(U, bl.BeamModel.unitTable())                    # the library's, host arithmetic only
    t = bm.make_tables(bm.params(), bc.CPM)
    assert t["ln2"] == 45426 and t["lt"][0] == 0 and t["reach"] == 100
    ps = np.unique(np.concatenate([np.arange(1, 5000), 2 ** np.arange(0, 31) - 1, 2 ** np.arange(0, 31), 2 ** np.arange(0, 31) + 1,
                                   np.random.default_rng(1).integers(1, 2 ** 31 - 1, 20000)]))
    ps = ps[(ps >= 1) & (ps < 2 ** 31)]
    v = bm.lg(ps, t)
    assert (np.diff(v) >= 0).all()                                        # non-decreasing in p
    assert abs(int(bm.lg(np.array([2 ** 30]), t)[0])) == 0
    exact = 65536.0 * np.log(ps / 2.0 ** 30)
    assert np.abs(v - exact).max() <= 65536.0 / 256 + 2                   # the mantissa keeps 8 bits: below by at most ln(1 + 1 / 256)
    assert (np.diff(t["hit"].astype(np.int64)) <= 0).all() and (np.diff(t["short"].astype(np.int64)) <= 0).all()


def test_parameter_rule():
    assert bm.params_ok(bm.params())
    for bad in (dict(z_rand=0.0), dict(z_max=0.0), dict(blocked_factor=0.0), dict(z_rand=1e-7), dict(z_hit=1.5, z_rand=0.6),
                dict(z_hit=2.5), dict(hit_cut=0), dict(hit_cut=1024), dict(span=0), dict(ray_stride=65), dict(occ_min=0),
                dict(sigma_cells=0.0), dict(max_range=0.15), dict(max_range=float("nan")), dict(lam=-1.0)):
        assert not bm.params_ok(bm.params(**bad)), bad
    with pytest.raises(bm.ArgError):
        bm.make_tables(bm.params(max_range=300.0), bc.CPM)


def test_two_walls_the_endpoint_score_ties_and_the_beam_score_does_not():
    c = bc.two_walls()
    assert c["cells"].shape == (48, 96)
    A, B = c["poses"]
    rg, th = sm.valid_rays(c["ranges"], c["thetas"], 8.0)
    end = [int(sm.score_volume(c["cells"], c["origin"], c["cpm"], rg, th, tuple(p), 0, 0, 0, F32(0.01))[0, 0, 0]) for p in (A, B)]
    assert end[0] == end[1] == 100 * len(rg)                              # every end cell in a wall, for both
    t = bm.make_tables(c["params"], c["cpm"])
    S = bm.scores(c["cells"], c["origin"], c["cpm"], c["ranges"], c["thetas"], c["poses"], c["params"], t)
    assert S[0] > S[1]
    u = bm.units(S, bm.DEFAULTS["span"])
    assert u[0] == 2 ** 20 and u[1] == 1                                  # B at the floor for the default span
    gb = bm.cast(c["cells"], c["origin"], c["cpm"], bm.used_rays(c["ranges"], c["thetas"], c["params"]), B, c["params"], t)
    assert (gb["zstar"] < gb["z"]).all() and (gb["first"] < gb["K"]).all()    # B's rays pass through the first wall


def test_units_rule():
    span = 1000
    S = np.array([50, 50, 50 - span + 1, 50 - span, 50 - span - 1, bm.OFF_GRID, 49, -10 ** 9], np.int64)
    u = bm.units(S, span)
    U = bm.unit_table()
    assert u.tolist() == [2 ** 20, 2 ** 20, int(U[255]), 1, 1, 1, int(U[0]), 1]
    assert bm.units(np.array([bm.OFF_GRID, bm.OFF_GRID]), span).tolist() == [1, 1]
    assert bm.units(np.zeros(3, np.int64), span).tolist() == [2 ** 20] * 3


def _ends(c, poses, thetas):
    """(s, e, m) cells per pose and ray, for the mirror-exactness check."""
    out = []
    mr = np.full(len(thetas), F32(c["params"]["max_range"]), np.float32)
    for p in poses:
        s = bm.pose_start(p, c["origin"], c["cpm"], c["cells"].shape[1], c["cells"].shape[0])
        ex, ey, he = sm.endpoints(c["ranges"], thetas, tuple(F32(v) for v in p), 0, F32(0), c["origin"], c["cpm"])
        mx, my, hm = sm.endpoints(mr, thetas, tuple(F32(v) for v in p), 0, F32(0), c["origin"], c["cpm"])
        assert he.all() and hm.all() and s is not None
        out.append((s, ex, ey, mx, my))
    return out


def test_symmetry_transpose_and_mirror():
    c = bc.mirror_case()
    h, w = c["cells"].shape
    t = bm.make_tables(c["params"], c["cpm"])
    S = bm.scores(c["cells"], c["origin"], c["cpm"], c["ranges"], c["thetas"], c["poses"], c["params"], t)
    base = _ends(c, c["poses"], c["thetas"])
    # x <-> y: the grid transposed, (x, y, theta) -> (y, x, pi / 2 - theta), the rays' angles negated
    pt = np.stack([c["poses"][:, 1], c["poses"][:, 0], (F32(math.pi / 2) - c["poses"][:, 2]).astype(np.float32)], axis=1)
    ct = dict(c, cells=np.ascontiguousarray(c["cells"].T))
    for (s, ex, ey, mx, my), (s2, ex2, ey2, mx2, my2) in zip(base, _ends(ct, pt, -c["thetas"])):
        assert s2 == (s[1], s[0]) and np.array_equal(ex2, ey) and np.array_equal(ey2, ex) and np.array_equal(mx2, my) and np.array_equal(my2, mx)
    St = bm.scores(ct["cells"], c["origin"], c["cpm"], c["ranges"], -c["thetas"], pt, c["params"], t)
    assert np.array_equal(S, St)
    # x -> W - 1 - x: the grid mirrored, (x, y, theta) -> (W mpc - x, y, pi - theta), the rays' angles negated
    pm = np.stack([(F32(w * bc.MPC) - c["poses"][:, 0]).astype(np.float32), c["poses"][:, 1], (F32(math.pi) - c["poses"][:, 2]).astype(np.float32)], axis=1)
    cm = dict(c, cells=np.ascontiguousarray(c["cells"][:, ::-1]))
    for (s, ex, ey, mx, my), (s2, ex2, ey2, mx2, my2) in zip(base, _ends(cm, pm, -c["thetas"])):
        assert s2 == (w - 1 - s[0], s[1]) and np.array_equal(ex2, w - 1 - ex) and np.array_equal(ey2, ey)
        assert np.array_equal(mx2, w - 1 - mx) and np.array_equal(my2, my)
    Sm = bm.scores(cm["cells"], c["origin"], c["cpm"], c["ranges"], -c["thetas"], pm, c["params"], t)
    assert np.array_equal(S, Sm)
    assert len(set(S.tolist())) > 1 and (S != bm.OFF_GRID).all()
