"""tests/beam_edge_cases.py on the model alone: every case reaches what its builder claims, and the vectorised model equals the plain
loops of test_beam_model_cpu.py on the new cases (the closed-form walk beside the loop at K = 4096 among them).  No GPU."""
import math

import numpy as np
import pytest

import beam_cases as bc
import beam_edge_cases as ec
import beam_model as bm
import scan_match_model as sm
from test_beam_model_cpu import loop_lg, loop_score

F32 = np.float32


def tables(c):
    return bm.make_tables(c["params"], c["cpm"])


def casts(c, t=None):
    """bm.cast of the case's distinct poses that take part."""
    t = tables(c) if t is None else t
    rays = bm.used_rays(c["ranges"], c["thetas"], c["params"])
    out = []
    for bits in np.unique(c["poses"].view(np.uint32), axis=0):
        g = bm.cast(c["cells"], c["origin"], c["cpm"], rays, bits.view(np.float32), c["params"], t)
        if g is not None:
            out.append(g)
    return out


def equals_the_loops(c):
    t = tables(c)
    rays = bm.used_rays(c["ranges"], c["thetas"], c["params"])
    uniq = np.unique(c["poses"].view(np.uint32), axis=0).view(np.float32)
    S = ec.model_scores(dict(c, poses=uniq), t)
    for i, pose in enumerate(uniq):
        exp, rows = loop_score(c, pose, t)
        assert int(S[i]) == exp, i
        got = bm.cast(c["cells"], c["origin"], c["cpm"], rays, pose, c["params"], t)
        assert (got is None) == (rows is None)
        if rows is not None:
            for k, col in enumerate(("first", "K", "z", "zstar", "p")):
                assert got[col].tolist() == [r[k] for r in rows], (i, col)


# ------------------------------------------------------------------------------------------------------------------ A
def test_smax_cases_order_the_poses_and_keep_the_poor_one_off_the_clamps():
    c = ec.smax_case(64, 0)
    t = tables(c)
    assert len(bm.used_rays(c["ranges"], c["thetas"], c["params"])[0]) == 3
    best, poor = c["poses"][c["best"]], c["poses"][c["best"] + 1]
    S = bm.scores(c["cells"], c["origin"], c["cpm"], c["ranges"], c["thetas"], [best, poor, ec.OFF_POSE], c["params"], t)
    assert S[0] > S[1] > bm.OFF_GRID == S[2]
    j = ((int(S[0]) - int(S[1])) * 256) // c["params"]["span"]
    assert 0 < j < 256 and bm.params_ok(c["params"])
    u = bm.units(S, c["params"]["span"])
    assert u[0] == 2 ** 20 and 1 < u[1] < 2 ** 20 and u[2] == 1
    equals_the_loops(c)


def test_smax_cases_put_the_best_pose_in_the_workgroup_they_name():
    seen = set()
    for B, wg, off in ec.smax_cases():
        c = ec.smax_case(B, wg, off)
        n = len(c["poses"])
        assert n == 32 * (B - 1) + 1 and (n + 31) // 32 == B and c["best"] // 32 == wg
        uniq, inv = np.unique(c["poses"].view(np.uint32), axis=0, return_inverse=True)
        assert len(uniq) == (3 if off and 0 < c["best"] < n - 1 else 2)
        S = ec.model_scores(c, tables(c))
        assert int(S.argmax()) == c["best"] and (S == S.max()).sum() == 1
        if off:
            assert (S[:c["best"]] == bm.OFF_GRID).all() and c["best"] >= 32 and (S[c["best"] + 1:] != bm.OFF_GRID).all()
            u = bm.units(S, c["params"]["span"])
            assert (u[:c["best"]] == 1).all() and u[c["best"]] == 2 ** 20
        else:
            assert (S != bm.OFF_GRID).all()
        seen.add((B, wg))
    for B in (64, 65, 1024, 1025, 2049):
        assert {wg for wg in (0, 63, 64, 1023, 1024, B - 1) if wg < B} <= {w for b, w in seen if b == B}
    assert max(32 * (B - 1) + 1 for B, _, _ in ec.smax_cases()) == 65537   # beyond 32 768 poses k_beam_final's loop runs a third time


@pytest.mark.parametrize("clustered,path", [([True] * 64 + [False] * 2, 2), ([True] * 65 + [False], 2), ([False] * 65 + [True], 2), ([True] * 66, 0)])
def test_path_count_cases(clustered, path):
    c = ec.path_count_case(clustered)
    assert c["cells"].shape == (70, 130) and bm.reach_cells(c["params"], c["cpm"]) == 10 and len(c["poses"]) == 66 * 32
    wins = ec.wg_windows(c)
    assert [v[2] * v[3] <= 2048 for v in wins] == clustered
    assert ec.expected_path(c, 2048) == path
    S = ec.model_scores(c, tables(c))
    assert (S != bm.OFF_GRID).all() and len(set(S.tolist())) > 8


def test_filter_cloud():
    c = ec.filter_cloud()
    assert len(c["poses"]) == 2081 and (len(c["poses"]) + 31) // 32 == 66 and c["best"] == 2080
    S = ec.model_scores(c, tables(c))
    assert (S == bm.OFF_GRID).sum() == 3 and int(S.argmax()) == 2080
    u = bm.units(S, c["params"]["span"])
    assert sorted(set(u.tolist()))[0] == 1 and len(set(u.tolist())) == 3


# ------------------------------------------------------------------------------------------------------------------ B
@pytest.mark.parametrize("W", [128, 129, 130, 131])
def test_textured_windows(W):
    c = ec.textured_case(W)
    h, w = c["cells"].shape
    assert (h, w) == (96, W) and bm.reach_cells(c["params"], c["cpm"]) == ec.TEX_REACH and len(c["poses"]) == 12 * 32
    occ = (c["cells"] > 0).mean()
    assert 1 / 9 < occ < 1 / 6
    t = tables(c)
    S = ec.model_scores(c, t)
    assert (S != bm.OFF_GRID).all()                                          # the start cells are free and on the grid
    wins = dict(zip(c["names"], ec.wg_windows(c)))
    cc = ec.cluster_centres(W)
    pad = ec.TEX_REACH + 2
    assert sorted((cc["round%d" % k][0] - 1 - pad) & 3 for k in range(4)) == [0, 1, 2, 3]
    for k in range(4):                                                       # interior: nothing clipped; three of four left edges rounded
        x0, y0, ww, hh = wins["round%d" % k]
        cx = cc["round%d" % k][0]
        assert x0 == (cx - 1 - pad) & ~3 and x0 > 0 and x0 + ww <= W and y0 == 48 - 1 - pad and hh == 3 + 2 * pad
    assert wins["left"][0] == 0 and wins["bottom"][1] == 0 and wins["top"][1] + wins["top"][3] == 96
    x0, _, ww, _ = wins["right"]
    assert x0 + ww >= W and (x0 + ww > W) == (W % 4 != 0)                     # the columns at and beyond W are filled with 0
    for nm, ex, ey in (("bottom_left", 0, 0), ("bottom_right", 1, 0), ("top_left", 0, 1), ("top_right", 1, 1)):
        x0, y0, ww, hh = wins[nm]
        assert (x0 == 0, x0 + ww >= W, y0 == 0, y0 + hh == 96) == (ex == 0, ex == 1, ey == 0, ey == 1)
    assert all(v[2] * v[3] <= 40960 for v in wins.values()) and ec.expected_path(c, 40960) == 0
    # the texture: the cells under a window moved by one column, or by one row, change that cluster's scores
    for k, nm in enumerate(c["names"]):
        x0, y0, ww, hh = wins[nm]
        sub = dict(c, poses=c["poses"][32 * k:32 * k + 32])
        for axis in (0, 1):
            moved = c["cells"].copy()
            moved[y0:y0 + hh, x0:x0 + ww] = np.roll(moved[y0:y0 + hh, x0:x0 + ww], 1, axis=axis)
            S2 = ec.model_scores(dict(sub, cells=moved), t)
            assert (S2 != S[32 * k:32 * k + 32]).sum() >= 16, (nm, axis)
    # returns short of, at and behind the expected hit, max readings with and without one, first == K
    g = casts(c, t)
    z, zs, first, K = (np.concatenate([v[k] for v in g]) for k in ("z", "zstar", "first", "K"))
    for cond in ((z >= 0) & (zs > z), (z >= 0) & (zs == z), (zs >= 0) & (z > zs), (z < 0) & (zs >= 0), (z < 0) & (zs < 0), (z >= 0) & (first == K)):
        assert cond.sum() >= 12
    # the exact fit: the window of one interior workgroup alone
    one = ec.textured_case(W, names=["round1"])
    (x0, y0, ww, hh), = ec.wg_windows(one)
    assert ww % 4 == 0 and 16 <= ww * hh - 1 and ec.expected_path(one, ww * hh) == 0 and ec.expected_path(one, ww * hh - 1) == 1
    mixed = ec.textured_case(W, names=["round2", "top_right"], lead_off=True, tail=True)
    mw = ec.wg_windows(mixed)
    assert len(mixed["poses"]) == 97 and mw[0] is None and all(v is not None for v in mw[1:]) and ec.expected_path(mixed, 40960) == 2
    assert (ec.model_scores(mixed, t)[:32] == bm.OFF_GRID).all()


def test_textured_case_equals_the_loops():
    c = ec.textured_case(131, names=["round3", "top_right", "left"])
    equals_the_loops(c)


# ------------------------------------------------------------------------------------------------------------------ C
def test_the_reach_is_4096_cells_and_the_tables_do_not_hide_the_clamps():
    p = bm.params(**ec.LONG)
    assert bm.reach_cells(p, bc.CPM) == 4096 and bm.params_ok(p)
    far = bm.params(**dict(ec.LONG, max_range=ec.TOO_FAR))                  # float32(204.8) lies above 204.8; the float below it gives 4096
    assert bm.reach_cells(far, bc.CPM) == 4097 and bm.reach_cells(bm.params(max_range=np.nextafter(F32(ec.TOO_FAR), F32(0))), bc.CPM) == 4096
    with pytest.raises(bm.ArgError):
        bm.make_tables(far, bc.CPM)
    t = bm.make_tables(p, bc.CPM)
    assert 0 < t["short"][1023] != t["short"][1022] and 0 < t["hit"][1023] != t["hit"][1022] and t["reach"] == 4096
    d = bm.make_tables(bm.params(max_range=ec.LONG_RANGE), bc.CPM)
    assert d["short"][1022] == d["short"][1023] == 0                       # the default lambda: the clamp would not show


@pytest.mark.parametrize("W", [4104, 4103])
def test_corridor_clamps(W):
    free, wall = ec.corridor_free(W), ec.corridor_wall(W)
    assert free["cells"].shape == (5, W) and 5 * W <= 40960
    (win,) = set(ec.wg_windows(free))
    assert win == (0, 0, (W + 3) & ~3, 5) and ec.expected_path(free, 40960) == 0 and ec.expected_path(wall, 40960) == 0
    g = casts(free)
    z, zs, K = (np.concatenate([v[k] for v in g]) for k in ("z", "zstar", "K"))
    assert 4096 in K.tolist() and K.max() == 4096 and (zs < 0).all()
    assert {1022, 1023, 1024, 4000, 4095} <= set((z[z >= 0] >> 2).tolist())             # Short's index, no expected hit
    assert {16000} | {math.isqrt(16 * (dx * dx + dy * dy)) for dx, dy in ec.ROOT_CELLS} <= set(z.tolist())
    g = casts(wall)
    z, zs, K, first = (np.concatenate([v[k] for v in g]) for k in ("z", "zstar", "K", "first"))
    short = (z >= 0) & (zs > z)
    assert {1022, 1023, 1024, 4000} <= set((z[short] >> 2).tolist())                    # Short's index, z < z*
    both = (z >= 0) & (zs >= 0)
    d = np.abs(z - zs)[both]
    assert {1022, 1023, 1024} <= set(d.tolist()) and (d > 4000).sum() >= 4 and (d < 1022).any()
    assert {16356, 16360} <= set(zs.tolist()) and {4089, 4090} <= set(first.tolist())
    assert ((z < 0) & (zs >= 0)).any() and ((z < 0) & (zs < 0)).any()


@pytest.mark.parametrize("W", [4104, 4103])
def test_corridor_far_cell_is_excluded_and_the_cell_before_it_is_not(W):
    for at_far, first in ((True, 4096), (False, 4095)):
        c = ec.corridor_end(W, at_far)
        assert (c["cells"] > 0).sum() == 2 and all(0 <= x < W for x, _ in c["ends"])
        t = tables(c)
        for g in casts(c, t):
            assert g["K"].tolist() == [4096, 4096] and g["first"].tolist() == [first, first]
            assert g["zstar"].tolist() == ([-1, -1] if at_far else [4 * 4095] * 2) and g["z"].tolist() == [16000, -1]
            assert g["p"][1] == (t["max_free"] if at_far else t["max_blocked"])
            assert g["p"][0] == t["rand"] + (t["short"][1023] if at_far else t["hit"][380] + t["short"][1023])
        equals_the_loops(c)


def test_corridor_equals_the_loops():
    equals_the_loops(ec.corridor_wall(4103))
    c = ec.corridor_free(4104)
    equals_the_loops(dict(c, poses=c["poses"][[0, 4]]))


def test_square_root_at_the_largest_arguments():
    c = ec.corridor_free(4104)
    rays = bm.used_rays(c["ranges"], c["thetas"], c["params"])
    pose = c["poses"][0]
    s = bm.pose_start(pose, c["origin"], c["cpm"], 4104, 5)
    ex, ey, has = sm.endpoints(rays[0], rays[1], tuple(pose), 0, F32(0), c["origin"], c["cpm"])
    cells = list(zip((ex - s[0]).tolist(), (ey - s[1]).tolist()))
    assert has.all() and set(ec.ROOT_CELLS) <= set(cells)
    v = [16 * (dx * dx + dy * dy) for dx, dy in cells] + [16 * 4089 ** 2, 16 * 4090 ** 2, 16 * (4098 ** 2 + 4098 ** 2)]
    assert bm.isqrt(np.array(v)).tolist() == [math.isqrt(x) for x in v]
    assert math.isqrt(16 * (2400 ** 2 + 3200 ** 2)) ** 2 == 16 * (2400 ** 2 + 3200 ** 2) and max(v) < 2 ** 31
    # a float32 square root of the rounded argument, as the kernel starts from, is one too large at four of the cells and never too small
    start = {cl: int(np.sqrt(F32(16 * (cl[0] ** 2 + cl[1] ** 2)))) - math.isqrt(16 * (cl[0] ** 2 + cl[1] ** 2)) for cl in ec.ROOT_CELLS}
    assert sorted(start.values()) == [0] * 6 + [1] * 4


def test_float_square_root_is_never_too_small_within_the_contract():
    """Every pair of cells the contract allows (within reach + 2 <= 4098 of each other on each axis): the correctly rounded float32
    square root of the rounded 16 (dx^2 + dy^2), truncated, is floor(sqrt) or one more -- never less, so of the two corrections of the
    kernel's integer square root only the first can ever do work -- and it is one more at cells from 1028 cells out onwards."""
    dy = np.arange(4099, dtype=np.int64)[None, :]
    above, nearest = 0, None
    for a in range(0, 4099, 256):
        dx = np.arange(a, min(a + 256, 4099), dtype=np.int64)[:, None]
        v = 16 * (dx * dx + dy * dy)
        start = np.sqrt(v.astype(np.float32)).astype(np.int64)
        d = start - bm.isqrt(v)
        assert d.min() == 0 and d.max() <= 1 and v.max() < 2 ** 31
        above += int(d.sum())
        if d.any():
            far = np.where(d == 1, dx * dx + dy * dy, 2 ** 40).min()
            nearest = far if nearest is None else min(nearest, far)
    assert above > 6000 and nearest == 473 ** 2 + 913 ** 2


def test_every_return_scores_lg_1():
    c = ec.floor_p_case()
    t = tables(c)
    assert bm.params_ok(c["params"]) and t["rand"] == 1 and t["reach"] == 4096 and (t["hit"] == 0).all() and (t["short"] == 0).all()
    assert len(bm.used_rays(c["ranges"], c["thetas"], c["params"])[0]) == 4096 and not bm.used_rays(c["ranges"], c["thetas"], c["params"])[2].any()
    S = ec.model_scores(c, t)
    assert S.tolist() == [4096 * -30 * t["ln2"]] * 2 + [bm.OFF_GRID] and int(bm.lg(np.array([1]), t)[0]) == loop_lg(1, t) == -30 * t["ln2"]
    for span in (1, 1 << 40):
        assert bm.units(S, span).tolist() == [2 ** 20] * 2 + [1]
    d = ec.floor_p_case(max_reading=True)
    S = ec.model_scores(d, t)
    lo, hi = 4095 * -30 * t["ln2"] + loop_lg(t["max_blocked"], t), 4095 * -30 * t["ln2"] + loop_lg(t["max_free"], t)
    assert S.tolist()[:2] == [lo, hi] and lo < hi
    assert bm.units(S, 1).tolist()[:2] == [1, 2 ** 20] and bm.units(S, 1 << 40).tolist()[:2] == [2 ** 20, 2 ** 20]
    equals_the_loops(dict(d, params=bm.params(**dict(d["params"], ray_stride=64)), ranges=d["ranges"][::-1], thetas=d["thetas"][::-1]))


# ------------------------------------------------------------------------------------------------------------------ D
@pytest.mark.parametrize("w,h", [(64, 48), (37, 23)])
@pytest.mark.parametrize("origin,cpm", ec.FRAMES)
def test_frames_reach_what_conditions_reaches(w, h, origin, cpm):
    c = ec.conditions_frame(w, h, origin, cpm)
    base = bc.conditions(w, h)
    t = tables(c)
    assert t["reach"] == 30 and abs(c["mpc"] * c["cpm"] - 1) < 1e-6
    assert t["rand"] == bm.make_tables(base["params"], base["cpm"])["rand"]           # the same reach in cells
    assert bm.make_tables(c["params"], bc.CPM)["rand"] != t["rand"]                    # Rand follows the map's cells per metre
    rays = bm.used_rays(c["ranges"], c["thetas"], c["params"])
    assert len(rays[0]) == 32 + 5 and rays[2][-5:].tolist() == [False, True, False, True, True]
    seen = dict(first0=False, firstK=False, max_hit=False, max_free=False, short=False, behind=False, off=0)
    starts = []
    for pose, ref in zip(c["poses"], base["poses"]):
        starts.append(bm.pose_start(pose, c["origin"], c["cpm"], w, h))
        assert starts[-1] == bm.pose_start(ref, base["origin"], base["cpm"], w, h)   # the same cells as at the origin
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


def test_frames_equal_the_loops():
    for (origin, cpm), (w, h) in zip(ec.FRAMES[1::2], [(64, 48), (37, 23), (64, 48)]):
        equals_the_loops(ec.conditions_frame(w, h, origin, cpm))


# ------------------------------------------------------------------------------------------------------------------ E
def test_log_sweep_spans_the_exponents_and_the_mantissa_edges():
    ps = ec.log_sweep()
    assert ps[0] == 1 and ps[-1] == 2 ** 31 - 128 and {p.bit_length() - 1 for p in ps} >= {0, 1, 7, 8, 16, 23, 24, 29, 30}
    t = bm.make_tables(bm.params(), bc.CPM)
    mant = {(((p << (31 - (p.bit_length() - 1))) & 0xFFFFFFFF) >> 23) & 255 for p in ps}
    assert {0, 1, 255, 128} <= mant
    assert bm.lg(np.array(ps), t).tolist() == [loop_lg(p, t) for p in ps]
    for p in ps:
        c = ec.log_case(p)
        assert bm.params_ok(c["params"]), p
        tp = tables(c)
        assert tp["max_free"] == p == tp["max_blocked"]
        S = ec.model_scores(c, tp)
        assert S.tolist() == [loop_lg(p, tp)] * 2
        g = casts(c, tp)
        assert sorted(int(v["zstar"][0]) for v in g) == [-1, 12] and all(v["z"][0] == -1 for v in g)
    c = ec.log_case(2 ** 20, blocked_factor=2.0 ** -20)
    assert bm.params_ok(c["params"]) and tables(c)["max_blocked"] == 1 and tables(c)["max_free"] == 2 ** 20
    equals_the_loops(c)


def test_parameter_rule_at_its_boundary():
    for ok, bad in ec.boundary_params():
        assert bm.params_ok(bm.params(**ok)), ok
        assert not bm.params_ok(bm.params(**bad)), bad
        for k in ok:                                                          # neighbouring float32 values, or the named limit itself
            a, b = F32(bm.params(**ok)[k]), F32(bm.params(**bad)[k])
            assert a == b or b in (np.nextafter(a, F32(-1)), np.nextafter(a, F32(9)))
    ok_b, bad_b = ec.blocked_floor()
    zm = bm.TWO30 * bm.params()["z_max"]
    assert bm._lround(zm * ok_b) == 1 and bm._lround(zm * bad_b) == 0
