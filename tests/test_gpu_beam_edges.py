"""The beam model on the device against its model on the cases of tests/beam_edge_cases.py: k_beam_final beyond its
first wave, staged windows inside a textured grid, walks of 4096 cells with the table clamps, other frames, the logarithm over p's
range and bl_beam_set_params at its boundary.  Every comparison is equality, on the library's own tables."""
import numpy as np
import pytest

import botlab_amd as bl
import beam_cases as bc
import beam_edge_cases as ec
import beam_model as bm
from test_gpu_beam import KEYS, beam_of, check, grid_of, same_tables, scan_of

pytestmark = pytest.mark.gpu
F32 = np.float32
COLS = ("first", "K", "z", "zstar", "p")


def set_params(beam, p):
    beam.setParams(**{k: p[k] for k in KEYS})


def compare(beam, grid, c, path=None, casts=(), exp=None):
    """test_gpu_beam.check with the model's scores formed once per distinct pose (and the rays in chunks): tables, scores, path,
    units and debug_cast of the poses `casts`.  exp: the model's scores where a test has them already (they do not depend on span).
    Returns (scores, units)."""
    t = beam.tables(c["cpm"])
    same_tables(t, bm.make_tables(c["params"], c["cpm"]))
    exp = ec.model_scores(c, t) if exp is None else exp
    got = beam.scores(grid, scan_of(c), c["poses"])
    bad = np.flatnonzero(got != exp)
    assert len(bad) == 0, (len(bad), int(bad[0]), int(got[bad[0]]), int(exp[bad[0]]))
    if path is not None:
        assert beam.debugPath() == path
    u = beam.units(len(c["poses"]))
    want = bm.units(exp, c["params"]["span"], bl.BeamModel.unitTable())
    bad = np.flatnonzero(u != want)
    assert len(bad) == 0, (len(bad), int(bad[0]), int(u[bad[0]]), int(want[bad[0]]))
    rays = bm.used_rays(c["ranges"], c["thetas"], c["params"])
    for i in casts:
        g = beam.debug_cast(grid, scan_of(c), c["poses"][i])
        e = bm.cast(c["cells"], c["origin"], c["cpm"], rays, c["poses"][i], c["params"], t)
        for col in COLS:
            assert np.array_equal(g[col], e[col]), (i, col, g[col].tolist(), e[col].tolist())
    return got, u


def both_paths(ctx, c, casts=(), staged_path=0, window_bytes=0):
    """The case read directly (the default) and with staging on; the same scores both times."""
    beam, grid = beam_of(ctx, c), grid_of(ctx, c)
    try:
        a, _ = compare(beam, grid, c, path=1, casts=casts)
        beam.debugSet(stage_windows=True, window_bytes=window_bytes)
        b, _ = compare(beam, grid, c, path=staged_path, casts=casts)
        assert np.array_equal(a, b)
        return a
    finally:
        beam.close()
        grid.close()


# ------------------------------------------------------------------------------------------------------------------ A
@pytest.mark.parametrize("B", [64, 65, 1024, 1025, 2049])
def test_smax_from_any_workgroup(gpu_ctx, B):
    cases = [v for v in ec.smax_cases() if v[0] == B and not v[2]]
    c = ec.smax_case(*cases[0])
    beam, grid = beam_of(gpu_ctx, c), grid_of(gpu_ctx, c)
    mid = int(bl.BeamModel.unitTable()[128])
    try:
        for v in cases:
            c = ec.smax_case(*v)
            s, u = compare(beam, grid, c, path=1)
            assert int(s.argmax()) == c["best"] and u[c["best"]] == 2 ** 20 and (np.delete(u, c["best"]) == mid).all(), v
    finally:
        beam.close()
        grid.close()


@pytest.mark.parametrize("B", [65, 1025])
def test_smax_behind_workgroups_of_off_grid_poses(gpu_ctx, B):
    cases = [v for v in ec.smax_cases() if v[0] == B and v[2]]
    c = ec.smax_case(*cases[0])
    beam, grid = beam_of(gpu_ctx, c), grid_of(gpu_ctx, c)
    try:
        for v in cases:
            c = ec.smax_case(*v)
            s, u = compare(beam, grid, c, path=1)
            at = c["best"]
            assert (s[:at] == bm.OFF_GRID).all() and (u[:at] == 1).all() and u[at] == 2 ** 20 and (u[at + 1:] > 1).all(), v
    finally:
        beam.close()
        grid.close()


@pytest.mark.parametrize("clustered,path", [([True] * 64 + [False] * 2, 2), ([True] * 65 + [False], 2), ([False] * 65 + [True], 2), ([True] * 66, 0)])
def test_path_counts_beyond_the_first_wave(gpu_ctx, clustered, path):
    c = ec.path_count_case(clustered)
    assert ec.expected_path(c, 2048) == path
    beam, grid = beam_of(gpu_ctx, c), grid_of(gpu_ctx, c)
    try:
        beam.debugSet(stage_windows=True, window_bytes=2048)
        compare(beam, grid, c, path=path, casts=[0, 65 * 32 + 1])
    finally:
        beam.close()
        grid.close()


def test_reweigh_a_filter_of_66_workgroups(gpu_ctx):
    c = ec.filter_cloud()
    n = len(c["poses"])
    beam, grid, pf = beam_of(gpu_ctx, c), grid_of(gpu_ctx, c), bl.ParticleFilter(n, ctx=gpu_ctx)
    try:
        cloud = np.zeros(n, bl.PARTICLE_DTYPE)
        for k, f in enumerate(("x", "y", "theta")):
            cloud[f] = cloud["p_" + f] = c["poses"][:, k]
        cloud["utime"] = cloud["p_utime"] = 1_000_000
        cloud["weight"] = 1.0 / n
        pf.setParticles(cloud)
        pf.reweigh_beam(beam, grid, scan_of(c))
        S = ec.model_scores(c, beam.tables(c["cpm"]))
        u = bm.units(S, c["params"]["span"], bl.BeamModel.unitTable())
        assert u[2080] == 2 ** 20 and (u == 2 ** 20).sum() == 1 and (u == 1).sum() == 3
        assert np.array_equal(beam.units(n), u) and beam.debugPath() == 1
        after = pf.particles()
        assert np.array_equal(after["weight"], u.astype(np.float64) / float(u.astype(np.uint64).sum()))
        for f in ("x", "y", "theta"):
            assert after[f].tobytes() == cloud[f].tobytes()
    finally:
        pf.close()
        beam.close()
        grid.close()


# ------------------------------------------------------------------------------------------------------------------ B
@pytest.mark.parametrize("W", [128, 129, 130, 131])
def test_windows_inside_a_textured_grid(gpu_ctx, W):
    c = ec.textured_case(W)
    assert ec.expected_path(c, 40960) == 0
    both_paths(gpu_ctx, c, casts=[32 * k + 4 for k in range(len(c["names"]))])


@pytest.mark.parametrize("W", [128, 129, 130, 131])
def test_window_that_fits_exactly_and_one_byte_short(gpu_ctx, W):
    c = ec.textured_case(W, names=["round1"])
    (_, _, w, h), = ec.wg_windows(c)
    a = both_paths(gpu_ctx, c, window_bytes=w * h, staged_path=0)
    b = both_paths(gpu_ctx, c, window_bytes=w * h - 1, staged_path=1)
    assert np.array_equal(a, b)


@pytest.mark.parametrize("W", [128, 131])
def test_empty_box_two_windows_and_a_last_workgroup_of_one_pose(gpu_ctx, W):
    c = ec.textured_case(W, names=["round2", "top_right"], lead_off=True, tail=True)
    s = both_paths(gpu_ctx, c, staged_path=2, casts=[36, 96])
    assert (s[:32] == bm.OFF_GRID).all() and (s[32:] != bm.OFF_GRID).all()


# ------------------------------------------------------------------------------------------------------------------ C
@pytest.mark.parametrize("W", [4104, 4103])
@pytest.mark.parametrize("make", [ec.corridor_free, ec.corridor_wall], ids=["free", "wall"])
def test_walks_of_4096_cells_and_the_table_clamps(gpu_ctx, W, make):
    c = make(W)
    both_paths(gpu_ctx, c, casts=range(len(c["poses"])))


@pytest.mark.parametrize("W", [4104, 4103])
@pytest.mark.parametrize("at_far_cell", [True, False])
def test_far_cell_excluded_from_the_walk(gpu_ctx, W, at_far_cell):
    c = ec.corridor_end(W, at_far_cell)
    both_paths(gpu_ctx, c, casts=[0, 1])


def test_reach_of_4097_cells_refused(gpu_ctx):
    c = ec.corridor_free(4103)
    far = dict(c, params=bm.params(**dict(c["params"], max_range=ec.TOO_FAR)))
    beam, grid = beam_of(gpu_ctx, far), grid_of(gpu_ctx, c)
    try:
        with pytest.raises(bl.BotlabHipError, match="status 2"):
            beam.scores(grid, scan_of(c), c["poses"])
        with pytest.raises(bl.BotlabHipError, match="status 2"):
            beam.tables(c["cpm"])
        set_params(beam, bm.params(**dict(c["params"], max_range=np.nextafter(F32(ec.TOO_FAR), F32(0)))))
        assert beam.tables(c["cpm"])["reach"] == 4096
    finally:
        beam.close()
        grid.close()


def test_the_most_negative_score(gpu_ctx):
    c, e = ec.floor_p_case(), ec.floor_p_case(max_reading=True)
    beam, grid = beam_of(gpu_ctx, c), grid_of(gpu_ctx, c)
    try:
        t = beam.tables(c["cpm"])
        exp_c, exp_e = ec.model_scores(c, t), ec.model_scores(e, t)
        for span in (1, 1 << 40):
            prm = bm.params(**dict(c["params"], span=span))
            set_params(beam, prm)
            s, u = compare(beam, grid, dict(c, params=prm), path=1, exp=exp_c)
            assert s.tolist() == [4096 * -30 * 45426] * 2 + [bm.OFF_GRID] and u.tolist() == [2 ** 20] * 2 + [1]
            s, u = compare(beam, grid, dict(e, params=prm), path=1, exp=exp_e)
            assert s[0] < s[1] and u.tolist() == ([1, 2 ** 20, 1] if span == 1 else [2 ** 20, 2 ** 20, 1])
        beam.debugSet(stage_windows=True)
        compare(beam, grid, dict(c, params=prm), path=0, exp=exp_c)
    finally:
        beam.close()
        grid.close()


# ------------------------------------------------------------------------------------------------------------------ D
@pytest.mark.parametrize("w,h", [(64, 48), (37, 23)])
@pytest.mark.parametrize("origin,cpm", ec.FRAMES)
def test_other_frames(gpu_ctx, w, h, origin, cpm):
    c = ec.conditions_frame(w, h, origin, cpm)
    a, _ = check(gpu_ctx, c, casts=range(len(c["poses"])), path=1)
    assert (a == bm.OFF_GRID).sum() == 4 and a[0] == a[9]
    beam = beam_of(gpu_ctx, c)
    try:
        assert beam.tables(c["cpm"])["rand"] != beam.tables(bc.CPM)["rand"]
        beam.debugSet(stage_windows=True)
        b, _ = check(gpu_ctx, c, casts=range(len(c["poses"])), path=0, beam=beam)
        assert np.array_equal(a, b)
    finally:
        beam.close()


# ------------------------------------------------------------------------------------------------------------------ E
def test_logarithm_over_the_range_of_p(gpu_ctx):
    from test_beam_model_cpu import loop_lg
    c = ec.log_case(1)
    beam, grid = beam_of(gpu_ctx, c), grid_of(gpu_ctx, c)
    try:
        for p in ec.log_sweep():
            c = ec.log_case(p)
            set_params(beam, c["params"])
            t = beam.tables(c["cpm"])
            assert t["max_free"] == p == t["max_blocked"]
            s, _ = compare(beam, grid, c, path=1, casts=[0, 1])
            assert s.tolist() == [loop_lg(p, t)] * 2, p
        c = ec.log_case(2 ** 20, blocked_factor=2.0 ** -20)                   # MaxBlocked = 1 beside MaxFree = 2^20
        set_params(beam, c["params"])
        t = beam.tables(c["cpm"])
        assert (t["max_free"], t["max_blocked"]) == (2 ** 20, 1)
        s, u = compare(beam, grid, c, path=1, casts=[0, 1])
        assert s.tolist() == [loop_lg(2 ** 20, t), -30 * t["ln2"]]
    finally:
        beam.close()
        grid.close()


def test_set_params_at_the_boundary_of_the_two_conditions_on_p(gpu_ctx):
    base = bm.params()
    beam = bl.BeamModel(ctx=gpu_ctx, **{k: base[k] for k in KEYS})
    try:
        for ok, bad in ec.boundary_params():
            good = bm.params(**ok)
            assert bm.params_ok(good) and not bm.params_ok(bm.params(**bad))
            set_params(beam, good)
            before = beam.tables(bc.CPM)
            same_tables(before, bm.make_tables(good, bc.CPM))
            with pytest.raises(bl.BotlabHipError, match="status 2"):
                set_params(beam, bm.params(**bad))
            same_tables(beam.tables(bc.CPM), before)                          # the handle keeps what it had
        ok_b, _ = ec.blocked_floor()
        set_params(beam, bm.params(blocked_factor=ok_b))
        assert beam.tables(bc.CPM)["max_blocked"] == 1
    finally:
        beam.close()
