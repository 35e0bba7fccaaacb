"""The likelihood field's model (tests/likelihood_field_model.py) against an independent brute-force form, the ends of its table, and
the premise of the feature: on the shipped maps a pose's scan score is a needle on the raw map and a smooth, unimodal hill on the
field.  No GPU, no library call."""
import os
import sys

import numpy as np
import pytest

import helpers
import likelihood_field_model as lm
import scan_match_model as sm

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import sim_lidar  # noqa: E402

MPC = np.float32(0.05)


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_model_equals_all_pairs_brute_force(seed):
    rng = np.random.default_rng(seed)
    density = (0.005, 0.03, 0.2, 0.6)[seed - 1]
    cells = np.where(rng.random((20, 23)) < density, rng.integers(1, 128, (20, 23)), rng.integers(-128, 1, (20, 23))).astype(np.int8)
    for R, occ_min, peak, sigma in ((1, 1, 127, 0.1), (3, 1, 127, 0.1), (6, 40, 100, 0.1), (30, 1, 127, 0.4), (64, 1, 1, 0.3)):
        assert not lm.near_half(sigma, R, MPC, peak)
        got, exp = lm.field(cells, sigma, R, MPC, occ_min, peak), lm.brute_force(cells, sigma, R, MPC, occ_min, peak)
        assert got.dtype == np.int8 and np.array_equal(got, exp), (seed, R, occ_min, peak)
        assert got.min() >= 0 and got.max() <= peak
        if lm.table(sigma, R, MPC, peak)[1] < peak:
            assert np.array_equal(got == peak, cells >= occ_min)


def test_sources_are_log_odds_at_least_occ_min_never_zero_or_negative():
    cells = np.array([[0, -1, 5, 6, -128, 127]], np.int8)
    assert np.array_equal(lm.codes(cells, 1, 1)[0], [2, 1, 0, 0, 1, 0])
    assert np.array_equal(lm.codes(cells, 1, 6)[0], [2, 2, 1, 0, 1, 0])
    assert np.array_equal(lm.codes(cells, 1, 127)[0], [2, 2, 2, 2, 1, 0])
    none = np.zeros((3, 4), np.int8)
    assert (lm.codes(none, 5, 1) == 26).all() and (lm.field(none, 0.1, 5, MPC) == 0).all()


def test_table_ends_and_the_quoted_entries():
    t = lm.table(0.1, 6, MPC, 127)
    assert t.dtype == np.int8 and len(t) == 38 and not lm.near_half(0.1, 6, MPC, 127)
    assert t[:12].tolist() == [127, 112, 99, 87, 77, 68, 60, 53, 47, 41, 36, 32] and t[36] == 1 and t[37] == 0
    assert (np.diff(t.astype(int)) <= 0).all()
    for peak in (1, 50, 127):
        for R in (1, 6, 64):
            t = lm.table(0.1, R, MPC, peak)
            assert len(t) == R * R + 2 and t[0] == peak and t[lm.far(R)] == 0


def test_narrow_sigma_marks_the_sources_only():
    rng = np.random.default_rng(7)
    cells = np.where(rng.random((20, 23)) < 0.05, 90, -20).astype(np.int8)
    t = lm.table(0.01, 6, MPC, 127)
    assert t[0] == 127 and t[1] == 0 and not lm.near_half(0.01, 6, MPC, 127)
    assert np.array_equal(lm.field(cells, 0.01, 6, MPC), np.where(cells >= 1, 127, 0))


def test_wide_sigma_is_a_disc_indicator():
    """sigma = 10 m: every T[k <= R^2] is the peak, so the field is peak within R cells of a source and 0 beyond -- the FAR edge."""
    R = 6
    t = lm.table(10.0, R, MPC, 127)
    assert (t[:R * R + 1] == 127).all() and t[R * R + 1] == 0 and not lm.near_half(10.0, R, MPC, 127)
    cells = np.full((20, 23), -20, np.int8)
    cells[9, 11] = 100
    yy, xx = np.mgrid[0:20, 0:23]
    disc = (yy - 9) ** 2 + (xx - 11) ** 2 <= R * R
    f = lm.field(cells, 10.0, R, MPC)
    assert np.array_equal(f, np.where(disc, 127, 0)) and f[9, 17] == 127 and f[9, 18] == 0 and f[3, 11] == 127 and f[2, 11] == 0


def _profile(cells, m, ranges, thetas):
    vol = sm.score_volume(cells, m["origin"], helpers.CPM_DEFAULT, ranges, thetas, (0.0, 0.0, 0.3), 8, 0, 0, 0.01)
    return vol[0, 0].astype(np.int64)


@pytest.mark.parametrize("name", ["obstacle_slam_10mx10m_5cm", "convex_10mx10m_5cm"])
def test_premise_needle_on_the_map_hill_on_the_field(maps, name):
    """A 290-ray scan cast from (0, 0, 0.3), scored with the pose shifted by -8 .. +8 cells in x."""
    m = maps[name]
    world = sim_lidar.Map(m["cells"], m["origin"][0], m["origin"][1], m["mpc"])
    th, rg, _ = sim_lidar.scan(world, lambda t: (0.0, 0.0, 0.3), 1.0)
    ranges, thetas = sm.valid_rays(np.array(rg, np.float32), np.array(th, np.float32), 100.0)
    assert len(ranges) == 290
    raw = _profile(m["cells"], m, ranges, thetas)
    assert not lm.near_half(0.1, 6, m["mpc"], 127)
    fld = _profile(lm.field(m["cells"], 0.1, 6, m["mpc"]), m, ranges, thetas)
    assert len(raw) == len(fld) == 17
    # the field: strictly up to shift 0, strictly down after it
    assert (np.diff(fld[:9]) > 0).all() and (np.diff(fld[8:]) < 0).all()
    # the raw map: the maximum is at shift 0 too, but the profile is no hill.  (On the convex map neither flank is monotone; on the
    # obstacle map the left flank is not -- 5708 5472 4993 5190 -- while the right one happens to fall all the way.)
    assert int(np.argmax(raw)) == 8 and (raw[8] > np.delete(raw, 8)).all()
    left, right = bool((np.diff(raw[:9]) >= 0).all()), bool((np.diff(raw[8:]) <= 0).all())
    assert not left
    assert not right or name == "obstacle_slam_10mx10m_5cm"
