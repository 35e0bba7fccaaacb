"""The numpy model of bl_pf_clusters (tests/pf_cluster_model.py) against itself and against plain float64: the union-find
components equal a brute-force search over every pair of bins on every hand-built cloud (tests/pf_cluster_cases.py); the pose
helper -- the model's and the header's own bl_pf_cluster_pose, which the library exports -- equals a float64 weighted mean and
covariance of the fine coordinates; and the wide case really passes 2^64."""
import ctypes as C
import math

import numpy as np
import pytest

import pf_cluster_cases as cases
import pf_cluster_model as pm
from botlab_amd import _capi

CASES = cases.all_cases()


def _model(c, finder=pm.components_union_find):
    return pm.clusters(c["x"], c["y"], c["th"], c["units"], c["bin_xy"], c["T"], c["K"], finder=finder)


def _strip(r):
    return [{k: v for k, v in c.items() if k != "bins"} for c in r["clusters"]]


@pytest.mark.parametrize("name", sorted(CASES))
def test_union_find_equals_brute_force(name):
    c = CASES[name]
    a, b = _model(c), _model(c, pm.components_brute_force)
    assert a["num_clusters"] == b["num_clusters"] and a["units_sum"] == b["units_sum"] and a["active"] == b["active"] == len(c["x"])
    assert _strip(a) == _strip(b)
    assert np.array_equal(a["labels"], b["labels"])
    assert sum(k["count"] for k in a["clusters"]) == len(c["x"]) and sum(k["units"] for k in a["clusters"]) == a["units_sum"]


def test_cases_are_what_they_say():
    n = {k: _model(v) for k, v in CASES.items()}
    for size in cases.LAUNCH_SIZES:
        assert n["one_bin_%d" % size]["num_clusters"] == 1
        assert n["isolated_%d" % size]["num_clusters"] == size
    assert n["snake"]["num_clusters"] == 1 and n["two_snakes"]["num_clusters"] == 2 and n["ring"]["num_clusters"] == 2
    assert n["wrap_35"]["num_clusters"] == 1 and n["wrap_34"]["num_clusters"] == 2
    assert n["T1"]["num_clusters"] == 2 and n["K1"]["num_clusters"] == 3 and n["C100"]["num_clusters"] == 100
    assert (n["C100"]["labels"] == -1).sum() == 92
    b = n["bridges"]
    assert b["num_clusters"] == 3 and [c["units"] for c in b["clusters"]] == [45, 4, 0] and b["clusters"][0]["count"] == 8
    assert pm.cluster_pose(b["clusters"][2], b["units_sum"], cases.BIN) is None
    # the heading terms stop at |theta| = 100: the four particles from there on, the NaN and the infinities add none
    px, py, it, si, ci = pm.particle_terms(CASES["heading_values"]["x"], CASES["heading_values"]["y"], CASES["heading_values"]["th"], cases.BIN, 36)
    assert [int(v) for v in (np.abs(si) + np.abs(ci) != 0)] == [1, 1, 1, 1, 1, 0, 0, 1, 0, 0, 0, 0]
    # floor, not truncation; clamps; NaN at the lower clamp
    px = pm.particle_terms(CASES["position_edges"]["x"], CASES["position_edges"]["y"], CASES["position_edges"]["th"], cases.BIN, 36)[0]
    assert [int(v) >> 10 for v in px] == [0, 1, -2, -1, -1, 0, 0, -1, 0, 2 ** 20 - 1, -2 ** 20, 2 ** 20 - 1, -2 ** 20, -2 ** 20, 2 ** 20 - 1, -2 ** 20]


def _float64_moments(c, members):
    px, py, it, si, ci = pm.particle_terms(c["x"], c["y"], c["th"], c["bin_xy"], c["T"])
    u = c["units"][members].astype(np.float64)
    fx, fy = px[members].astype(np.float64), py[members].astype(np.float64)
    s = 1024.0 / c["bin_xy"]
    mx, my = np.sum(u * fx) / u.sum(), np.sum(u * fy) / u.sum()
    return ((mx + 0.5) / s, (my + 0.5) / s, np.sum(u * (fx - mx) ** 2) / u.sum() / s ** 2, np.sum(u * (fy - my) ** 2) / u.sum() / s ** 2,
            np.sum(u * (fx - mx) * (fy - my)) / u.sum() / s ** 2)


def _c_pose(cl, units_sum, bin_xy, T):
    raw = _capi.PfCluster()
    raw.count, raw.units = cl["count"], cl["units"]
    for n in pm.SUMS:
        v = cl[n] & ((1 << 128) - 1)
        getattr(raw, n).lo = v & ((1 << 64) - 1)
        getattr(raw, n).hi = (v >> 64) - (1 << 64 if v >> 127 else 0)
    raw.anchor_ix, raw.anchor_iy, raw.anchor_it = cl["anchor"]
    p = _capi.PfClusterParams(float(bin_xy), T, 1)
    out = _capi.PfClusterPose()
    if not _capi.load().bl_pf_cluster_pose(C.byref(raw), C.c_uint64(units_sum), C.byref(p), C.byref(out)):
        return None
    return {f: getattr(out, f) for f, _ in _capi.PfClusterPose._fields_}


@pytest.mark.parametrize("name", ["one_bin_1025", "big_units", "bimodal", "snake"])
def test_pose_helper_equals_float64_moments(name):
    c = CASES[name]
    r = _model(c)
    cl = r["clusters"][0]
    members = np.flatnonzero(r["labels"] == 0)
    ref = _float64_moments(c, members)
    mine = pm.cluster_pose(cl, r["units_sum"], c["bin_xy"])
    assert mine == _c_pose(cl, r["units_sum"], c["bin_xy"], c["T"])           # the header's code, the same doubles
    got = (mine["mean_x"], mine["mean_y"], mine["var_x"], mine["var_y"], mine["cov_xy"])
    for g, e in zip(got, ref):
        assert abs(g - e) <= 1e-9 * max(abs(e), 1e-300), (name, got, ref)
    assert mine["share"] == cl["units"] / r["units_sum"]
    assert 0.0 <= mine["theta_resultant"] <= 1.0 + 1e-6


def test_bimodal_share_and_pose():
    c = CASES["bimodal"]
    r = _model(c)
    a = r["clusters"][0]
    assert (a["units"], r["units_sum"], a["count"]) == (7000, 10000, 1400)
    p = pm.cluster_pose(a, r["units_sum"], c["bin_xy"])
    assert p["share"] == 0.7
    assert abs(p["mean_x"] - 1.0) < 0.01 and abs(p["mean_y"] - 2.0) < 0.01 and abs(p["theta"] - 0.5) < 0.01


def test_zero_unit_cluster_has_no_pose_in_the_header_either():
    r = _model(CASES["bridges"])
    assert _c_pose(r["clusters"][2], r["units_sum"], cases.BIN, 36) is None


def test_wide_case_passes_64_bits():
    r = _model(CASES["big_units"])
    cl = r["clusters"][0]
    assert r["num_clusters"] == 1 and cl["count"] == 4097
    assert cl["sx"] > 2 ** 64 and cl["sxx"] > 2 ** 90 and cl["syy"] > 2 ** 90 and cl["sxy"] > 2 ** 90
    # and relative to a bin's corner one bin's share of the squares passes 2^64 for 10^6 such particles: 2^32 * 1023^2 * 2^20
    assert (2 ** 32 - 1) * 1023 ** 2 * 10 ** 6 > 2 ** 64
