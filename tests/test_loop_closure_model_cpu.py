"""The loop-closure model and its named cases, without a GPU (tests/loop_closure_model.py, tests/loop_closure_cases.py).

Every case reaches the path it is named for, on the model; over the case set the model yields kept edges and candidates with every
rejecting flag, so no comparison of the device with the model can pass vacuously.  The stated edge arithmetic (cofactor inverse, one-step
wrap, float sine and cosine widened) is measured against the formulation of botlab_amd.find_loop_closures (np.linalg.inv,
atan2(sin, cos), libm's double sine and cosine).

Measured over the 128 kept edges of the case set: info differs by at most 1.44e-8 of the edge's largest information entry (the 1.25 cm
case, whose quantisation term is the smallest; 4.2e-9 over the 127 edges at 5 cm), z by at most 2.5e-8 (the float sine and cosine of theta_j, relative error 6e-8, times offsets of up to 0.5 m).  The bounds are four times that, as
DESIGN.md 4.32 did for its dense solve: a rounding difference between two formulations in double, not a tuning number."""
import time

import numpy as np
import pytest

import loop_closure_cases as lcc
import loop_closure_model as lcm

INFO_REL_BOUND, Z_ABS_BOUND = lcc.INFO_REL_BOUND, lcc.Z_ABS_BOUND


@pytest.mark.parametrize("name", list(lcc.cases()))
def test_case_reaches_its_path(name):
    case = lcc.cases()[name]
    assert lcm.check_params(case.params)
    assert case.reaches(lcc.model(name)), name


assert list(lcc.edge_cases()) == ["long_log", "tie_same_lane", "tie_lane_order", "tie_three"]


@pytest.mark.parametrize("name", list(lcc.edge_cases()))
def test_edge_case_reaches_its_path(name):
    case = lcc.edge_cases()[name]
    assert lcm.check_params(case.params)
    t = time.time()
    m = lcc.model(name)
    kept = sum(c["flags"] == 0 for c in m)
    print(name, "model seconds %.2f" % (time.time() - t), "queries", -(-len(case.scans) // case.params["stride"]), "candidates", len(m), "kept", kept)
    assert case.reaches(m), name


def test_long_log_edges_against_the_python_formulation():
    """the kept edges of long_log within the bounds the case set has"""
    case = lcc.edge_cases()["long_log"]
    _, poses = case.retained()
    worst_info, worst_z, n = 0.0, 0.0, 0
    for c in lcc.model("long_log"):
        if c["flags"]:
            continue
        centre = tuple(np.float32(v) for v in poses[c["q"]][:3])
        z, info = lcm.edge_reference(c["ref"], centre, poses[c["j"]], case.mpc, case.params["dtheta"])
        info, z = np.array(info), np.array(z)
        worst_info = max(worst_info, float(np.abs(info - np.array(c["info"])).max() / np.abs(info).max()))
        worst_z = max(worst_z, float(np.abs(z - np.array(c["z"])).max()))
        n += 1
    print("long_log kept edges", n, "largest relative difference of info", worst_info, "largest absolute difference of z", worst_z)
    assert n >= 2
    assert worst_info <= INFO_REL_BOUND and worst_z <= Z_ABS_BOUND


def test_case_set_is_not_vacuous():
    kept, flags = 0, {lcm.NOT_ACCEPTED: 0, lcm.TIED: 0, lcm.ON_EDGE: 0, lcm.TOO_MANY_RAYS: 0}
    for name in lcc.cases():
        for c in lcc.model(name):
            kept += c["flags"] == 0
            for f in flags:
                flags[f] += bool(c["flags"] & f)
    print("kept edges", kept, "flagged", flags)
    assert kept >= 3
    assert all(v >= 1 for v in flags.values()), flags
    assert set(lcc.SECOND_FIND) <= set(lcc.cases()) and len(lcc.model(lcc.SECOND_FIND[0])) > len(lcc.model(lcc.SECOND_FIND[1])) >= 1


@pytest.mark.parametrize("name", ["two_lap", "equal_d2", "at_radius", "beyond_radius", "cut_end", "wrapped_ring"])
def test_pair_rule_is_find_loop_closures(name):
    """the restated loop against the numpy statements of botlab_amd.find_loop_closures"""
    case = lcc.cases()[name]
    _, poses = case.retained()
    p = case.params
    px = np.array([q[0] for q in poses], np.float32).astype(np.float64)
    py = np.array([q[1] for q in poses], np.float32).astype(np.float64)
    radius = float(np.float32(p["radius"]))
    want = []
    for q in range(0, len(poses), p["stride"]):
        last = q - p["min_gap"] - 1
        if last < 0:
            continue
        d2 = (px[:last + 1] - px[q]) ** 2 + (py[:last + 1] - py[q]) ** 2
        j = int(np.argmin(d2))
        if d2[j] > radius * radius:
            continue
        want.append((q, j))
    assert lcm.pairs(poses, p["stride"], p["min_gap"], p["radius"]) == want
    assert [(c["q"], c["j"]) for c in lcc.model(name)] == want


def test_submap_frame_and_records():
    m = lcc.model("cut_start")
    rec = lcm.records(m)
    assert rec.dtype.itemsize == 272 and len(rec) == len(m)
    for c, r in zip(m, rec):
        assert c["cells"].shape == (65, 65) and c["cells"].dtype == np.int8
        half = np.float32(65 * float(np.float32(lcc.MPC)) / 2.0)
        _, poses = lcc.cases()["cut_start"].retained()
        assert c["origin"] == (np.float32(poses[c["j"]][0]) - half, np.float32(poses[c["j"]][1]) - half)
        assert (r["flags"] == 0) == (c["z"] is not None)
        if c["flags"] == 0:
            assert r["edge"]["i"] == c["j"] and r["edge"]["j"] == c["q"] and np.isfinite(r["edge"]["info"]).all()
        else:
            assert not r["edge"].tobytes().strip(b"\0")
    assert len(lcm.edges(m)) == sum(c["flags"] == 0 for c in m)


def test_stated_edge_against_the_python_formulation():
    worst_info, worst_z, n = 0.0, 0.0, 0
    for name, case in lcc.cases().items():
        _, poses = case.retained()
        for c in lcc.model(name):
            if c["flags"]:
                continue
            centre = tuple(np.float32(v) for v in poses[c["q"]][:3])
            z, info = lcm.edge_reference(c["ref"], centre, poses[c["j"]], case.mpc, case.params["dtheta"])
            info, z = np.array(info), np.array(z)
            worst_info = max(worst_info, float(np.abs(info - np.array(c["info"])).max() / np.abs(info).max()))
            worst_z = max(worst_z, float(np.abs(z - np.array(c["z"])).max()))
            n += 1
            # the information matrix is symmetric positive definite
            I = np.array([[c["info"][0], c["info"][1], c["info"][3]], [c["info"][1], c["info"][2], c["info"][4]], [c["info"][3], c["info"][4], c["info"][5]]])
            assert np.linalg.eigvalsh(I).min() > 0
    print("kept edges", n, "largest relative difference of info", worst_info, "largest absolute difference of z", worst_z)
    assert n >= 3
    assert worst_info <= INFO_REL_BOUND and worst_z <= Z_ABS_BOUND


def test_refusals_of_the_parameter_check():
    ok = dict(lcm.DEFAULTS)
    assert lcm.check_params(ok)
    for bad in (dict(stride=0), dict(min_gap=-1), dict(radius=0.0), dict(radius=float("nan")), dict(w=32), dict(w=-1), dict(submap_cells=15),
                dict(submap_cells=513), dict(hitOdds=-1), dict(missOdds=128), dict(nx=65), dict(ntheta=181), dict(dtheta=0.0), dict(half_life=0),
                dict(half_life=(1 << 20) + 1), dict(prior=(1, 2, 1, 0)), dict(prior=(-1, 0, 0, 0))):
        assert not lcm.check_params(dict(ok, **bad)), bad
