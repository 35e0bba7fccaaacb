"""The model of loop closure by place recognition (tests/place_model.py) without a GPU: every named case takes the path
it is named for; the sign of the shift against synthetic truth; the matrix-product form of the best pairs against the definition as it
is written; the drift case's three conditions; every flag of the gate somewhere in the set."""
import math

import numpy as np
import pytest

from botlab_amd import synth

import loop_closure_cases as lcc
import loop_closure_model as lcm
import place_cases as pc
import place_model as pm

NAMES = list(pc.cases())


@pytest.mark.parametrize("name", NAMES)
def test_case_reaches_its_path(name):
    m = pc.model(name)
    assert pc.cases()[name].reaches(m), [tuple(p) for p in m[2]]
    assert [c["q"] for c in m[3]] == [int(p["q"]) for p in m[2] if p["partner"] >= 0]


def test_long_case_reaches_its_path():
    m = pc.model("long_log")
    assert pc.long_case().reaches(m)


@pytest.mark.parametrize("turn", [1.0, -1.0, 2.5, math.radians(100.0), math.radians(-37.0)])
def test_sign_of_the_shift(turn):
    """two scans from one spot, the query's heading `turn` ahead of the partner's: the descriptors line up at
    s = turn * 64 / (2 pi) modulo 64, and the centre's heading is the query's within two sectors"""
    w = lcc.world()
    spot, tj = (0.3, -0.2), 0.4
    sj = synth.raycast_scan(w, pc.ORIGIN, pc.MPC, (spot[0], spot[1], tj), (spot[0], spot[1], tj), 1000)
    sq = synth.raycast_scan(w, pc.ORIGIN, pc.MPC, (spot[0], spot[1], tj + turn), (spot[0], spot[1], tj + turn), 2000)
    d, bits = pm.descriptors([sj, sq], 4.0, 8.0)
    pl = pm.best(d, bits, 1, 0, 1, 0, 0)[1]
    assert pl["q"] == 1 and pl["j"] == 0
    want = turn * 64 / (2 * math.pi)
    off = (int(pl["shift"]) - want) % 64
    print("turn", turn, "shift", int(pl["shift"]), "expected", want % 64, "key", int(pl["key"]))
    assert min(off, 64 - off) <= 1.0
    c = pm.centre((np.float32(spot[0]), np.float32(spot[1]), np.float32(tj)), int(pl["shift"]))
    assert abs(math.remainder(float(c[2]) - (tj + turn), 2 * math.pi)) <= 2 * float(pm.STEP)


def test_constants_and_centre():
    assert pm.K == np.float32(32 / math.pi) and pm.STEP == np.float32(2 * math.pi / 64)
    pj = (np.float32(1.25), np.float32(-0.5), np.float32(3.0))
    assert pm.centre(pj, 0) == (pj[0], pj[1], pj[2])
    assert pm.centre(pj, 31)[2] == np.float32(np.float32(3.0) + np.float32(np.float32(31.0) * pm.STEP)) > np.float32(math.pi)
    assert pm.centre(pj, 32)[2] == np.float32(np.float32(3.0) + np.float32(np.float32(-32.0) * pm.STEP))
    assert pm.centre(pj, 63)[2] == np.float32(np.float32(3.0) - pm.STEP)
    # the product and the sum rounded one by one: not the double sum rounded once
    assert any(float(pm.centre((0, 0, np.float32(t)), s)[2]) != float(np.float32(float(np.float32(t)) + (s - 64) * float(pm.STEP)))
               for t in (0.1, 0.7, 2.9) for s in range(33, 64))


@pytest.mark.parametrize("name", ["stride_3", "tie_half_turn", "empty_scans", "dilate_0", "min_bits_partners", "thetas"])
def test_best_pairs_against_the_definition_as_written(name):
    """place_model.best (bit planes and matrix products) against loops over (q, j, s) with word-wise popcounts"""
    case = pc.cases()[name]
    p = case.params
    d, bits, places, _ = pc.model(name)
    for pl in places:
        q = int(pl["q"])
        last = q - p["min_gap"] - 1
        dq = pm.dilated(d[q], p["dilate"])
        bq = int(pm.popcount(dq))
        bestk = None
        if bits[q] >= p["min_bits"]:
            for j in range(0, last + 1):
                if bits[j] < p["min_bits"]:
                    continue
                ov = pm.overlaps(dq, d[j])
                for s in range(64):
                    k = pm.key_of(ov[s], bq, bits[j])
                    if bestk is None or k > bestk[0]:
                        bestk = (k, j, s, int(ov[s]))
        if bestk is None:
            want = (q, -1, 0, 0, 0, int(bits[q]), 0, -1)
        else:
            k, j, s, o = bestk
            want = (q, j, s, k, o, int(bits[q]), int(bits[j]), j if k >= p["min_key"] else -1)
        assert tuple(int(v) for v in pl) == want


def test_descriptor_rules():
    r = np.array([0.15, 0.16, 0.25, 7.99, 8.0, 1.0, 1.0, 1.0, 1.0, np.nan], np.float32)
    t = np.array([0.0, 0.0, 0.0, 0.0, 0.0, -0.01, 6.29, 1024.5, np.nan, 0.0], np.float32)
    d = pm.descriptor(r, t, 4.0, 8.0)
    assert d[0] == (1 << 0) | (1 << 1) | (1 << 31) | (1 << 4)          # 0.16 -> bin 0, 0.25 -> 1, 7.99 -> 31; 6.29 rad is sector 64 & 63 = 0
    assert d[63] == 1 << 4 and int(pm.popcount(d)) == 5                  # -0.01 rad is sector -1 & 63
    assert pm.dilated(np.array([1 | 1 << 31, 1 << 5], np.uint32), 1).tolist() == [0b11 | 0b11 << 30, 0b111 << 4]
    assert pm.key_of(0, 0, 0) == 0 and pm.key_of(2048, 2048, 2048) == 65536 and pm.key_of(1, 2, 2) == 65536 // 3


def test_two_lap_error_is_the_stated_one():
    """pose mode's kept edges on loop_closure_cases' two_lap case against truth: what the drift case's bound is twice of"""
    truth = lcc.trajectories(32, 16)[0]
    errs = [pc.edge_error(c["z"], truth[c["j"]], truth[c["q"]]) for c in lcc.model("two_lap") if c["flags"] == 0]
    pos, ang = max(e[0] for e in errs), max(e[1] for e in errs)
    print("two_lap kept", len(errs), "position error", pos, "heading error", ang)
    assert len(errs) >= 3
    assert pos <= pc.TWO_LAP_POS_ERROR <= pos * 1.001 and ang <= pc.TWO_LAP_ANG_ERROR <= ang * 1.001


def test_drift_case():
    case = pc.cases()["drift"]
    p = case.params
    assert lcm.pairs(case.poses, p["stride"], p["min_gap"], pc.DRIFT_RADIUS) == []
    assert math.hypot(*pc.DRIFT_XY) > pc.DRIFT_RADIUS
    kept = [c for c in pc.model("drift")[3] if c["flags"] == 0]
    assert len(kept) >= 1
    for c in kept:
        pos, ang = pc.edge_error(c["z"], case.truth[c["j"]], case.truth[c["q"]])
        print("drift edge", c["j"], c["q"], "shift", c["shift"], "position error", pos, "heading error", ang)
        assert pos <= pc.DRIFT_POS_BOUND and ang <= pc.DRIFT_ANG_BOUND


def test_every_flag_of_the_gate_is_raised_somewhere():
    seen = set()
    for name in NAMES:
        for c in pc.model(name)[3]:
            seen.add(c["flags"])
    assert 0 in seen and lcm.TOO_MANY_RAYS in seen
    for bit in (lcm.NOT_ACCEPTED, lcm.TIED, lcm.ON_EDGE):
        assert any(f & bit for f in seen if f != lcm.TOO_MANY_RAYS), bit


def test_parameter_limits():
    ok = dict(pm.PLACE_DEFAULTS)
    assert pm.check_place(ok)
    for bad in (dict(bins_per_meter=0.0), dict(bins_per_meter=-1.0), dict(bins_per_meter=1000.5), dict(bins_per_meter=float("nan")),
                dict(place_max_range=0.15), dict(place_max_range=1001.0), dict(place_max_range=float("nan")), dict(dilate=2), dict(dilate=-1),
                dict(min_key=-1), dict(min_key=65537), dict(min_bits=-1), dict(min_bits=2049)):
        assert not pm.check_place(dict(ok, **bad)), bad
    for fine in (dict(bins_per_meter=1000.0), dict(place_max_range=1000.0), dict(min_key=65536), dict(min_bits=2048), dict(min_key=0, min_bits=0)):
        assert pm.check_place(dict(ok, **fine)), fine
