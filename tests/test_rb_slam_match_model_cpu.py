"""The model of the scan-matched Rao-Blackwellized SLAM (tests/rb_slam_match_model.py) and the inputs of its GPU tests, on the CPU.

CASES are the inputs tests/test_gpu_rb_slam_match.py runs on the device; record(name) runs the model over one of them ONCE per session
and keeps what the device is compared with after every update.  The tests here show that every input reaches the condition it is there
for (the counts are printed and asserted non-zero), that a 0, 0, 0 window is the run of RBSlamModel, that an all-zero map moves nobody,
and the one behavioural claim: with slipping wheels the match keeps the SLAM pose where dead reckoning loses it."""
import math

import numpy as np
import pytest

import rb_slam_match_model as rmm
import rb_slam_model as rbm
import scan_match_model as smm
from botlab_amd import synth
from test_rb_slam_model_cpu import CPM, HIT, MAX_LASER, MISS, RAGGED_ORIGIN, RAGGED_SHAPE, make_run

DTH = math.radians(0.5)
HEADING_PI = math.pi - 0.004            # "heading_pi": the run's first heading, less than one step of DTH below pi
CROP = 64
BIG = 10 ** 9


def _scans(maps, steps, rays=synth.RAYS, pause_at=None):
    m, poses, odoms, scans = make_run(maps, steps, pause_at=pause_at)
    if rays != synth.RAYS:
        truth = np.where(m["cells"] > 0, 127, -127).astype(np.int8)
        scans = [synth.raycast_scan(truth, m["origin"], 0.05, poses[max(k - 1, 0)], poses[k], odoms[k][3], rays=rays) for k in range(len(poses))]
    return m, odoms, scans


def _cell_of(m, xy):
    return int((xy[0] - float(m["origin"][0])) / 0.05), int((xy[1] - float(m["origin"][1])) / 0.05)


def _crop(m, x0, y0, w, h):
    """cells[y0 : y0 + h, x0 : x0 + w] with zeros outside the map, and the origin of that block."""
    H, W = m["cells"].shape
    out = np.zeros((h, w), np.int8)
    ys, xs = np.arange(y0, y0 + h), np.arange(x0, x0 + w)
    oky, okx = (ys >= 0) & (ys < H), (xs >= 0) & (xs < W)
    out[np.ix_(oky, okx)] = m["cells"][np.ix_(ys[oky], xs[okx])]
    return out


def _origin_at(m, x0, y0):
    return (np.float32(float(m["origin"][0]) + 0.05 * x0), np.float32(float(m["origin"][1]) + 0.05 * y0))


def _case(maps, name):
    """dict(P, shape, origin, mpc, cpm, num, den, spread, odoms, scans, init_maps (P x H x W or None), match: per update the
    setScanMatching keywords or None, seed)."""
    c = dict(num=1, den=1, mpc=None, cpm=CPM, seed=17, spread=5)
    on = lambda **kw: dict(dict(nx=2, ny=2, ntheta=3, dtheta=DTH, max_range=8.0, min_score=0), **kw)
    if name in ("main", "min_score", "p1", "p1000", "pause", "heading_pi"):
        P = {"main": 16, "min_score": 4, "p1": 1, "p1000": 1000, "pause": 4, "heading_pi": 16}[name]
        steps = {"main": 6, "min_score": 3, "p1": 4, "p1000": 2, "pause": 5, "heading_pi": 3}[name]
        m, odoms, scans = _scans(maps, steps, rays=64 if name == "p1000" else synth.RAYS, pause_at=3 if name == "pause" else None)
        if name == "heading_pi":
            # the odometry's heading turned to just below pi (the maps then fit no scan: only the arithmetic is under test), so that a
            # particle moved by dk > 0 crosses pi and its heading is wrapped
            odoms = [(o[0], o[1], o[2] + HEADING_PI, o[3]) for o in odoms]
        cx, cy = _cell_of(m, odoms[0])
        x0, y0 = cx - CROP // 2, cy - CROP // 2
        rng = np.random.default_rng(3)
        sh = rng.integers(-2, 3, (P, 2))
        init = np.stack([_crop(m, x0 + int(sh[p, 0]), y0 + int(sh[p, 1]), CROP, CROP) for p in range(P)])
        kw = on(max_range=2.0) if name == "main" else on(min_score=BIG) if name == "min_score" else on(nx=1, ny=1, ntheta=1) if name == "p1000" else on()
        c.update(P=P, shape=(CROP, CROP), origin=_origin_at(m, x0, y0), init_maps=init, match=[kw] * len(odoms))
    elif name in ("zero_window", "off_on_off", "uniform", "uniform_81", "all_zero", "rays720", "no_valid_rays", "all_beyond"):
        steps = {"zero_window": 4, "off_on_off": 6, "uniform": 1, "uniform_81": 1, "all_zero": 2, "rays720": 2, "no_valid_rays": 2,
                 "all_beyond": 2}[name]
        m, odoms, scans = _scans(maps, steps, rays=720 if name == "rays720" else synth.RAYS)
        P = 4
        init = np.stack([m["cells"]] * P)
        kw = on()
        if name == "zero_window":
            kw = on(nx=0, ny=0, ntheta=0)
        if name == "uniform":
            init = np.full_like(init, 5)
            kw = on(ntheta=2)
        if name == "uniform_81":
            # 81 candidates a heading: the ties are counted in two waves of the kernel's workgroup; and a ray at the lower limit itself,
            # which does not count (on this map every ray that counts adds 5 to every score)
            init = np.full_like(init, 5)
            kw = on(nx=4, ny=4, ntheta=1)
            for s in scans:
                s.ranges[0] = smm.MIN_RANGE
        if name == "all_zero":
            init = None
        if name == "no_valid_rays":
            for s in scans:
                s.ranges[:] = np.float32(0.1)
        if name == "all_beyond":
            kw = on(max_range=0.2)
        match = [kw] * len(odoms)
        if name == "off_on_off":
            match = [None, None, None, kw, kw, None, None]
        c.update(P=P, shape=m["cells"].shape, origin=m["origin"], init_maps=init, match=match)
    elif name == "ragged":
        m, odoms, scans = _scans(maps, 3)
        P = 8
        x0, y0 = _cell_of(m, RAGGED_ORIGIN)
        block = _crop(m, x0, y0, RAGGED_SHAPE[1], RAGGED_SHAPE[0])
        c.update(P=P, shape=RAGGED_SHAPE, origin=RAGGED_ORIGIN, init_maps=np.stack([block] * P), match=[on(ntheta=2)] * len(odoms))
    elif name == "direct":
        # 400 x 400 cells of 1.25 cm around the start: rays of 2.4 m and more reach 192 cells, the bound of the window is the whole grid
        # (160000 bytes) and cannot be staged.  The maps are noise: only the arithmetic is under test.
        m, odoms, scans = _scans(maps, 2)
        P = 4
        rng = np.random.default_rng(8)
        init = rng.integers(-128, 128, (P, 400, 400)).astype(np.int8)
        origin = (np.float32(odoms[0][0] - 2.5), np.float32(odoms[0][1] - 2.5))
        c.update(P=P, shape=(400, 400), origin=origin, mpc=np.float32(0.0125), cpm=np.float32(80.0), init_maps=init,
                 match=[on(nx=1, ny=1, ntheta=1)] * len(odoms))
    else:
        raise KeyError(name)
    if c["mpc"] is None:
        c["mpc"] = m["mpc"]
    c.update(odoms=odoms, scans=scans, name=name)
    return c


CASES = ["main", "zero_window", "off_on_off", "direct", "ragged", "uniform", "min_score", "rays720", "no_valid_rays", "all_beyond", "pause",
         "p1", "p1000", "uniform_81", "heading_pi"]
_records = {}


def new_model(oracle, c, plain=False):
    mk = rbm.started_model if plain else rmm.started_model
    mdl = mk(oracle, c["P"], c["shape"], c["mpc"], c["cpm"], c["origin"], MAX_LASER, HIT, MISS, c["num"], c["den"], c["odoms"][0], c["spread"])
    if c["init_maps"] is not None:
        mdl.maps[:] = c["init_maps"]
    return mdl


def record(oracle, maps, name, plain=False):
    """(case, per-update snapshots of the model); computed once per session and never changed.  plain: rb_slam_model.RBSlamModel,
    matching ignored."""
    key = (name, plain)
    if key in _records:
        return _records[key]
    c = _case(maps, name)
    mdl = new_model(oracle, c, plain)
    rng = np.random.default_rng(c["seed"])
    snaps, current = [], "unset"
    for k, o in enumerate(c["odoms"]):
        kw = None if plain else c["match"][k]
        if not plain and kw is not current:
            assert mdl.set_scan_matching(**kw) if kw is not None else mdl.set_scan_matching(None)
            current = kw
        noise = mdl.draw_noise(o, rng)
        before = mdl.parts.copy()
        r = mdl.update(o, c["scans"][k], 900 + k, noise)
        matched = r["moved"] and kw is not None
        snaps.append(dict(r=r, noise=noise, rand_value=900 + k, parts=mdl.parts.copy(), cum=mdl.cum.copy(), units=mdl.units.copy(), idx=mdl.idx.copy(),
                          like=mdl.like.copy(), maps=mdl.maps.copy(), matched=matched, before=before,
                          match={f: v.copy() for f, v in mdl.match.items()} if matched else None))
    _records[key] = (c, snaps)
    return _records[key]


def conditions(c, snaps):
    """The six counts of the issue's table over the matched updates of a run."""
    n = dict(moved_off_centre=0, distinct=0, ties=0, rejected=0, clipped=0, skipped_rays=0)
    seen = set()
    H, W = c["shape"]
    for k, s in enumerate(snaps):
        if not s["matched"]:
            continue
        kw, mt = c["match"][k], s["match"]
        off = (mt["di"] != 0) | (mt["dj"] != 0) | (mt["dk"] != 0)
        n["moved_off_centre"] += int(np.count_nonzero(off))
        seen |= set(zip(mt["di"].tolist(), mt["dj"].tolist(), mt["dk"].tolist()))
        n["ties"] += int(np.count_nonzero(mt["ties"] > 1))
        n["rejected"] += int(np.count_nonzero(mt["accepted"] == 0))
        sc = c["scans"][k]
        n["skipped_rays"] += int(np.count_nonzero((sc.ranges > smm.MIN_RANGE) & ~(sc.ranges < np.float32(kw["max_range"]))))
        reach = rmm.reach_cells(sc, kw["max_range"], c["cpm"])
        for p in range(c["P"]):
            # the centre of the match: the pose the action left = the matched pose moved back by the accepted shift; the window's
            # clipping does not depend on a shift of two cells where it is counted (a window of > 100 cells on grids it overhangs)
            raw, clip = rmm.window_of((s["parts"]["x"][p], s["parts"]["y"][p]), c["origin"], c["cpm"], reach, kw["nx"], kw["ny"], W, H)
            n["clipped"] += int(raw != clip)
    n["distinct"] = len(seen)
    return n


@pytest.mark.parametrize("name", CASES)
def test_inputs_reach_their_conditions(oracle, maps, name):
    c, snaps = record(oracle, maps, name)
    n = conditions(c, snaps)
    print(name, n, "path", [rmm.window_path(c["scans"][k], c["match"][k]["max_range"], c["cpm"], c["shape"][1], c["shape"][0], c["match"][k]["nx"],
                                           c["match"][k]["ny"]) for k, s in enumerate(snaps) if s["matched"]])
    assert any(s["matched"] for s in snaps)
    want = {"main": ["moved_off_centre", "distinct", "clipped", "skipped_rays"], "uniform": ["ties"], "min_score": ["rejected"],
            "ragged": ["clipped", "moved_off_centre"], "all_beyond": ["skipped_rays"], "direct": ["moved_off_centre"], "p1000": ["distinct"],
            "rays720": ["moved_off_centre"]}.get(name, [])
    for f in want:
        assert n[f] > 0, (name, f, n)
    if name == "main":
        assert n["distinct"] > 3
        assert any(s["r"]["resampled"] and s["matched"] and not np.array_equal(s["idx"], np.arange(c["P"])) for s in snaps)
    if name == "uniform":                               # every candidate ties and the centre wins
        mt = snaps[1]["match"]
        assert np.all(mt["ties"] == 5 * 5 * 5) and not mt["di"].any() and not mt["dj"].any() and not mt["dk"].any() and np.all(mt["score"] > 0)
    if name == "uniform_81":                            # 243 ties, 64 of a heading's 81 candidates in the workgroup's first wave
        mt, sc = snaps[1]["match"], c["scans"][1]
        counted = int(np.count_nonzero((sc.ranges > smm.MIN_RANGE) & (sc.ranges < np.float32(8.0))))
        assert sc.ranges[0] == smm.MIN_RANGE and counted == int(np.count_nonzero(sc.ranges < np.float32(8.0))) - 1
        assert np.all(mt["ties"] == 9 * 9 * 3) and np.all(mt["score"] == 5 * counted) and not (mt["di"] | mt["dj"] | mt["dk"]).any()
    if name == "heading_pi":                            # a particle turned by dk > 0 whose heading came out below zero: wrapped
        wrapped = sum(int(np.count_nonzero((s["match"]["dk"] > 0) & (s["match"]["accepted"] != 0) & (s["parts"]["theta"] < -3.0)))
                      for s in snaps if s["matched"])
        print("heading_pi: wrapped", wrapped)
        assert wrapped > 0
    if name == "min_score":
        assert all(not s["match"]["accepted"].any() for s in snaps if s["matched"])
    if name in ("no_valid_rays", "all_beyond"):
        assert all(not s["match"]["score"].any() for s in snaps if s["matched"])
    if name == "direct":
        assert all(rmm.window_path(c["scans"][k], 8.0, c["cpm"], 400, 400, 1, 1) == 1 for k in range(1, len(snaps)))
    if name == "pause":
        assert [s["r"]["moved"] for s in snaps].count(False) == 2 and not snaps[3]["r"]["moved"]
    if name == "off_on_off":
        assert [s["matched"] for s in snaps] == [False, False, False, True, True, False, False]


def _same_run(a, b):
    for x, y in zip(a, b):
        assert x["r"] == y["r"]
        assert x["parts"].tobytes() == y["parts"].tobytes() and x["maps"].tobytes() == y["maps"].tobytes()
        assert np.array_equal(x["cum"], y["cum"]) and np.array_equal(x["idx"], y["idx"]) and np.array_equal(x["like"], y["like"])


def test_zero_window_is_the_run_without_matching(oracle, maps):
    _same_run(record(oracle, maps, "zero_window")[1], record(oracle, maps, "zero_window", plain=True)[1])


def test_min_score_above_every_score_is_the_run_without_matching(oracle, maps):
    _same_run(record(oracle, maps, "min_score")[1], record(oracle, maps, "min_score", plain=True)[1])


def test_all_zero_map_moves_nobody(oracle, maps):
    c = _case(maps, "all_zero")
    mdl = new_model(oracle, c)
    mdl.set_scan_matching(2, 2, 3, DTH, 8.0, 0)
    rng = np.random.default_rng(1)
    mdl.update(c["odoms"][0], c["scans"][0], 1, mdl.draw_noise(c["odoms"][0], rng))        # latches: the maps stay empty
    plain = new_model(oracle, c, plain=True)
    rng2 = np.random.default_rng(1)
    plain.update(c["odoms"][0], c["scans"][0], 1, plain.draw_noise(c["odoms"][0], rng2))
    noise = mdl.draw_noise(c["odoms"][1], rng)
    assert not mdl.maps.any()
    mdl.update(c["odoms"][1], c["scans"][1], 2, noise)
    plain.update(c["odoms"][1], c["scans"][1], 2, plain.draw_noise(c["odoms"][1], rng2))
    assert not mdl.match["score"].any() and not mdl.match["di"].any() and not mdl.match["dj"].any() and not mdl.match["dk"].any()
    assert np.all(mdl.match["ties"] == 5 * 5 * 7)
    assert mdl.parts.tobytes() == plain.parts.tobytes() and mdl.maps.tobytes() == plain.maps.tobytes()


def test_refusals(oracle, maps):
    c = _case(maps, "p1")
    mdl = new_model(oracle, c)
    assert mdl.set_scan_matching(1, 1, 1, DTH, 8.0, 0)
    for bad in [dict(nx=9), dict(ny=9), dict(ntheta=17), dict(nx=-1), dict(dtheta=0.0), dict(dtheta=float("nan")), dict(dtheta=-1.0)]:
        assert not mdl.set_scan_matching(**dict(dict(nx=1, ny=1, ntheta=1, dtheta=DTH), **bad))
    assert mdl.matching["nx"] == 1                       # the previous setting stays


# ---- does it do anything?  Every particle holds the finished map, the wheels slip (the odometry reports half of each true
# translation), no noise, schedule 1 / 1, window 2, 2, 4 x 0.5 degrees.  BOUND is the one tests/test_scan_match_driver_cpu.py uses for
# its frozen-odometry run, set by the issue before anything was measured.
SLIP_P, SLIP_STEPS, BOUND = 8, 30, 0.10


def _slip_error(oracle, maps, slip, matching):
    m, poses, odoms, scans = make_run(maps, SLIP_STEPS)
    if slip:
        odo = [np.array(poses[0], dtype=np.float64)]
        for a, b in zip(poses[:-1], poses[1:]):
            odo.append(np.array([odo[-1][0] + 0.5 * (b[0] - a[0]), odo[-1][1] + 0.5 * (b[1] - a[1]), b[2]]))
        odoms = [(odo[k][0], odo[k][1], odo[k][2], odoms[k][3]) for k in range(len(odoms))]
    mdl = rmm.started_model(oracle, SLIP_P, m["cells"].shape, m["mpc"], CPM, m["origin"], MAX_LASER, HIT, MISS, 1, 1, odoms[0])
    mdl.maps[:] = m["cells"]
    if matching:
        mdl.set_scan_matching(2, 2, 4, DTH, 8.0, 0)
    rng = np.random.default_rng(0)
    r = None
    for k in range(len(odoms)):
        r = mdl.update(odoms[k], scans[k], 31 + k, mdl.draw_noise(odoms[k], rng, stds=(0.0, 0.0, 0.0)))
    return float(np.hypot(r["pose"][0] - poses[-1][0], r["pose"][1] - poses[-1][1]))


def test_matching_recovers_what_slipping_wheels_lose(oracle, maps):
    """Final position error of the SLAM pose after 30 steps (0.8 m of a 1.2 m path travelled straight, then a turn).
    Measured: see DESIGN.md section 4.16."""
    e_ref = _slip_error(oracle, maps, slip=False, matching=False)
    e_on = _slip_error(oracle, maps, slip=True, matching=True)
    e_off = _slip_error(oracle, maps, slip=True, matching=False)
    print("true odometry, matching off: %.3f m; slipping, matching on: %.3f m; slipping, matching off: %.3f m" % (e_ref, e_on, e_off))
    assert e_off > e_ref + BOUND, "the input proves nothing: dead reckoning survives the slip"
    assert e_on <= e_ref + BOUND
