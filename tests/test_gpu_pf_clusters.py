"""bl_pf_clusters on the GPU against the integer model (tests/pf_cluster_model.py): every field of every reported cluster, the
number of clusters, the total of the units and the labels are compared for equality -- no tolerance anywhere.  The clouds are the
hand-built ones of tests/pf_cluster_cases.py, uploaded with bl_pf_set_particles, and the filter's own clouds (a uniform
initialisation, sensor updates, an adaptive set).

The launch edges run from N = 2: bl_pf_create refuses a filter of one particle (the reference's assert), so N = 1 cannot exist."""
import ctypes as C
import math

import numpy as np
import pytest

import global_init_model as gm
import helpers
import pf_cluster_cases as cases
import pf_cluster_model as pm
import botlab_amd as bl
from botlab_amd import _capi, synth

pytestmark = pytest.mark.gpu
CASES = cases.all_cases()
_MODELS = {}


def _model(name):
    if name not in _MODELS:
        c = CASES[name]
        _MODELS[name] = pm.clusters(c["x"], c["y"], c["th"], c["units"], c["bin_xy"], c["T"], c["K"])
    return _MODELS[name]


def _particles(c):
    p = np.zeros(len(c["x"]), bl.PARTICLE_DTYPE)
    p["x"], p["y"], p["theta"] = c["x"], c["y"], c["th"]
    p["p_x"], p["p_y"], p["p_theta"] = c["x"], c["y"], c["th"]
    return p


def _upload(ctx, c, pf=None):
    pf = pf or bl.ParticleFilter(len(c["x"]), ctx=ctx)
    pf.setParticles(_particles(c), c["units"])
    return pf


def _same(res, mod, K, tag):
    """Everything the call reports equals the model."""
    assert (res["num_clusters"], res["units_sum"], res["active"]) == (mod["num_clusters"], mod["units_sum"], mod["active"]), tag
    shown = min(mod["num_clusters"], K)
    assert len(res["clusters"]) == shown, tag
    for rank, (g, e) in enumerate(zip(res["clusters"], mod["clusters"])):
        for f in ("count", "units", "anchor") + pm.SUMS:
            assert g[f] == e[f], (tag, rank, f, g[f], e[f])
    tail = bytes(res["raw"])[24 + 144 * shown:]
    assert tail == bytes(len(tail)), tag                    # the clusters beyond min(C, K) are zero
    if "labels" in res:
        bad = np.flatnonzero(res["labels"] != mod["labels"])
        assert bad.size == 0, (tag, bad[:8], res["labels"][bad[:8]], mod["labels"][bad[:8]])


def _run(pf, c, labels=True):
    return pf.clusters(c["bin_xy"], c["T"], c["K"], labels=labels)


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_built_cloud_equals_model(gpu_ctx, name):
    """Launch edges (one bin / every particle alone, N = 2 .. 4097), propagation depth (snakes, rings), the heading wrap and T = 1,
    2, 3, the position and heading edge values, zero-unit bridges and clusters, sums past 2^64, K against C -- and the same call
    again gives the same bytes, with and without labels."""
    c = CASES[name]
    pf = _upload(gpu_ctx, c)
    res = _run(pf, c)
    _same(res, _model(name), c["K"], name)
    again = _run(pf, c)
    assert bytes(again["raw"]) == bytes(res["raw"]) and np.array_equal(again["labels"], res["labels"])
    assert bytes(_run(pf, c, labels=False)["raw"]) == bytes(res["raw"])
    pf.close()


def test_case_properties_on_the_device(gpu_ctx):
    """What the cases are built to show, read off the device's own result."""
    def run(name):
        pf = _upload(gpu_ctx, CASES[name])
        r = _run(pf, CASES[name])
        pf.close()
        return r
    assert run("snake")["num_clusters"] == 1 and run("two_snakes")["num_clusters"] == 2 and run("ring")["num_clusters"] == 2
    assert run("wrap_35")["num_clusters"] == 1 and run("wrap_34")["num_clusters"] == 2
    b = run("bridges")
    assert [k["units"] for k in b["clusters"]] == [45, 4, 0] and b["clusters"][0]["count"] == 8
    assert bl.ParticleFilter.cluster_pose(b, 2) is None and bl.ParticleFilter.cluster_pose(b, 0)["share"] == 45 / 49
    k1, k64, c100 = run("K1"), run("K64"), run("C100")
    assert k1["num_clusters"] == 3 and len(k1["clusters"]) == 1 and sorted(set(k1["labels"])) == [-1, 0]
    assert k64["num_clusters"] == 3 and len(k64["clusters"]) == 3
    assert c100["num_clusters"] == 100 and (c100["labels"] == -1).sum() == 92 and sorted(set(c100["labels"])) == list(range(-1, 8))
    big = run("big_units")
    assert big["clusters"][0]["sxx"] > 2 ** 90


def test_reuse_two_clouds_on_one_filter(gpu_ctx):
    """A second call on a different cloud does not see the first call's table (1025 particles in one bin, then 1025 bins, then the
    first again)."""
    a, b = CASES["one_bin_1025"], CASES["isolated_1025"]
    pf = _upload(gpu_ctx, a)
    first = _run(pf, a)
    _same(first, _model("one_bin_1025"), a["K"], "a")
    _upload(gpu_ctx, b, pf)
    _same(_run(pf, b), _model("isolated_1025"), b["K"], "b")
    _upload(gpu_ctx, a, pf)
    back = _run(pf, a)
    assert bytes(back["raw"]) == bytes(first["raw"]) and np.array_equal(back["labels"], first["labels"])
    pf.close()


def _units_of(pf, parts):
    """The record's weight units from the exported weights u / S (u < 2^32 and S < 2^53: the product rounds back to u)."""
    S = pf.spread()["units_sum"]
    u = np.rint(parts["weight"] * float(S))
    assert int(u.sum()) == S
    return u.astype(np.uint64)


def _same_as_model_of_the_filter(pf, bin_xy, T, K, tag):
    parts = pf.particles()
    mod = pm.clusters(parts["x"], parts["y"], parts["theta"], _units_of(pf, parts), bin_xy, T, K)
    res = pf.clusters(bin_xy, T, K, labels=True)
    _same(res, mod, K, tag)
    return res


def _calibrated(maps, steps):
    m = maps[gm.CAL_MAP]
    truth = np.where(m["cells"] > 0, 127, -127).astype(np.int8)
    poses = synth.square_trajectory(gm.CAL_START, steps, step_len=0.04, turn=0.1, side=0.3)     # (test_gpu_recovery.py's scenario)
    odo = synth.odometry_from_truth(poses, np.random.default_rng(8))
    scans = [synth.raycast_scan(truth, m["origin"], 0.05, poses[max(k - 1, 0)], poses[k], 1000 + 100000 * k) for k in range(len(poses))]
    return m, odo, scans


def test_clouds_of_the_filter_itself(maps, gpu_ctx):
    """After initializeFilterUniformly on the 200 x 200 map, after three sensor updates from there, and on an adaptive set whose
    record holds fewer particles than the capacity: the call reads the `active` particles of the current record."""
    m, odo, scans = _calibrated(maps, 4)
    assert m["cells"].shape == (200, 200)
    g = bl.OccupancyGrid.from_cells(m["cells"], m["origin"], m["mpc"], cellsPerMeter=helpers.CPM_DEFAULT, ctx=gpu_ctx)
    n = 20_000
    pf = bl.ParticleFilter(n, ctx=gpu_ctx)
    pf.setNoiseSeed(17)
    pf.initializeFilterUniformly(g, utime=0, seed=gm.CAL_SEED)
    r = _same_as_model_of_the_filter(pf, 0.25, 36, 8, "uniform")
    assert r["active"] == n
    for k in range(4):                                       # the first one latches the odometry; three moved sensor updates
        pf.updateFilter(bl.make_pose(*odo[k], utime=scans[k].utime), scans[k], g, rand_value=1000 + k)
    _same_as_model_of_the_filter(pf, 0.25, 36, 8, "updated")
    pf.close()
    # adaptive: started at the pose, the count falls below the capacity
    pf = bl.ParticleFilter(n, ctx=gpu_ctx)
    pf.setNoiseSeed(17)
    pf.initializeFilterAtPose(bl.make_pose(*gm.CAL_START, utime=0), seed=5)
    pf.setAdaptive()
    for k in range(4):
        pf.updateFilter(bl.make_pose(*odo[k], utime=scans[k].utime), scans[k], g, rand_value=1000 + k)
    active = pf.adaptiveState()["active"]
    assert active < n
    r = _same_as_model_of_the_filter(pf, 0.25, 36, 8, "adaptive")
    assert r["active"] == active and len(r["labels"]) == active and sum(c["count"] for c in r["clusters"]) <= active
    pf.close()
    g.close()


def _call(ctx, pf, bin_xy, T, K, out, labels=None):
    p = _capi.PfClusterParams(bin_xy, T, K)
    return ctx.lib.bl_pf_clusters(pf.h, C.byref(p), C.byref(out), labels.ctypes.data if labels is not None else None)


def test_errors_leave_filter_and_out(maps, gpu_ctx):
    """Bad parameters: BL_ERR_ARG; before an initialisation, with an update pending and on a composed shard: BL_ERR_STATE.  out, the
    labels and the filter are as they were."""
    m, odo, scans = _calibrated(maps, 3)
    g = bl.OccupancyGrid.from_cells(m["cells"], m["origin"], m["mpc"], cellsPerMeter=helpers.CPM_DEFAULT, ctx=gpu_ctx)
    n = 2048
    out = _capi.PfClusters()
    C.memset(C.byref(out), 0xAB, C.sizeof(out))
    marked = bytes(out)
    labels = np.full(n, 77, np.int32)
    fresh = bl.ParticleFilter(n, ctx=gpu_ctx)
    assert _call(gpu_ctx, fresh, 0.25, 36, 8, out, labels) == _capi.BL_ERR_STATE            # before an initialisation
    pf = bl.ParticleFilter(n, ctx=gpu_ctx)
    pf.setNoiseSeed(3)
    pf.initializeFilterAtPose(bl.make_pose(*gm.CAL_START, utime=0), seed=5)
    pf.updateFilter(bl.make_pose(*odo[0], utime=scans[0].utime), scans[0], g, rand_value=1000)
    parts = pf.particles().tobytes()
    good = pf.clusters(0.25, 36, 8, labels=True)
    for bin_xy, T, K in [(0.0, 36, 8), (-1.0, 36, 8), (math.nan, 36, 8), (math.inf, 36, 8), (0.25, 0, 8), (0.25, -3, 8), (0.25, 4097, 8),
                         (0.25, 36, 0), (0.25, 36, 65), (0.25, 36, -1)]:
        assert _call(gpu_ctx, pf, bin_xy, T, K, out, labels) == _capi.BL_ERR_ARG, (bin_xy, T, K)
    assert gpu_ctx.lib.bl_pf_clusters(pf.h, None, C.byref(out), None) == _capi.BL_ERR_ARG
    assert _call(gpu_ctx, pf, 0.25, 4096, 64, out, labels) == _capi.BL_OK                       # the limits themselves are legal
    C.memset(C.byref(out), 0xAB, C.sizeof(out))
    labels[:] = 77
    pf.updateBegin(bl.make_pose(*odo[1], utime=scans[1].utime), scans[1], g, 1001)
    assert _call(gpu_ctx, pf, 0.25, 36, 8, out, labels) == _capi.BL_ERR_STATE                   # an update pending
    pf.updateEnd()
    # a composed shard: two ranks of one set on this device, each with the other's records mapped
    ranks = [bl.ParticleFilter(n, ctx=gpu_ctx, shard=(r * 1024, (r + 1) * 1024)) for r in range(2)]
    ptrs = []
    for r, k in enumerate(ranks):
        k.initializeFilterAtPose(bl.make_pose(*gm.CAL_START, utime=0), seed=5)
        _capi.check(gpu_ctx.lib.bl_pf_shard_setup(k.h, r, 2, 1024))
        p3 = [C.c_void_p() for _ in range(3)]
        _capi.check(gpu_ctx.lib.bl_pf_shard_local_ptrs(k.h, *[C.byref(q) for q in p3]))
        ptrs.append([q.value for q in p3])
    for k in ranks:
        for r in range(2):
            _capi.check(gpu_ctx.lib.bl_pf_shard_set_peer(k.h, r, *ptrs[r]))
        _capi.check(gpu_ctx.lib.bl_pf_shard_commit(k.h))
        assert _call(gpu_ctx, k, 0.25, 36, 8, out, labels) == _capi.BL_ERR_STATE
    assert bytes(out) == marked and np.all(labels == 77)
    # the filter the refused calls were made on: the same particles before the update, the same clusters as a filter never refused
    twin = bl.ParticleFilter(n, ctx=gpu_ctx)
    twin.setNoiseSeed(3)
    twin.initializeFilterAtPose(bl.make_pose(*gm.CAL_START, utime=0), seed=5)
    twin.updateFilter(bl.make_pose(*odo[0], utime=scans[0].utime), scans[0], g, rand_value=1000)
    assert twin.particles().tobytes() == parts
    assert bytes(twin.clusters(0.25, 36, 8, labels=True)["raw"]) == bytes(good["raw"])
    twin.updateBegin(bl.make_pose(*odo[1], utime=scans[1].utime), scans[1], g, 1001)
    twin.updateEnd()
    assert twin.particles().tobytes() == pf.particles().tobytes()
    a, b = twin.clusters(0.25, 36, 8, labels=True), pf.clusters(0.25, 36, 8, labels=True)
    assert bytes(a["raw"]) == bytes(b["raw"]) and np.array_equal(a["labels"], b["labels"])
    for h in ranks + [fresh, pf, twin, g]:
        h.close()


def test_bimodal_cloud_has_a_leading_hypothesis(gpu_ctx):
    """70 % of the units around A, 30 % around B four metres away: the whole cloud's spread is far above the driver's 0.2 m, its mean
    lies between the modes; the heaviest cluster holds exactly 0.7 and sits on A."""
    c = CASES["bimodal"]
    pf = _upload(gpu_ctx, c)
    s = pf.spread()
    assert s["position_std"] > 0.2 and 1.5 < s["mean_x"] < 4.5
    res = _run(pf, c)
    mod = _model("bimodal")
    _same(res, mod, c["K"], "bimodal")
    a = res["clusters"][0]
    assert (a["units"], res["units_sum"]) == (7000, 10000)
    pose = bl.ParticleFilter.cluster_pose(res, 0)
    assert pose["share"] == 0.7
    # A's weighted mean by the model, in fine units of bin_xy / 1024
    members = np.flatnonzero(mod["labels"] == 0)
    px, py, _, _, _ = pm.particle_terms(c["x"], c["y"], c["th"], c["bin_xy"], c["T"])
    u = c["units"][members].astype(object)
    fine = c["bin_xy"] / 1024.0
    mx = float(sum(u * px[members].astype(object))) / float(sum(u))
    my = float(sum(u * py[members].astype(object))) / float(sum(u))
    assert abs(pose["mean_x"] / fine - (mx + 0.5)) <= 1.0 and abs(pose["mean_y"] / fine - (my + 0.5)) <= 1.0
    want = pm.cluster_pose(mod["clusters"][0], mod["units_sum"], c["bin_xy"])
    assert {k: pose[k] for k in want} == want
    assert pose["position_std"] < 0.2 and pose["theta_std"] < 0.3 and abs(pose["theta"] - 0.5) < 0.02
    pf.close()
