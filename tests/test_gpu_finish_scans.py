"""The end of a sensor update (bl_mcl_finish.h) at the sizes and on the clouds where its wave-wide sums and scans can go wrong.

A cloud is uploaded, one sensor update runs against a shipped 200 x 200 map, and OraclePF consumes the same noise:
  * the pose estimate is the oracle's, bit for bit (x, y: the serially rounded float sums; theta: atan2 of the ordered double sums);
  * the weights are the oracle's (1e-5 relative, the bound of tests/test_gpu_parity.py);
  * the NEXT update draws the oracle's source indices -- they come from the weight prefix this update's groups wrote.
Every case runs once with the finish riding in the map update's launch (updateBegin + updateMapFinishingFilter) and once on its own
(updateFilter); the oracle's side is computed once per case.

Sizes: lanes and waves partly empty (2, 63..65; a filter of one particle cannot be made: the constructor refuses it as
particle_filter.cpp:11 does), the sub-tile edge (127..129), the group edge (511..513), the end of the
pre-chain's nine sub-tiles (1151..1153), a mid-sized set that is no multiple of a wave, the smallest set with a second region in
k_mcl_main's launch on the device at hand, and the 1024-thread groups (163 841).
Clouds: `offset` around (3.3, -2.1): both sums only ever cross binades upwards; `origin`: the sums hover around zero (wild maps,
trees); `axis`: every y exactly 0; `dominant`: one particle holds nearly all the weight; `floor`: every particle at the likelihood
floor."""
import numpy as np
import pytest

import botlab_amd as bl
import helpers
import oracle_lib
from botlab_amd import synth
from botlab_amd.host import PARTICLE_DTYPE, LidarScan

pytestmark = pytest.mark.gpu

MAP = "obstacle_slam_10mx10m_5cm"
SECOND_REGION = "second_region"
SIZES = [2, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1151, 1152, 1153, 4099, SECOND_REGION, 163_841]
CLOUDS = ("offset", "origin", "axis", "dominant", "floor")
CASES = [(n, c) for c in CLOUDS[:2] for n in SIZES] + [(n, c) for c in CLOUDS[2:] for n in (129, 1153, 4099)]
STEP = 0.04                                     # metres driven per update, along +x
RANDS = (1804289383, 846930886)                 # glibc rand(), unseeded


def _second_region_size():
    """k_mcl_main's launch takes a second region when the particles exceed whole rounds of the device by a little (pf_launch_main:
    128 particles per workgroup at this size, three workgroups per CU, a round counted 1/128 short): one round and nine particles
    -- two workgroups of the second region -- is 97 536 + 9 on 256 CUs."""
    import torch
    per_round = 3 * torch.cuda.get_device_properties(0).multi_processor_count
    return (per_round - per_round // 128) * 128 + 9


def _centre(cloud):
    return {"origin": (0.0, 0.0), "axis": (2.0, 0.0)}.get(cloud, (3.3, -2.1))


def build_case(maps, N, cloud):
    """(particles to upload, odometry poses 0..2, scans 0..2, zero_noise)."""
    m = maps[MAP]
    truth = np.where(m["cells"] > 0, 127, -127).astype(np.int8)
    cx, cy = _centre(cloud)
    poses = [(cx - STEP + k * STEP, cy, 0.0) for k in range(3)]         # the cloud lies around `centre` after the first moved update
    scans = [synth.raycast_scan(truth, m["origin"], 0.05, poses[max(k - 1, 0)], poses[k], 1_000_000 + 100_000 * k) for k in range(3)]
    if cloud == "floor":
        # every ray ends 0.3 m away, in cells the map knows nothing about: no hit, every particle gets the floor
        scans = [LidarScan(np.full(s.ranges.size, 0.3, np.float32), s.thetas, s.times, utime=s.utime) for s in scans]
    rng = np.random.default_rng(1000 * CLOUDS.index(cloud) + 7)
    p = np.zeros(N, PARTICLE_DTYPE)
    p["x"] = (poses[0][0] + 0.02 * rng.standard_normal(N)).astype(np.float32)
    p["y"] = (poses[0][1] + 0.02 * rng.standard_normal(N)).astype(np.float32)
    p["theta"] = (0.02 * rng.standard_normal(N)).astype(np.float32)
    if cloud == "axis":
        p["y"] = 0.0
        p["theta"] = 0.0                                                # with no noise and a drive along +x, y stays 0
    if cloud == "dominant":
        # one particle where the scan was taken, every other one a metre and a half off and turned away
        p["x"] += np.float32(1.5)
        p["theta"] += np.float32(2.0)
        p["x"][N // 2], p["y"][N // 2], p["theta"][N // 2] = poses[0]
    p["p_x"], p["p_y"], p["p_theta"] = p["x"], p["y"], p["theta"]
    p["utime"] = p["p_utime"] = int(scans[0].utime)
    p["weight"] = 1.0 / N
    return p, poses, scans, cloud == "axis"


def oracle_side(oracle, maps, N, cloud):
    """What OraclePF makes of the case: per moved update its result dict, and the particles after the first."""
    m = maps[MAP]
    p, poses, scans, zero_noise = build_case(maps, N, cloud)
    opf = oracle_lib.OraclePF(oracle, N)
    opf.set_particles(p)
    args = (m["cells"], m["mpc"], helpers.CPM_DEFAULT, m["origin"])
    latch = opf.update(oracle.pose(*poses[0], utime=scans[0].utime), scans[0], *args, 777)
    assert not latch["moved"]
    opf.set_particles(p)
    zeros = np.zeros(3 * N, np.float32) if zero_noise else None
    res, after = [], None
    for k in (1, 2):
        r = opf.update(oracle.pose(*poses[k], utime=scans[k].utime), scans[k], *args, RANDS[k - 1], noise_in=zeros)
        assert r["moved"]
        res.append(r)
        if k == 1:
            after = opf.particles()
    return p, poses, scans, res, after


def check_intent(cloud, N, res, after):
    """The clouds are what their names say (on the oracle's numbers)."""
    w = after["weight"].astype(np.float64)
    if cloud == "offset":
        assert after["x"].min() > 3.0 and after["y"].max() < -1.8
    if cloud == "origin" and N >= 63:
        assert (after["x"] > 0).any() and (after["x"] < 0).any() and (after["y"] > 0).any() and (after["y"] < 0).any()
    if cloud == "axis":
        assert np.all(after["y"] == 0.0)
    if cloud == "dominant":
        assert w.max() > 0.9 and int(w.argmax()) == N // 2
    if cloud == "floor":
        assert np.all(res[0]["raw"] == 0.0) and np.all(w == w[0])


def _bits(pose):
    return [int(v) for v in np.array([pose.x, pose.y, pose.theta], np.float32).view(np.uint32)]


@pytest.mark.parametrize("N,cloud", CASES, ids=[f"{n}-{c}" for n, c in CASES])
def test_finish_matches_the_oracle_riding_and_alone(oracle, maps, gpu_ctx, N, cloud):
    if N == SECOND_REGION:
        N = _second_region_size()
    m = maps[MAP]
    p, poses, scans, res, after = oracle_side(oracle, maps, N, cloud)
    check_intent(cloud, N, res, after)
    for riding in (True, False):
        g = bl.OccupancyGrid.from_cells(m["cells"], m["origin"], m["mpc"], cellsPerMeter=helpers.CPM_DEFAULT, ctx=gpu_ctx)
        gm = bl.OccupancyGrid.from_cells(m["cells"], m["origin"], m["mpc"], cellsPerMeter=helpers.CPM_DEFAULT, ctx=gpu_ctx)
        pf = bl.ParticleFilter(N, ctx=gpu_ctx)
        mapper = bl.Mapping(5.0, 4, 1, ctx=gpu_ctx)
        try:
            pf.setParticles(p)
            pf.debugEnable(True)
            pf.updateFilter(bl.make_pose(*poses[0], utime=scans[0].utime), scans[0], g, rand_value=777, want_pose=False)      # latches the odometry
            pf.setParticles(p)
            for k in (1, 2):
                r = res[k - 1]
                odo = bl.make_pose(*poses[k], utime=scans[k].utime)
                if riding:
                    # (the map update writes a grid of its own: the filter's map stays the one the oracle reads)
                    assert pf.updateBegin(odo, scans[k], g, RANDS[k - 1], noise=r["noise"])
                    mapper.updateMapFinishingFilter(scans[k], pf, scans[k].utime, gm)
                    pose = pf.poseEstimate()
                else:
                    pose = pf.updateFilter(odo, scans[k], g, rand_value=RANDS[k - 1], noise=r["noise"])
                where = (N, cloud, "riding" if riding else "alone", k)
                idx, like = pf.debugLast()
                assert np.array_equal(idx, r["idx"]), where                                # k = 2: drawn from the prefix update 1 left
                assert np.array_equal(like.astype(np.float64) * 0.5, r["raw"]), where
                assert _bits(pose) == _bits(r["pose"]), where + ((pose.x, pose.y, pose.theta), (r["pose"].x, r["pose"].y, r["pose"].theta),
                                                                 pf.debugEstimateStats())
                if cloud == "origin" and N >= 4099:
                    # a sum that hovers around zero leaves its binade every few terms (a third of the sub-tiles): behind the
                    # pre-chain's nine sub-tiles some must have gone by a replay, a table or the slow walk -- the branches the predictions
                    # (now summed on DPP) steer
                    stats = pf.debugEstimateStats()
                    print("estimate stats", where, stats)
                    assert sum(stats) > 0, where + (stats,)
                if k == 1:
                    got = pf.particles()
                    for f in ("x", "y", "theta"):
                        assert np.array_equal(got[f], after[f]), where + (f,)
                    assert np.allclose(got["weight"], after["weight"], rtol=1e-5, atol=0), where
        finally:
            mapper.close(); pf.close(); g.close(); gm.close()
