"""The map update that runs ahead of the filter's exact pose (bl_mapping.hip, k_map_update carrying the filter's finish): both of
its branches on a real SLAM sequence.

The map workgroup traces the rays with its own double-precision weighted mean of x and y, and when the finisher's exact x, y -- the
reference's serially rounded float sums -- arrive, places the rays again (bl_ray_place: the angle part of a ray does not depend on
x or y).  Equal cells: the counts stand and only the stores remain.  Any cell different: everything runs again with the exact pose.

Which steps of the sequence must run again is worked out on the CPU from the oracle's particles (the double weighted mean, the
exact estimate, rb_slam_model.ray_cells for both) and held against bl_pf_debug_lookahead: the sequence contains steps of both
kinds.  After every step the map is OracleMapping's byte for byte, and so is the replanner's snapshot (bl_planner_debug_snapshot;
the path planned on it is the one the synchronous planner finds on the map itself); the zero-framed copy the filter reads through the next update's
likelihoods."""
import numpy as np
import pytest

import botlab_amd as bl
import helpers
import oracle_lib
import rb_slam_model as rbm
from botlab_amd import synth

pytestmark = pytest.mark.gpu

MAP = "obstacle_slam_10mx10m_5cm"
N = 4096
SEED = 13               # chosen on the CPU (sequence_with_predictions with ulp_margin): step 1 must run again, steps 2 and 3 must not,
STEPS = 4                # and no verdict changes with the provisional x, y one ulp either way; step 0 latches filter and mapper
MAX_LASER, HIT, MISS = 5.0, 4, 1
START = (-0.75, 0.2, 0.0)
GOAL = (-0.35, 0.2)


def provisional_xy(parts):
    """The map workgroup's x, y: double sums of weight * coordinate over the total weight, narrowed to float."""
    w = parts["weight"].astype(np.float64)
    return (np.float32(np.dot(w, parts["x"].astype(np.float64)) / w.sum()), np.float32(np.dot(w, parts["y"].astype(np.float64)) / w.sum()))


def sequence_with_predictions(oracle, maps, seed=SEED, steps=STEPS, ulp_margin=False):
    """The oracle's run of the sequence: per step its filter result, the map after its map update, and whether a look-ahead with the
    provisional pose must run again.  ulp_margin: also say whether the verdict stands with the provisional x, y one ulp either way."""
    m = maps[MAP]
    truth = np.where(m["cells"] > 0, 127, -127).astype(np.int8)
    poses = synth.square_trajectory(START, steps, step_len=0.04, side=0.8)
    scans = [synth.raycast_scan(truth, m["origin"], 0.05, poses[k - 1], poses[k], 1_000_000 + 100_000 * k) for k in range(1, len(poses))]
    cells = m["cells"].copy()
    frame = (m["mpc"], helpers.CPM_DEFAULT, m["origin"])
    opf = oracle_lib.OraclePF(oracle, N)
    opf.init_at_pose(oracle.pose(*START, utime=int(scans[0].times[0])), seed)
    first = opf.particles()
    om = oracle_lib.OracleMapping(oracle, MAX_LASER, HIT, MISS)
    out, prev, firm = [], None, True
    for k, sc in enumerate(scans):
        res = opf.update(oracle.pose(*poses[k + 1], utime=sc.utime), sc, cells, *frame, 1000 + k)
        e = res["pose"]
        again = False
        if res["moved"] and prev is not None:
            px, py = provisional_xy(opf.particles())
            exact = rbm.ray_cells(oracle, sc, prev, e, m["origin"], helpers.CPM_DEFAULT, MAX_LASER)
            verdicts = set()
            for dx in ((-1, 0, 1) if ulp_margin else (0,)):
                for dy in ((-1, 0, 1) if ulp_margin else (0,)):
                    qx = np.float32(px) if dx == 0 else np.nextafter(np.float32(px), np.float32(dx * np.inf))
                    qy = np.float32(py) if dy == 0 else np.nextafter(np.float32(py), np.float32(dy * np.inf))
                    prov = rbm.ray_cells(oracle, sc, prev, oracle.pose(float(qx), float(qy), e.theta, utime=e.utime), m["origin"], helpers.CPM_DEFAULT, MAX_LASER)
                    v = not np.array_equal(prov, exact)
                    verdicts.add(v)
                    if dx == 0 and dy == 0:
                        again = v
            firm = firm and len(verdicts) == 1
        if k == 0:
            e = oracle.pose(*START, utime=sc.utime)                     # the pose the mapper is handed where the filter only latched
        om.update(sc, oracle.pose(e.x, e.y, e.theta, utime=e.utime), cells, *frame)
        prev = oracle.pose(e.x, e.y, e.theta, utime=e.utime)
        out.append(dict(res=res, cells=cells.copy(), again=again))
    return m, poses, scans, first, out, firm


def test_both_branches_on_a_slam_sequence(oracle, maps, gpu_ctx):
    m, poses, scans, first, want, firm = sequence_with_predictions(oracle, maps, ulp_margin=True)
    assert firm                     # the device forms its provisional x, y from block sums in another order: no verdict within an ulp of flipping
    moved = [bool(w["res"]["moved"]) for w in want]
    assert moved == [False] + [True] * (len(want) - 1)                          # (the first update latches the odometry, the first map update the pose)
    n_again = sum(int(w["again"]) for w in want)
    assert n_again >= 1 and sum(int(mv and not w["again"]) for mv, w in zip(moved, want)) >= 1, [w["again"] for w in want]
    g = bl.OccupancyGrid.from_cells(m["cells"], m["origin"], m["mpc"], cellsPerMeter=helpers.CPM_DEFAULT, ctx=gpu_ctx)
    pf = bl.ParticleFilter(N, ctx=gpu_ctx)
    mapper = bl.Mapping(MAX_LASER, HIT, MISS, ctx=gpu_ctx)
    aplanner = bl.AsyncPlanner(ctx=gpu_ctx, lanes=1, batch=1)
    planner = bl.MotionPlanner(ctx=gpu_ctx)
    goal = bl.make_pose(*GOAL, 0.0)
    try:
        pf.setParticles(first)
        pf.debugEnable(True)
        assert pf.debugLookahead() == (0, 0)
        for k, (sc, w) in enumerate(zip(scans, want)):
            r = w["res"]
            if k == 0:
                # the filter latches its odometry, the mapper its pose (handed over from the host): nothing rides, nothing runs ahead
                pf.updateFilter(bl.make_pose(*poses[1], utime=sc.utime), sc, g, rand_value=1000, noise=r["noise"], want_pose=False)
                mapper.updateMap(sc, bl.make_pose(*START, utime=sc.utime), g)
                assert np.array_equal(g.cells(), w["cells"])
                assert pf.debugLookahead() == (0, 0)
                continue
            assert pf.updateBegin(bl.make_pose(*poses[k + 1], utime=sc.utime), sc, g, 1000 + k, noise=r["noise"])
            aplanner.submit_with_map_update_finishing(mapper, sc, pf, sc.utime, g, goal)
            path = aplanner.fetch()                                     # planned on the snapshot the map kernel left behind
            assert np.array_equal(aplanner.debugSnapshot(g), w["cells"]), k             # the snapshot is the map, cell for cell
            pose = pf.poseEstimate()
            idx, like = pf.debugLast()
            assert np.array_equal(idx, r["idx"]), k
            assert np.array_equal(like.astype(np.float64) * 0.5, r["raw"]), k          # read from the framed copy the last map update wrote
            got = np.array([pose.x, pose.y, pose.theta], np.float32).view(np.uint32)
            exp = np.array([r["pose"].x, r["pose"].y, r["pose"].theta], np.float32).view(np.uint32)
            assert np.array_equal(got, exp), k
            assert np.array_equal(g.cells(), w["cells"]), (k, int((g.cells() != w["cells"]).sum()))
            planner.setMap(g)
            bl.search_for_path_begin(goal, planner.distances_, planner.searchParams_, start_dev=pf.poseDevicePtr())
            direct = bl.search_for_path_end(planner.distances_)
            assert [(p.utime, p.x, p.y, p.theta) for p in path] == [(p.utime, p.x, p.y, p.theta) for p in direct], k
            assert pf.debugLookahead() == (sum(moved[:k + 1]), sum(int(v["again"]) for v in want[:k + 1])), (k, [v["again"] for v in want])
    finally:
        aplanner.close(); mapper.close(); pf.close(); g.close()


# ------------------------------------------------------------------ hand-built scans for the end cells the leaders tag
# In the dword form of the window pass a leader leaves its end cell's finished value in its u16 counter, tagged, in front of the wait
# for the exact pose, and the window threads form their dwords in registers from counts and tagged values alike (bl_mapping.hip).
# The scans are arrays written by hand in the robot's frame, in the style of tests/mapping_cases.py; the conditions below prove on
# the CPU, on the oracle's ray cells, that each scan holds what it is there for.  Every case runs through Mapping::updateMap with the
# pose handed over, and with the filter's finish riding in the map kernel (a filter of identical particles and no noise: its
# estimate is the particles' pose, which the oracle's filter gives bit for bit).
import math

import mapping_cases as mc

START_VALUES = np.array([127, -128, 0], np.int8)
HAND_ODDS = [(127, 127), (4, 1)]
HAND_GRIDS = {"dword_200x200": (200, 200, False), "whole_200x200": (200, 200, True), "byte_203x197": (203, 197, False)}
HAND_N = 64


def _hand_scan(whole, t0, t1):
    """Along the heading (stamped t1, so that equal rays are equal rays): ends in four neighbouring cells -- every place in a
    dword --, one of them hit twice and one three times, and a longer ray that crosses them all.  A few rays elsewhere.  whole: four
    rays past the grid's corners, so that the window is the whole grid."""
    ranges = [1.0, 1.05, 1.05, 1.10, 1.10, 1.10, 1.15, 2.0]
    dirs = [0.0] * len(ranges)
    times = [t1] * len(ranges)
    rng = np.random.default_rng(31)
    extra = 40
    ranges += list(rng.uniform(0.3, 2.5, extra)); dirs += list(rng.uniform(-math.pi, math.pi, extra))
    times += list(mc._times(extra, t0, t1))
    if whole:
        ranges += [7.6] * 4; dirs += [math.pi / 4, 3 * math.pi / 4, -math.pi / 4, -3 * math.pi / 4]; times += [t1] * 4
    return mc._scan(ranges, dirs, t0, t1, times=np.asarray(times, np.int64))


def hand_case(oracle, grid, hit, miss):
    W, H, whole = HAND_GRIDS[grid]
    yy, xx = np.mgrid[0:H, 0:W]
    start = START_VALUES[(xx + 2 * yy) % 3]
    case = mc.Case(f"tagged_{grid}_{hit}_{miss}", W, H, 0.05, 8.0, hit, miss, start, None, None)
    x0, y0 = case.centre_of(W // 2 + 0.5, H // 2 + 0.5)
    odo = [(x0 + 0.03 * k, y0, 0.0) for k in range(4)]
    t = [1_000_000 + 100_000 * k for k in range(4)]
    scans = [_hand_scan(whole, t[k] - 100_000, t[k]) for k in range(4)]
    # the filter's poses: identical particles, no noise -- whatever the map says, they keep equal weights
    p = np.zeros(HAND_N, bl.host.PARTICLE_DTYPE)
    p["x"], p["y"], p["theta"] = np.float32(odo[0][0]), np.float32(odo[0][1]), 0.0
    p["p_x"], p["p_y"], p["p_theta"] = p["x"], p["y"], p["theta"]
    p["utime"] = p["p_utime"] = t[0]
    p["weight"] = 1.0 / HAND_N
    opf = oracle_lib.OraclePF(oracle, HAND_N)
    opf.set_particles(p)
    zeros = np.zeros(3 * HAND_N, np.float32)
    poses, results = [], []
    for k in range(4):
        r = opf.update(oracle.pose(*odo[k], utime=t[k]), scans[k], start, case.mpc, case.cpm, case.origin, 500 + k, noise_in=zeros)
        assert r["moved"] == (k > 0)
        if k == 0:
            opf.set_particles(p)
        e = r["pose"]
        poses.append((float(np.float32(odo[0][0])), float(np.float32(odo[0][1])), 0.0, t[0]) if k == 0 else (e.x, e.y, e.theta, t[k]))
        results.append(r)

    def condition(case, refs, geo):
        seen = set()
        for g in geo[1:]:
            c = g["cells"]
            w = mc.window(case, g)
            assert w["dword"] == (W % 4 == 0) and w["rows_per_strip"] == w["wh"] and g["kept"] <= mc.SEG_RAYS
            if whole:
                assert w["cells"] == W * H and W * H // 4 > 2 * 4 * 1024        # more items than two batches of a workgroup hold
            ends, n = np.unique(c[:, 2:], axis=0, return_counts=True)
            assert 2 in n and 3 in n                                             # two and three rays ending in one cell
            crossed = {}
            for ray in c:
                for cell in mc.walk(*[int(v) for v in ray]):
                    crossed[cell] = crossed.get(cell, 0) + 1
            inside = [(int(e[0]), int(e[1])) for e in ends if 0 <= e[0] < W and 0 <= e[1] < H]
            assert any(e in crossed for e in inside)                             # an end cell that other rays cross
            mates = [e for e in inside if any((4 * (e[0] // 4) + j, e[1]) in crossed and (4 * (e[0] // 4) + j, e[1]) not in inside for j in range(4))]
            assert mates                                                         # an end cell sharing a dword with crossed cells
            assert {e[0] % 4 for e in inside} == {0, 1, 2, 3}
            seen |= {int(start[e[1], e[0]]) for e in inside}
        assert seen == {127, -128, 0}
        assert not np.array_equal(refs[-1], refs[-2])

    case.updates = [(scans[k], poses[k]) for k in range(4)]
    case.condition = condition
    return case, odo, results, p


@pytest.mark.parametrize("hit,miss", HAND_ODDS)
@pytest.mark.parametrize("grid", list(HAND_GRIDS))
def test_tagged_end_cells_by_hand(oracle, gpu_ctx, grid, hit, miss):
    case, odo, results, p = hand_case(oracle, grid, hit, miss)
    refs, _ = mc.evaluate(case, oracle)
    for riding in (False, True):
        g = bl.OccupancyGrid.from_cells(case.start, case.origin, case.mpc, ctx=gpu_ctx)
        fmap = bl.OccupancyGrid.from_cells(case.start, case.origin, case.mpc, ctx=gpu_ctx)      # the filter's map (its weights do not matter here)
        mapper = bl.Mapping(case.max_laser, case.hit, case.miss, ctx=gpu_ctx)
        pf = bl.ParticleFilter(HAND_N, ctx=gpu_ctx)
        try:
            pf.setParticles(p)
            for k, (scan, q) in enumerate(case.updates):
                if riding and k > 0:
                    assert pf.updateBegin(bl.make_pose(*odo[k], utime=q[3]), scan, fmap, 500 + k, noise=np.zeros(3 * HAND_N, np.float32))
                    mapper.updateMapFinishingFilter(scan, pf, q[3], g)
                    est = pf.poseEstimate()
                    assert (est.x, est.y, est.theta) == (q[0], q[1], q[2]), (k, (est.x, est.y, est.theta), q)
                else:
                    if riding:
                        pf.updateFilter(bl.make_pose(*odo[0], utime=q[3]), scan, fmap, rand_value=500, noise=np.zeros(3 * HAND_N, np.float32), want_pose=False)
                        pf.setParticles(p)
                    mapper.updateMap(scan, bl.make_pose(q[0], q[1], q[2], utime=q[3]), g)
                got = g.cells()
                diff = np.nonzero(got != refs[k])
                assert diff[0].size == 0, (case.name, riding, k, int(diff[0].size), [(int(x), int(y), int(got[y, x]), int(refs[k][y, x])) for y, x in zip(diff[0][:6], diff[1][:6])])
            if riding:
                assert pf.debugLookahead()[0] == 3
        finally:
            pf.close(); mapper.close(); g.close(); fmap.close()
