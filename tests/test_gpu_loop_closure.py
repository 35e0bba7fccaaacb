"""Loop closure end to end on the device: botlab_amd.find_loop_closures (scan history + map rebuild + scan matcher) makes the loop
edges, botlab_amd.close_loops gates them through the pose graph's subsets and corrects the history, and the map rebuilt at the
corrected poses is closer to the map at the true poses than the map at the recorded ones.

The world is a 200 x 200 one from botlab_amd.synth (10 m a side, four blocks, a border).  The robot drives a circle of 1.5 m radius
twice, 80 scans a lap, and stands still for each scan (every ray carries the scan's end time, so the mapper takes the pose itself).
The scans are ray-cast at the truth; the recorded poses are the truth's steps replayed with a constant heading bias of 0.4 mrad
added to every step, so the second lap comes back 32 mrad and some centimetres off the first."""
import math

import numpy as np
import pytest

import botlab_amd as bl
from botlab_amd import synth

pytestmark = pytest.mark.gpu

SIZE, MPC, ORIGIN = 200, 0.05, (-5.0, -5.0)
LAP, N, RADIUS, BIAS = 80, 160, 1.5, 0.0004
DTHETA = math.radians(0.5)
MAX_LASER, HIT, MISS = 5.0, 3, 1
# odometry as the chain believes it: 5 mm and 3 mrad a step (untuned; the bias is 0.13 of the heading sigma)
CHAIN_INFO = np.array([1 / 0.005 ** 2, 0.0, 1 / 0.005 ** 2, 0.0, 0.0, 1 / 0.003 ** 2])


def _rel(a, b):
    c, s = math.cos(a[2]), math.sin(a[2])
    dx, dy = b[0] - a[0], b[1] - a[1]
    return np.array([c * dx + s * dy, -s * dx + c * dy, math.atan2(math.sin(b[2] - a[2]), math.cos(b[2] - a[2]))])


def _world():
    cells = np.zeros((SIZE, SIZE), np.int8)
    for y0, y1, x0, x1 in ((60, 75, 40, 60), (130, 150, 150, 165), (30, 45, 140, 170), (150, 170, 50, 60)):
        cells[y0:y1, x0:x1] = 100
    return synth.tile_world(cells, SIZE)


def _trajectories():
    t = np.arange(N) / LAP * 2 * math.pi
    truth = np.stack([RADIUS * np.cos(t), RADIUS * np.sin(t), np.arctan2(np.sin(t + math.pi / 2), np.cos(t + math.pi / 2))], 1)
    rec = np.zeros_like(truth)
    rec[0] = truth[0]
    for k in range(N - 1):
        z = _rel(truth[k], truth[k + 1])
        c, s = math.cos(rec[k, 2]), math.sin(rec[k, 2])
        th = rec[k, 2] + z[2] + BIAS
        rec[k + 1] = [rec[k, 0] + c * z[0] - s * z[1], rec[k, 1] + s * z[0] + c * z[1], math.atan2(math.sin(th), math.cos(th))]
    return truth, rec


def _poses(xyt):
    p = np.zeros(len(xyt), bl.POSE_DTYPE)
    p["utime"] = 100000 * (np.arange(len(xyt)) + 1)
    p["x"], p["y"], p["theta"] = xyt[:, 0], xyt[:, 1], xyt[:, 2]
    return p


def _scans(world, truth, utimes):
    """ray-cast at the truth, the robot standing still: every ray carries the scan's end time"""
    out = []
    for k in range(len(truth)):
        s = synth.raycast_scan(world, ORIGIN, MPC, truth[k], truth[k], int(utimes[k]))
        out.append(bl.LidarScan(s.ranges, s.thetas, np.full(s.num_ranges, int(utimes[k]), np.int64), utime=int(utimes[k])))
    return out


def _map(ctx, history, poses):
    g = bl.OccupancyGrid(SIZE * MPC, SIZE * MPC, MPC, ctx=ctx)
    history.rebuild(g, MAX_LASER, HIT, MISS, poses=poses)
    cells = g.cells()
    g.close()
    return cells


def test_loop_closure_corrects_the_history_and_the_map(gpu_ctx):
    world = _world()
    truth, rec = _trajectories()
    history = bl.ScanHistory(N, synth.RAYS, ctx=gpu_ctx)
    rec_p, truth_p = _poses(rec), _poses(truth)
    for k, s in enumerate(_scans(world, truth, rec_p["utime"])):
        history.append(s, bl.make_pose(rec[k, 0], rec[k, 1], rec[k, 2], utime=int(rec_p["utime"][k])))
    like = bl.OccupancyGrid(SIZE * MPC, SIZE * MPC, MPC, ctx=gpu_ctx)
    matcher = bl.ScanMatcher(ctx=gpu_ctx)
    graph = bl.PoseGraph(N, 64, 65, ctx=gpu_ctx)
    try:
        map_true, map_rec = _map(gpu_ctx, history, truth_p), _map(gpu_ctx, history, None)
        edges = bl.find_loop_closures(history, matcher, like, stride=4, min_gap=40, radius=0.5, w=5, submap_cells=200, nx=8, ny=8, ntheta=12,
                                      dtheta=DTHETA, max_range=8.0, half_life=64, maxLaserDistance=MAX_LASER, hitOdds=HIT, missOdds=MISS)
        print("loop edges found:", len(edges))
        assert len(edges) >= 1
        for e in edges:
            want = _rel(truth[e["i"]], truth[e["j"]])
            d = e["z"] - want
            d[2] = math.atan2(math.sin(d[2]), math.cos(d[2]))
            print("edge", e["i"], e["j"], "z - truth", d, "info", e["info"])
        # a planted false edge: the first true edge's z shifted by 10 cells
        false = edges[:1].copy()
        false["z"][0, 0] += 10 * MPC
        cand = np.concatenate([edges, false])
        kept, results, poses, alone = bl.close_loops(history, graph, cand, CHAIN_INFO)
        print("alone costs", alone)
        print("kept", len(kept), "of", len(cand), "result", results[0])
        assert alone[-1] > 11.345 and not any(k.tobytes() == false[0].tobytes() for k in kept)
        assert len(kept) >= 1
        for e in kept:
            d = e["z"] - _rel(truth[e["i"]], truth[e["j"]])
            assert abs(d[0]) <= MPC and abs(d[1]) <= MPC and abs(math.atan2(math.sin(d[2]), math.cos(d[2]))) <= DTHETA, (e, d)
        before, after = graph.edge_chi2(0)
        print("summed chi2 of the kept loop edges: before", before[N - 1:].sum(), "after", after[N - 1:].sum())
        assert after[N - 1:].sum() < before[N - 1:].sum()
        got = history.poses()
        assert got.tobytes() == poses.tobytes()                        # the history holds the corrected poses
        map_cor = _map(gpu_ctx, history, None)
        n_rec, n_cor = int(np.count_nonzero(map_rec != map_true)), int(np.count_nonzero(map_cor != map_true))
        n_self = int(np.count_nonzero(map_true != 0))
        print("cells differing from the map at the true poses: recorded", n_rec, "corrected", n_cor, "(cells the true map knows:", n_self, ")")
        err_rec = np.abs(rec[:, :2] - truth[:, :2]).max()
        err_cor = max(np.abs(poses["x"] - truth[:, 0]).max(), np.abs(poses["y"] - truth[:, 1]).max())
        print("largest position error: recorded %.3f m, corrected %.3f m" % (err_rec, err_cor))
        assert n_cor < n_rec
    finally:
        graph.close(); matcher.close(); like.close(); history.close()
