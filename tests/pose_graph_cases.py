"""Named graphs for the pose-graph tests.  Each case carries the condition that shows it reaches its path, evaluated on the model's
trace (tests/pose_graph_model.py): a case whose condition does not hold in the model is a broken case, and the tests assert it.

Nodes are float32 values (the device takes bl_pose_xyt_t), edges are doubles.
"""
import math
from collections import namedtuple

import numpy as np

import pose_graph_model as pgm

Case = namedtuple("Case", "name graph params masks condition why")


def _rel(a, b):
    c, s = math.cos(a[2]), math.sin(a[2])
    dx, dy = b[0] - a[0], b[1] - a[1]
    d = (b[2] - a[2] + math.pi) % (2 * math.pi) - math.pi
    return np.array([c * dx + s * dy, -s * dx + c * dy, d])


def loop_graph(N, L, seed=0, drift=0.002, loop_sigma=(0.02, 0.02, 0.01), loop_info=None, loops=None, start_heading=None, radius=3.0,
               odo_sigma=(0.01, 0.01, None)):
    """Two laps of a circle: odometry with noise, dead reckoning for the nodes, loop edges between the laps."""
    rng = np.random.default_rng(seed)
    t = np.arange(N) / max(N / 2.0, 1.0) * 2 * math.pi
    h0 = math.pi / 2 if start_heading is None else start_heading
    truth = np.stack([radius * np.cos(t), radius * np.sin(t), (t + h0 + math.pi) % (2 * math.pi) - math.pi], 1)
    so = np.array([odo_sigma[0], odo_sigma[1], drift if odo_sigma[2] is None else odo_sigma[2]])
    info_o = np.array([1 / so[0] ** 2, 0.0, 1 / so[1] ** 2, 0.0, 0.0, 1 / so[2] ** 2])
    ei, ej, z, info = [], [], [], []
    x = np.zeros((N, 3))
    x[0] = truth[0]
    for k in range(N - 1):
        zk = _rel(truth[k], truth[k + 1]) + rng.normal(0, so)
        ei.append(k); ej.append(k + 1); z.append(zk); info.append(info_o)
        c, s = math.cos(x[k, 2]), math.sin(x[k, 2])
        x[k + 1] = [x[k, 0] + c * zk[0] - s * zk[1], x[k, 1] + s * zk[0] + c * zk[1], (x[k, 2] + zk[2] + math.pi) % (2 * math.pi) - math.pi]
    sl = np.array(loop_sigma)
    info_l = np.array([1 / sl[0] ** 2, 0.0, 1 / sl[1] ** 2, 0.0, 0.0, 1 / sl[2] ** 2]) if loop_info is None else np.asarray(loop_info, float)
    if loops is None:
        loops = []
        for _ in range(L):
            i = int(rng.integers(0, max(N // 2 - 1, 1)))
            loops.append((i, min(i + N // 2, N - 1)))
    for (i, j) in loops:
        ei.append(i); ej.append(j); z.append(_rel(truth[i], truth[j]) + rng.normal(0, sl)); info.append(info_l)
    nodes = x.astype(np.float32).astype(np.float64)
    return pgm.Graph(nodes, ei, ej, np.array(z), np.array(info)), truth


def _converged(r):
    return (r.status & 15) in (pgm.CONVERGED_STEP, pgm.CONVERGED_DECREASE) and r.accepted >= 1 and r.cost_after < r.cost_before


def _levels(n):
    return int(math.floor(math.log2(n))) + 1


def all_on(L, n=1):
    return np.full((n, max((L + 31) // 32, 1)), 0xffffffff, np.uint32)


def cases():
    P = pgm.DEFAULT
    out = []

    def add(name, graph, params=P, masks=None, condition=_converged, why="converges"):
        out.append(Case(name, graph, params, masks, condition, why))

    # sizes: the minimum, the first loop, a node count past every level of the cyclic reduction, more nodes and edges than threads
    g2, _ = loop_graph(2, 0, seed=1)
    g2.z[0] = g2.z[0] + np.array([0.05, -0.02, 0.01])
    add("n2_chain_only", g2, why="N = 2: one chain edge that disagrees with the nodes")
    add("n3_loop_0_2", loop_graph(3, 0, seed=2, loops=[(0, 2)])[0], why="N = 3 with the loop (0, 2)")
    for n, l in ((5, 1), (9, 2), (17, 2), (33, 3), (64, 1), (65, 4), (100, 32), (129, 5), (257, 33), (513, 8), (1025, 8), (2049, 8)):
        add("n%d_l%d" % (n, l), loop_graph(n, l, seed=n)[0], P._replace(fixed=(0, n - 1, n // 2)[n % 3]),
            condition=lambda r, n=n: _converged(r), why="%d levels of reduction, fixed %d" % (_levels(n), (0, n - 1, n // 2)[n % 3]))
    add("n64_l0", loop_graph(64, 0, seed=5)[0], condition=lambda r: r.accepted >= 1 and r.cg_per_try[0] == 1, why="no loop edge: the preconditioner is H, one iteration")
    add("n64_fixed_last", loop_graph(64, 3, seed=6)[0], P._replace(fixed=63), why="fixed = N - 1")
    add("n100_fixed_mid", loop_graph(100, 3, seed=7)[0], P._replace(fixed=50), why="fixed in the middle")
    add("n64_repeated_pair", loop_graph(64, 0, seed=8, loops=[(3, 35), (3, 35), (35, 3)])[0], why="a pair three times, once reversed")
    add("n64_loop_on_fixed", loop_graph(64, 0, seed=9, loops=[(0, 32), (40, 0)])[0], why="loop edges on the held node 0")
    add("n64_adjacent_loop", loop_graph(64, 0, seed=10, loops=[(10, 11), (5, 37)])[0], why="a loop edge between chain neighbours")
    add("n64_across_pi", loop_graph(64, 2, seed=11, start_heading=math.pi - 0.05)[0], condition=lambda r: _converged(r) and r.wrapped,
        why="some |theta_j - theta_i - z_theta| > pi before the wrap")
    add("n64_full_info", loop_graph(64, 3, seed=12, loop_info=[2500.0, 300.0, 2000.0, -150.0, 90.0, 8000.0])[0], why="a full information matrix")
    add("n64_semidefinite", loop_graph(64, 3, seed=13, loop_info=[2500.0, 0.0, 0.0, 0.0, 0.0, 10000.0])[0], why="no information along y")
    gz, _ = loop_graph(64, 3, seed=14)
    gz.info[64] = 0.0
    add("n64_zero_info", gz, why="loop edge 1 carries no information")
    # step control and status
    add("n64_rejected_try", loop_graph(64, 2, seed=22)[0], condition=lambda r: _converged(r) and r.tries > r.accepted, why="a try is rejected")
    add("n64_out_of_tries", loop_graph(64, 2, seed=16)[0], P._replace(max_tries=1, step_tol=0.0, rel_tol=0.0),
        condition=lambda r: (r.status & 15) == pgm.OUT_OF_TRIES and r.tries == 1, why="max_tries spent")
    add("n100_cg_cap", loop_graph(100, 8, seed=17)[0], P._replace(max_cg=3), condition=lambda r: bool(r.status & pgm.CG_CAP),
        why="the iteration cap ends the conjugate gradients")
    return out


def subset_masks(L, n_subsets, seed=0):
    """n_subsets masks over L loop edges: all on, all off, each edge alone in turn, then random ones"""
    words = max((L + 31) // 32, 1)
    rng = np.random.default_rng(seed)
    m = np.zeros((n_subsets, words), np.uint32)
    for s in range(n_subsets):
        if s == 0:
            m[s] = 0xffffffff
        elif s == 1:
            m[s] = 0
        elif s - 2 < L:
            m[s, (s - 2) >> 5] = np.uint32(1) << np.uint32((s - 2) & 31)
        else:
            m[s] = rng.integers(0, 1 << 32, words, dtype=np.uint64).astype(np.uint32)
    return m


def large_case():
    """N = 4096, L = 64"""
    return Case("n4096_l64", loop_graph(4096, 64, seed=4096, drift=0.0005)[0], pgm.DEFAULT, None, _converged, "13 levels, 8 nodes a thread")
