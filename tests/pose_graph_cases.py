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
    # the two converged statuses by name: _converged takes either
    add("n64_fixed_last", loop_graph(64, 3, seed=6)[0], P._replace(fixed=63),
        condition=lambda r: _converged(r) and (r.status & 15) == pgm.CONVERGED_STEP, why="fixed = N - 1; ends by the step rule after an accepted step")
    add("n100_fixed_mid", loop_graph(100, 3, seed=7)[0], P._replace(fixed=50),
        condition=lambda r: _converged(r) and (r.status & 15) == pgm.CONVERGED_DECREASE, why="fixed in the middle; ends by the relative-decrease rule")
    add("n64_repeated_pair", loop_graph(64, 0, seed=8, loops=[(3, 35), (3, 35), (35, 3)])[0], why="a pair three times, once reversed")
    g_held = loop_graph(64, 0, seed=9, loops=[(0, 32), (40, 0)])[0]
    add("n64_loop_on_fixed", g_held, condition=lambda r, g=g_held: _converged(r) and r.trial_wrapped and bool(np.all(np.abs(g.nodes[:, 2]) < pgm.PI)),
        why="loop edges on the held node 0; a trial heading x + dx leaves [-pi, pi] though every node starts strictly inside")
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


HUB, HUB_EDGES = 7, 600
F32_PI = float(np.float32(math.pi))             # 3.1415927410125732 > PG_PI: a float heading of pi lies outside [-PG_PI, PG_PI] in double


def hub_loops(N=48, L=1024, seed=48):
    """loop edges 0 .. HUB_EDGES - 1 touch node HUB, alternately as i and as j; the others are random pairs, repeats allowed"""
    rng = np.random.default_rng(seed)
    loops = []
    for l in range(HUB_EDGES):
        o = int(rng.integers(0, N - 1))
        o = o + 1 if o >= HUB else o
        loops.append((HUB, o) if l % 2 == 0 else (o, HUB))
    for l in range(L - HUB_EDGES):
        i, j = int(rng.integers(0, N)), int(rng.integers(0, N - 1))
        loops.append((i, j + 1 if j >= i else j))
    return loops


def pi_headings_graph(seed=41):
    """64 nodes, two loop edges; the two free nodes nearest +pi are set to exactly +float32(pi), the two nearest -pi to -float32(pi)
    (none among the first eight: a node beside the held one hardly moves and would end within rounding of +-pi, where a heading and
    its other representation differ by 2 pi), and the chain is made consistent with the nodes by the residual's own statements."""
    g0, _ = loop_graph(64, 2, seed=seed, start_heading=math.pi - 0.05)
    nodes = g0.nodes.copy()
    k = np.arange(8, 64)
    up = k[np.argsort(np.abs(nodes[k, 2] - math.pi))[:2]]
    down = k[np.argsort(np.abs(nodes[k, 2] + math.pi))[:2]]
    nodes[up, 2], nodes[down, 2] = F32_PI, -F32_PI
    z = pgm.relative_pose(nodes[:-1], nodes[1:])
    return pgm.Graph(nodes, g0.i, g0.j, np.concatenate([z, g0.z[63:]]), g0.info)


def _power_of(final, lambda0, up, most):
    lam = lambda0
    for _ in range(most + 1):
        if lam == final:
            return True
        lam = lam * up
    return False


_edge_cases = None


def edge_cases():
    """The limits cases() does not reach: loop edges past one trip of the workgroup and past two mask words, a long node list, float
    headings of +-pi, and the accepted parameter values at the ends of their ranges."""
    global _edge_cases
    if _edge_cases is not None:
        return _edge_cases
    P = pgm.DEFAULT
    out = []

    def add(name, graph, params=P, condition=_converged, why="converges"):
        out.append(Case(name, graph, params, None, condition, why))

    hub = loop_graph(48, 0, seed=48, loops=hub_loops())[0]
    add("n48_l1024_hub", hub,
        condition=lambda r, g=hub: _converged(r) and g.L == 1024 and r.node_lists[HUB] >= pgm.PG_T + 1 and r.node_lists.sum() == 2 * 1024,
        why="L = 1024: two trips of the set-up, 32 mask words, entries up to 2047, a node list of more than 512 entries, three loop terms a thread in the cost")
    g600 = loop_graph(600, 513, seed=600)[0]
    add("n600_l513", g600, condition=lambda r, g=g600: _converged(r) and g.N > pgm.PG_T and g.L == pgm.PG_T + 1, why="N and L one trip past PG_T")
    g97 = loop_graph(64, 97, seed=97)[0]
    add("n64_l97", g97, condition=lambda r, g=g97: _converged(r) and g.L == 97 and r.node_lists.sum() == 2 * 97, why="four mask words, the last holding one bit")
    gpi = pi_headings_graph()
    add("n64_pi_headings", gpi,
        condition=lambda r, g=gpi: _converged(r) and r.trial_wrapped and g.nodes[0, 2] != F32_PI and
        int(np.sum(g.nodes[1:, 2] == F32_PI)) >= 1 and int(np.sum(g.nodes[1:, 2] == -F32_PI)) >= 1 and F32_PI > pgm.PI,
        why="free nodes at exactly +-float32(pi), outside +-PG_PI in double; a trial heading wraps")
    # accepted parameter values at the ends of their ranges
    g30, g31 = loop_graph(64, 3, seed=30)[0], loop_graph(64, 3, seed=31)[0]
    add("n64_lambda0_zero", g30, P._replace(lambda0=0.0), condition=lambda r: r.final_lambda == 0.0 and r.accepted >= 1 and r.cost_after < r.cost_before,
        why="lambda0 = 0: no damping, and lambda stays 0 whatever the tries do")
    add("n64_lambda_down_one", g30, P._replace(lambda_down=1.0),
        condition=lambda r: _converged(r) and r.tries > r.accepted and _power_of(r.final_lambda, P.lambda0, P.lambda_up, r.tries),
        why="lambda_down = 1: lambda only ever rises, final_lambda = lambda0 times a power of lambda_up")
    add("n64_max_cg_one", g30, P._replace(max_cg=1), condition=lambda r: all(n == 1 for n in r.cg_per_try) and bool(r.status & pgm.CG_CAP) and r.accepted >= 1,
        why="max_cg = 1: every try is one iteration, ended by the cap")
    add("n64_cg_tol_zero", g31, P._replace(cg_tol=0.0),
        condition=lambda r: _converged(r) and not (r.status & pgm.CG_CAP) and all(end == "tol" and rz == 0.0 for end, rz in r.cg_ends),
        why="cg_tol = 0: the iteration ends only at r' T^-1 r == 0 exactly")
    _edge_cases = out
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
