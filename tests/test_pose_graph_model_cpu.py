"""tests/pose_graph_model.py, the restatement the device is compared with bit for bit, against an independent dense solve (plain normal
equations through np.linalg.solve with the same step control) on every graph of tests/pose_graph_cases.py, and the properties the
solver's contract names.

Agreement with the dense solve is bounded, not exact: LAPACK's order is not the model's, and the two stop within the tolerances of the
optimum from different sides.  Measured on the machine this was written on, over the cases that end converged: the largest pose
difference 8.9e-6 (n9_l2, ended by the relative-decrease rule one accepted step before the dense solve), the largest relative cost
difference 8.4e-5 (n64_l0).  The bounds are four times those: other builds of LAPACK round differently.  A cost is compared relative to
max(cost, 1e-6): with no loop edge the optimum is 0, and a pose error of step_tol = 1e-6 under the largest information of the cases,
2.5e5, already costs 2.5e-7 -- below 1e-6 a cost is zero to within the stop rule.
"""
import math
import time

import numpy as np
import pytest

import pose_graph_cases as pgc
import pose_graph_model as pgm

POSE_BOUND = 4 * 8.9e-6
COST_BOUND = 4 * 8.4e-5
COST_FLOOR = 1e-6
# The preconditioned system is the identity plus rank <= 6 L, so exact arithmetic ends in 6 L + 1 iterations.  In doubles, with
# cg_tol = 1e-8, the largest excess measured over the cases was 6 iterations; the slack allowed is twice that.
CG_SLACK = 12
# A loop edge alone with a consistent chain: optimal cost against e' (Omega^-1 + J H_chain^-1 J')^-1 e, the Mahalanobis distance of the
# edge's residual under the chain's accumulated covariance.  The two differ by the linearisation; on chains of 8 - 32 nodes with
# odometry noise of 2 mm / 0.5 mrad the largest relative difference measured was 3.5e-5.  Bound: four times that.
MAHALANOBIS_BOUND = 4 * 3.5e-5

CASES = {c.name: c for c in pgc.cases()}
EDGE_CASES = {c.name: c for c in pgc.edge_cases()}
assert not set(CASES) & set(EDGE_CASES)
assert set(EDGE_CASES) == {"n48_l1024_hub", "n600_l513", "n64_l97", "n64_pi_headings", "n64_lambda0_zero", "n64_lambda_down_one", "n64_max_cg_one",
                           "n64_cg_tol_zero"}
CASES.update(EDGE_CASES)
MODEL_SECONDS_LIMIT = 60.0                  # test_large_case_model_is_quick_enough_to_keep's own; no edge case may take longer
_results, _seconds = {}, {}


def _solve(name):
    if name not in _results:
        c = CASES[name]
        t = time.time()
        _results[name] = pgm.solve(c.graph, c.params)
        _seconds[name] = time.time() - t
    return _results[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_reaches_its_path_and_agrees_with_the_dense_solve(name):
    c = CASES[name]
    r = _solve(name)
    assert c.condition(r), (name, c.why, r.tries, r.accepted, r.status)
    if name in EDGE_CASES:
        print(name, "model seconds %.2f" % _seconds[name], "tries", r.tries, "accepted", r.accepted, "status", r.status, "iterations", r.cg_iterations,
              "longest node list", int(r.node_lists.max()))
        assert _seconds[name] < MODEL_SECONDS_LIMIT
    # the slack was measured with a tolerance: with cg_tol = 0 the iteration goes on to an exact zero, far past the rank
    assert max(r.cg_per_try) <= 6 * c.graph.L + 1 + CG_SLACK or c.params.max_cg < 6 * c.graph.L + 1 or c.params.cg_tol == 0.0
    assert np.all(np.abs(r.poses[:, 2]) <= math.pi) and np.array_equal(r.poses[c.params.fixed], c.graph.nodes[c.params.fixed])
    if (r.status & 15) == pgm.OUT_OF_TRIES or (r.status & pgm.CG_CAP):
        return                                           # not at the optimum by construction: nothing to compare with
    x, F, tries, accepted = pgm.dense_solve(c.graph, c.params)
    dp = float(np.abs(x - r.poses).max())
    dc = abs(F - r.cost_after) / max(F, COST_FLOOR)
    print(name, "pose difference %.3g" % dp, "relative cost difference %.3g" % dc, "model tries", r.tries, "dense tries", tries)
    assert dp <= POSE_BOUND and dc <= COST_BOUND


def _chain_from_nodes(g, info=(1e4, 0.0, 1e4, 0.0, 0.0, 2.5e5)):
    z = pgm.relative_pose(g.nodes[:-1], g.nodes[1:])
    zi = np.tile(np.asarray(info, float), (g.N - 1, 1))
    return pgm.Graph(g.nodes, g.i, g.j, np.concatenate([z, g.z[g.N - 1:]]), np.concatenate([zi, g.info[g.N - 1:]]))


@pytest.mark.parametrize("name", ["n2_chain_only", "n64_l0", "n64_across_pi", "n257_l33"])
def test_chain_from_nodes_with_no_loop_edge_costs_exactly_nothing(name):
    g = _chain_from_nodes(CASES[name].graph)
    r = pgm.solve(g, pgm.DEFAULT, np.zeros(max((g.L + 31) // 32, 1), np.uint32))
    assert r.cost_before == 0.0 and r.cost_after == 0.0 and r.accepted == 0 and (r.status & 15) == pgm.CONVERGED_STEP
    assert r.poses.tobytes() == g.nodes.tobytes()
    assert np.all(r.chi2_before[:g.N - 1] == 0.0)


def test_a_zero_information_loop_edge_gives_the_bits_of_the_graph_without_it():
    c = CASES["n64_zero_info"]
    g = c.graph
    keep = np.ones(g.E, bool)
    keep[64] = False
    without = pgm.Graph(g.nodes, g.i[keep], g.j[keep], g.z[keep], g.info[keep])
    a, b = pgm.solve(g, c.params), pgm.solve(without, c.params)
    assert a.poses.tobytes() == b.poses.tobytes() and a.cost_after == b.cost_after and a.cost_before == b.cost_before
    assert (a.tries, a.accepted, a.cg_iterations, a.status, a.final_lambda) == (b.tries, b.accepted, b.cg_iterations, b.status, b.final_lambda)
    # and so does masking it out
    m = pgm.solve(g, c.params, np.array([0b101], np.uint32))
    assert m.poses.tobytes() == a.poses.tobytes() and m.cost_after == a.cost_after


def _mahalanobis(g, fixed=0):
    N, e = g.N, g.N - 1
    on = np.ones(g.E, bool)
    on[N - 1:] = False
    Hc, _, _ = pgm._dense_build(g, g.nodes, on, fixed)
    keep = np.ones(3 * N, bool)
    keep[3 * fixed:3 * fixed + 3] = False
    Hc = Hc[np.ix_(keep, keep)]
    i, j = int(g.i[e]), int(g.j[e])
    x = g.nodes
    c, s = math.cos(float(np.float32(x[i, 2]))), math.sin(float(np.float32(x[i, 2])))
    dx, dy = x[j, 0] - x[i, 0], x[j, 1] - x[i, 1]
    d = (x[j, 2] - x[i, 2] - g.z[e, 2] + math.pi) % (2 * math.pi) - math.pi
    r = np.array([c * dx + s * dy - g.z[e, 0], -s * dx + c * dy - g.z[e, 1], d])
    J = np.zeros((3, 3 * N))
    J[:, 3 * i:3 * i + 3] = [[-c, -s, -s * dx + c * dy], [s, -c, -c * dx - s * dy], [0, 0, -1.0]]
    J[:, 3 * j:3 * j + 3] = [[c, s, 0], [-s, c, 0], [0, 0, 1.0]]
    J = J[:, keep]
    S = J @ np.linalg.solve(Hc, J.T) + np.linalg.inv(pgm.full(g.info[e]))
    return float(r @ np.linalg.solve(S, r))


@pytest.mark.parametrize("n", [8, 16, 32])
def test_alone_cost_of_a_loop_edge_is_its_mahalanobis_distance(n):
    worst = 0.0
    for seed in range(8):
        g0, _ = pgc.loop_graph(n, 1, seed=100 + seed, drift=0.0005, odo_sigma=(0.002, 0.002, None))
        g = _chain_from_nodes(g0, g0.info[0])
        r = pgm.solve(g, pgm.DEFAULT)
        m = _mahalanobis(g)
        assert r.cost_before > r.cost_after > 0.0
        worst = max(worst, abs(r.cost_after - m) / m)
    print("n", n, "largest relative difference %.3g" % worst)
    assert worst <= MAHALANOBIS_BOUND


def test_large_case_model_is_quick_enough_to_keep():
    c = pgc.large_case()
    t = time.time()
    r = pgm.solve(c.graph, c.params)
    took = time.time() - t
    print("n4096_l64 model seconds %.1f" % took, r.tries, r.accepted, r.cg_per_try)
    assert c.condition(r) and took < MODEL_SECONDS_LIMIT
