"""The pose-graph solver on the device (bl_posegraph_*, botlab_amd.PoseGraph) against tests/pose_graph_model.py, BIT FOR BIT: the poses
in double, their narrowing to floats with utime carried, the per-edge chi2, the costs, the counters and the status, on the graphs of
tests/pose_graph_cases.py (each asserted to reach its path in the model), over subsets and their order, through the device-to-device
transfers to and from a scan log, and with every refusal leaving the handle as it was."""
import ctypes as C
import functools

import numpy as np
import pytest

import botlab_amd as bl
import pose_graph_cases as pgc
import pose_graph_model as pgm
from botlab_amd import _capi

pytestmark = pytest.mark.gpu
BL_ERR_ARG, BL_ERR_STATE = 2, 4
CASES = {c.name: c for c in pgc.cases()}
EDGE_CASES = {c.name: c for c in pgc.edge_cases()}          # run by tests/test_gpu_pose_graph_edges.py, which shares _model


@functools.lru_cache(maxsize=None)
def _model(name, mask_key=None):
    c = CASES[name] if name in CASES else EDGE_CASES[name] if name in EDGE_CASES else pgc.large_case()
    mask = None if mask_key is None else np.array(mask_key, np.uint32)
    return pgm.solve(c.graph, c.params, mask)


def _nodes(g, utime0=1000):
    p = np.zeros(g.N, bl.POSE_DTYPE)
    p["utime"] = utime0 + 7 * np.arange(g.N)
    p["x"], p["y"], p["theta"] = g.nodes[:, 0], g.nodes[:, 1], g.nodes[:, 2]
    assert np.array_equal(p["x"].astype(np.float64), g.nodes[:, 0])         # the cases' nodes are float values
    return p


def _params(p):
    return bl.posegraph_params(**p._asdict())


def _load(pg, g):
    pg.set_nodes(_nodes(g))
    e = bl.posegraph_edges(g.i, g.j, g.z, g.info)
    pg.set_chain(e[:g.N - 1])
    pg.set_loops(e[g.N - 1:])


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if np.asarray(a).dtype == np.float64 else np.uint32)


def _assert_equals_model(pg, g, subset, want, label):
    r = pg.results()[subset]
    p32, p64 = pg.poses(subset, want_double=True)
    before, after = pg.edge_chi2(subset)
    print(label, "device", r, "model", want.cost_before, want.cost_after, want.tries, want.accepted, want.cg_iterations, want.status)
    assert (r["tries"], r["accepted"], r["cg_iterations"], r["status"]) == (want.tries, want.accepted, want.cg_iterations, want.status), label
    for name, got, exp in (("cost_before", r["cost_before"], want.cost_before), ("cost_after", r["cost_after"], want.cost_after),
                           ("final_lambda", r["final_lambda"], want.final_lambda)):
        assert np.float64(got).view(np.uint64) == np.float64(exp).view(np.uint64), (label, name, got, exp)
    assert np.array_equal(_bits(p64), _bits(want.poses)), (label, np.abs(p64 - want.poses).max())
    assert np.array_equal(_bits(before), _bits(want.chi2_before)) and np.array_equal(_bits(after), _bits(want.chi2_after)), label
    nodes = _nodes(g)
    assert np.array_equal(p32["utime"], nodes["utime"])
    for k, f in enumerate(("x", "y", "theta")):
        assert np.array_equal(_bits(p32[f]), _bits(want.poses32[:, k])), (label, f)


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_equals_model(gpu_ctx, name):
    c = CASES[name]
    want = _model(name)
    assert c.condition(want), (name, c.why)
    pg = bl.PoseGraph(c.graph.N, max(c.graph.L, 1), 1, ctx=gpu_ctx)
    try:
        _load(pg, c.graph)
        pg.solve(_params(c.params))
        _assert_equals_model(pg, c.graph, 0, want, name)
    finally:
        pg.close()


@pytest.mark.parametrize("name,n_subsets", [("n100_l32", 1), ("n100_l32", 2), ("n257_l33", 65), ("n64_repeated_pair", 5)])
def test_subsets_equal_the_model_alone_in_either_order(gpu_ctx, name, n_subsets):
    c = CASES[name]
    g = c.graph
    masks = pgc.subset_masks(g.L, n_subsets, seed=3)
    pg = bl.PoseGraph(g.N, g.L, n_subsets, ctx=gpu_ctx)
    try:
        _load(pg, g)
        for order in (np.arange(n_subsets), np.arange(n_subsets)[::-1]):
            pg.solve(_params(c.params), masks[order])
            for s in (range(n_subsets) if n_subsets <= 5 else (0, 1, 2, 33, 34, 35, 64)):
                m = masks[order[s]]
                want = _model(name, tuple(int(v) for v in m))
                _assert_equals_model(pg, g, s, want, "%s subset %d (mask %d)" % (name, s, order[s]))
                if not m.any():                                         # the all-zero mask: the chain alone
                    assert want.cost_after <= want.cost_before
    finally:
        pg.close()


def test_all_zero_mask_on_a_consistent_chain_returns_the_poses(gpu_ctx):
    g = CASES["n65_l4"].graph
    pg = bl.PoseGraph(g.N, g.L, 2, ctx=gpu_ctx)
    try:
        nodes = _nodes(g)
        pg.set_nodes(nodes)
        pg.set_chain_from_nodes(np.array([1e4, 0, 1e4, 0, 0, 2.5e5]))
        pg.set_loops(bl.posegraph_edges(g.i, g.j, g.z, g.info)[g.N - 1:])
        pg.solve(masks=np.array([[0], [0xffffffff]], np.uint32))
        r = pg.results()
        p32, p64 = pg.poses(0, want_double=True)
        assert r[0]["cost_before"] == 0.0 and r[0]["cost_after"] == 0.0 and r[0]["accepted"] == 0 and r[0]["status"] == bl.POSEGRAPH_CONVERGED_STEP
        assert np.array_equal(_bits(p64), _bits(g.nodes)) and p32.tobytes() == nodes.tobytes()
        # the chain made on the device is the model's relative poses, and the other subset is the model's solve of that graph
        z = pgm.relative_pose(g.nodes[:-1], g.nodes[1:])
        zi = np.tile(np.array([1e4, 0, 1e4, 0, 0, 2.5e5]), (g.N - 1, 1))
        g2 = pgm.Graph(g.nodes, g.i, g.j, np.concatenate([z, g.z[g.N - 1:]]), np.concatenate([zi, g.info[g.N - 1:]]))
        want = pgm.solve(g2, pgm.DEFAULT, np.array([0xffffffff], np.uint32))
        assert want.accepted >= 1
        _assert_equals_model(pg, g2, 1, want, "chain from nodes")
    finally:
        pg.close()


def test_large_graph(gpu_ctx):
    """N = 4096, L = 64: the model takes about 4 s on one core."""
    c = pgc.large_case()
    want = _model(c.name)
    assert c.condition(want)
    pg = bl.PoseGraph(4096, 64, 1, ctx=gpu_ctx)
    try:
        _load(pg, c.graph)
        pg.solve(_params(c.params))
        _assert_equals_model(pg, c.graph, 0, want, c.name)
        print("n4096_l64 device ms", pg.lastDeviceMs())
    finally:
        pg.close()


def _scan(n=8):
    return bl.LidarScan(np.full(n, 1.0, np.float32), np.linspace(0, 6.0, n).astype(np.float32), np.arange(n, dtype=np.int64) + 5, utime=20)


def test_transfers_to_and_from_a_scan_log(gpu_ctx):
    g = CASES["n5_l1"].graph
    nodes = _nodes(g)
    log = bl.ScanHistory(7, 16, ctx=gpu_ctx)
    # a ring that has wrapped: 9 appends into 7 slots, the 5 nodes are entries 1 .. 5
    junk = bl.make_pose(9.0, 9.0, 0.5, utime=3)
    for k in range(3):
        log.append(_scan(), junk)
    for k in range(5):
        log.append(_scan(), bl.make_pose(float(nodes["x"][k]), float(nodes["y"][k]), float(nodes["theta"][k]), utime=int(nodes["utime"][k])))
    log.append(_scan(), junk)
    assert len(log) == 7
    a, b = bl.PoseGraph(8, 4, 1, ctx=gpu_ctx), bl.PoseGraph(8, 4, 1, ctx=gpu_ctx)
    try:
        e = bl.posegraph_edges(g.i, g.j, g.z, g.info)
        a.set_nodes(nodes)
        b.set_nodes_from_log(log, 1, 5)
        for pg in (a, b):
            pg.set_chain(e[:4]); pg.set_loops(e[4:]); pg.solve(_params(CASES["n5_l1"].params))
        want = _model("n5_l1")
        _assert_equals_model(a, g, 0, want, "uploaded")
        _assert_equals_model(b, g, 0, want, "from the log")
        b.poses_to_log(log, 0, 1)
        got = log.poses()
        assert got[1:6].tobytes() == a.poses(0).tobytes()
        assert got[0]["x"] == 9.0 and got[6]["x"] == 9.0
        other = bl.ScanHistory(7, 16, ctx=gpu_ctx)
        for k in range(7):
            other.append(_scan(), junk)
        other.set_poses(1, a.poses(0))
        assert other.poses().tobytes() == got.tobytes()
        other.close()
    finally:
        a.close(); b.close(); log.close()


def test_refusals_change_nothing(gpu_ctx):
    c = CASES["n9_l2"]
    g = c.graph
    lib = gpu_ctx.lib
    pg = bl.PoseGraph(16, 4, 2, ctx=gpu_ctx)
    log = bl.ScanHistory(4, 16, ctx=gpu_ctx)
    try:
        h = C.c_void_p()
        for args in ((1, 0, 1), (4097, 0, 1), (8, -1, 1), (8, 1025, 1), (8, 0, 0), (4096, 1024, 400)):
            assert lib.bl_posegraph_create(gpu_ctx.h, *args, C.byref(h)) == BL_ERR_ARG, args
        prm = _params(c.params)
        e = bl.posegraph_edges(g.i, g.j, g.z, g.info)
        assert lib.bl_posegraph_set_chain(pg.h, e.ctypes.data) == BL_ERR_STATE
        assert lib.bl_posegraph_solve(pg.h, C.byref(prm), 1, None) == BL_ERR_STATE
        res = np.zeros(2, bl.POSEGRAPH_RESULT_DTYPE)
        assert lib.bl_posegraph_results(pg.h, res.ctypes.data) == BL_ERR_STATE
        pg.set_nodes(_nodes(g))
        assert lib.bl_posegraph_solve(pg.h, C.byref(prm), 1, None) == BL_ERR_STATE        # no chain yet
        pg.set_chain(e[:8]); pg.set_loops(e[8:])
        pg.solve(prm)
        want = _model("n9_l2")
        _assert_equals_model(pg, g, 0, want, "before the refusals")

        def refused(rc, code=BL_ERR_ARG):
            assert rc == code
        nodes = _nodes(g)
        refused(lib.bl_posegraph_set_nodes(pg.h, 1, nodes.ctypes.data))
        refused(lib.bl_posegraph_set_nodes(pg.h, 17, nodes.ctypes.data))
        refused(lib.bl_posegraph_set_nodes_from_log(pg.h, log.h, 0, 2))                   # an empty log
        bad = e[:8].copy(); bad["j"][3] = 5
        refused(lib.bl_posegraph_set_chain(pg.h, bad.ctypes.data))
        bad = e[:8].copy(); bad["info"][2, 1] = np.nan
        refused(lib.bl_posegraph_set_chain(pg.h, bad.ctypes.data))
        for i, j in ((2, 2), (-1, 3), (3, 9)):
            bad = e[8:].copy(); bad["i"][1], bad["j"][1] = i, j
            refused(lib.bl_posegraph_set_loops(pg.h, 2, bad.ctypes.data))
        refused(lib.bl_posegraph_set_loops(pg.h, 5, e.ctypes.data))
        m = np.full(4, 0xffffffff, np.uint32)
        for kw in (dict(fixed=9), dict(fixed=-1), dict(max_tries=0), dict(max_cg=0), dict(lambda0=-1.0), dict(lambda_up=1.0), dict(lambda_down=0.0),
                   dict(lambda_down=1.5), dict(step_tol=-1.0), dict(rel_tol=float("nan")), dict(cg_tol=float("inf"))):
            bp = _params(c.params._replace(**kw))
            refused(lib.bl_posegraph_solve(pg.h, C.byref(bp), 1, m.ctypes.data))
        refused(lib.bl_posegraph_solve(pg.h, C.byref(prm), 3, m.ctypes.data))
        refused(lib.bl_posegraph_solve(pg.h, C.byref(prm), 0, m.ctypes.data))
        refused(lib.bl_posegraph_solve(pg.h, C.byref(prm), 2, None))
        out = np.zeros(g.N, bl.POSE_DTYPE)
        refused(lib.bl_posegraph_poses(pg.h, 1, out.ctypes.data, None))                   # the last solve had one subset
        refused(lib.bl_posegraph_poses_to_log(pg.h, 0, log.h, 0))                         # no room in the log
        # nodes, edges and the last results are as they were
        _assert_equals_model(pg, g, 0, want, "after the refusals")
        pg.solve(prm)
        _assert_equals_model(pg, g, 0, want, "solved again after the refusals")
    finally:
        pg.close(); log.close()
