"""The pose-graph solver on the device at the limits tests/test_gpu_pose_graph.py does not reach (pose_graph_cases.edge_cases; DESIGN.md
4.32), BIT FOR BIT against tests/pose_graph_model.py as there: 1024 loop edges with a node list of more than 512 entries, 513 loop
edges on 600 nodes, four mask words, masks of 32 words with single bits in the high words, float headings of +-pi, the accepted
parameter values at the ends of their ranges, and one handle larger than its graphs that solves a large graph, a small one and the
large one again with three subsets each."""
import numpy as np
import pytest

import botlab_amd as bl
import pose_graph_cases as pgc
import pose_graph_model as pgm
from test_gpu_pose_graph import CASES as BASE_CASES
from test_gpu_pose_graph import EDGE_CASES, _assert_equals_model, _load, _model, _params

pytestmark = pytest.mark.gpu


def _key(mask):
    return tuple(int(v) for v in mask)


def _bit(words, l):
    m = np.zeros(words, np.uint32)
    m[l >> 5] = np.uint32(1) << np.uint32(l & 31)
    return m


@pytest.mark.parametrize("name", sorted(EDGE_CASES))
def test_device_equals_model(gpu_ctx, name):
    c = EDGE_CASES[name]
    want = _model(name)
    assert c.condition(want), (name, c.why)
    pg = bl.PoseGraph(c.graph.N, max(c.graph.L, 1), 1, ctx=gpu_ctx)
    try:
        _load(pg, c.graph)
        pg.solve(_params(c.params))
        _assert_equals_model(pg, c.graph, 0, want, name)
        print(name, "device ms", pg.lastDeviceMs())
    finally:
        pg.close()


def _hub_masks():
    rng = np.random.default_rng(1024)
    m = np.zeros((7, 32), np.uint32)
    m[0] = 0xffffffff
    m[2] = _bit(32, 1023)
    m[3] = _bit(32, 512)
    m[4, 16] = 0xffffffff
    m[5] = _bit(32, 0)
    m[6] = rng.integers(0, 1 << 32, 32, dtype=np.uint64).astype(np.uint32)
    return m


def _subsets_in_both_orders(gpu_ctx, name, masks):
    c = EDGE_CASES[name]
    g = c.graph
    n = len(masks)
    assert masks.shape == (n, (g.L + 31) // 32)
    pg = bl.PoseGraph(g.N, g.L, n, ctx=gpu_ctx)
    try:
        _load(pg, g)
        for order in (np.arange(n), np.arange(n)[::-1]):
            pg.solve(_params(c.params), masks[order])
            print(name, n, "subsets, device ms", pg.lastDeviceMs())
            for s in range(n):
                want = _model(name, _key(masks[order[s]]))
                _assert_equals_model(pg, g, s, want, "%s subset %d (mask %d)" % (name, s, order[s]))
    finally:
        pg.close()


def test_hub_subsets_over_32_mask_words(gpu_ctx):
    """all on, all off, bit 1023, bit 512, word 16, bit 0, a random mask: each equals the model alone, in either order"""
    masks = _hub_masks()
    g = EDGE_CASES["n48_l1024_hub"].graph
    # the single bits pick the edges they name, and no two masks solve the same graph
    for s, l in ((2, 1023), (3, 512), (5, 0)):
        on = pgm.in_force(g, masks[s])
        assert on[g.N - 1 + l] and on[g.N - 1:].sum() == 1
    assert pgm.in_force(g, masks[4])[g.N - 1:].nonzero()[0].tolist() == list(range(512, 544))
    assert len({_model("n48_l1024_hub", _key(m)).cost_after for m in masks}) == 7
    _subsets_in_both_orders(gpu_ctx, "n48_l1024_hub", masks)


def test_single_bits_at_the_word_borders(gpu_ctx):
    """L = 97: bits 31, 32, 95 and 96 alone, and all on"""
    masks = np.stack([_bit(4, 31), _bit(4, 32), _bit(4, 95), _bit(4, 96), np.full(4, 0xffffffff, np.uint32)])
    assert len({_model("n64_l97", _key(m)).cost_after for m in masks}) == 5
    _subsets_in_both_orders(gpu_ctx, "n64_l97", masks)


def test_a_handle_larger_than_its_graphs_is_reused(gpu_ctx):
    """PoseGraph(300, 70, 3): n257_l33, then n64_l1, then n257_l33 again, three masks each.  max_nodes > N with several subsets: the loop
    edges sit at max_nodes - 1, a subset's poses at subset * max_nodes, its workspace at subset times the stride of the maxima; and the
    workspace is never cleared, so the small solve runs on what the large one left and the large one on what the small one left."""
    pg = bl.PoseGraph(300, 70, 3, ctx=gpu_ctx)
    try:
        for name in ("n257_l33", "n64_l1", "n257_l33"):
            c = BASE_CASES[name]
            g = c.graph
            assert g.N < 300 and g.L < 70
            masks = pgc.subset_masks(g.L, 3, seed=5)
            masks[2] = np.random.default_rng(g.N).integers(0, 1 << 32, masks.shape[1], dtype=np.uint64).astype(np.uint32)
            assert masks[0].all() and not masks[1].any()
            _load(pg, g)
            pg.solve(_params(c.params), masks)
            for s in range(3):
                want = _model(name, _key(masks[s]))
                _assert_equals_model(pg, g, s, want, "%s on the larger handle, subset %d" % (name, s))
            assert _model(name, _key(masks[0])).accepted >= 1
    finally:
        pg.close()
