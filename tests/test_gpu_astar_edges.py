"""search_for_path at the edges no fixture map reaches (tests/astar_edge_cases.py; what each input reaches is asserted on the CPU by
tests/test_astar_edge_cases_cpu.py): pushes refused by the fCost < INT16_MAX rule and keys up to 65 532 beside k_astar2's 0xFFFF
sentinel, open lists that drain to empty from the deep regime, from the LDS regime and from a few entries, lists of ONE entry for
thousands of iterations, pops of border and corner cells, the same on grids of more than 524 288 cells (the forms that ask for cell
lines two steps ahead), the early exits, and the capacity outcome.  Every case: stats == the oracle's, pose bytes equal, the distance
grid bit-equal first; in the default form in this process and once each in a child process per switch (the switches are read once
per process); the batch form against the single searches; the capacity count against the model in every form.

No case is dropped from any form: the slowest child takes a few seconds."""
import ctypes as C
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import astar_edge_cases as ec
import helpers

pytestmark = pytest.mark.gpu

GROUPS = {"corridors": ec.CORRIDOR_CASES, "twins": ec.TWIN_CASES, "exits_and_rings": None}
CAPACITY_CASE = "h15_centre_d3270"                       # its list reaches 19 740 entries
CAPACITY = 16384                                         # the least the host allows: the capacity falls where the list leaves the LDS tier
POSE_DTYPE = [("utime", "<i8"), ("x", "<f4"), ("y", "<f4"), ("theta", "<f4")]


def _group(name):
    return GROUPS[name] if GROUPS[name] is not None else ec.EARLY_EXIT_CASES + [ec.RING_CHECKED] + ec.ring_cases()


def _expected(oracle, cases):
    """what the children need of the oracle's results: plain data, the distance grid once per world"""
    out = dict(cases=[], dist={})
    for c in cases:
        r = ec.reference(oracle, c)
        assert r["stats"][0] <= ec.MAX_POPS
        out["dist"][c.world] = r["dist"]
        out["cases"].append(dict(name=c.name, world=c.world, start=c.start, goal=c.goal, params=c.params, stats=r["stats"], path=r["path"].tobytes()))
    return out


def _run(bl, ctx, expected, want_kernel):
    """Every case of expected on ctx.  Returns (names that passed, None or the first failure): a failure ends the list."""
    passed = []
    grids = {}
    for e in expected["cases"]:
        if e["world"] not in grids:
            w = ec.world(e["world"])
            g = bl.OccupancyGrid.from_cells(w.cells, w.origin, ec.MPC, cellsPerMeter=helpers.CPM_DEFAULT, ctx=ctx)
            d = bl.ObstacleDistanceGrid(ctx=ctx)
            d.setDistances(g)
            if not np.array_equal(d.cells().view(np.uint32), expected["dist"][e["world"]].view(np.uint32)):
                return passed, "%s: the distance grid differs from the oracle's" % (e["world"],)
            grids[e["world"]] = (g, d)
        d = grids[e["world"]][1]
        sp = bl._capi.SearchParams(*e["params"])
        path, stats = bl.search_for_path(bl.make_pose(*e["start"], 0.3), bl.make_pose(*e["goal"], 0.0), d, sp, return_stats=True, cap=4096)
        kernel = ctx.lib.bl_astar_debug_last_kernel(ctx.h)
        got = np.array([(p.utime, p.x, p.y, p.theta) for p in path], dtype=POSE_DTYPE).tobytes()
        if kernel != want_kernel:
            return passed, "%s: kernel %d ran, not %d" % (e["name"], kernel, want_kernel)
        if tuple(stats) != tuple(e["stats"]):
            return passed, "%s: (pops, pushes) %s, the oracle's %s" % (e["name"], tuple(stats), tuple(e["stats"]))
        if got != e["path"]:
            return passed, "%s: %d poses differ from the oracle's %d" % (e["name"], len(path), len(e["path"]) // 24)
        passed.append(e["name"])
    return passed, None


def _capacity_run(bl, expected):
    """the capacity case on a context of its own with a 16 384-entry list: (return code, poses, first pose == start, (pops, pushes)), twice"""
    e = next(x for x in expected["cases"] if x["name"] == CAPACITY_CASE)
    ctx = bl.Context(0)
    try:
        w = ec.world(e["world"])
        g = bl.OccupancyGrid.from_cells(w.cells, w.origin, ec.MPC, cellsPerMeter=helpers.CPM_DEFAULT, ctx=ctx)
        d = bl.ObstacleDistanceGrid(ctx=ctx)
        d.setDistances(g)
        assert ctx.lib.bl_astar_set_open_capacity(ctx.h, CAPACITY) == 0
        s, gl, sp = bl.make_pose(*e["start"], 0.3), bl.make_pose(*e["goal"], 0.0), bl._capi.SearchParams(*e["params"])
        seen = []
        for _ in range(2):
            buf = (bl._capi.Pose * 64)(); n = C.c_int(0); stats = (C.c_int64 * 2)()
            rc = ctx.lib.bl_astar_search(ctx.h, d.h, C.byref(s), C.byref(gl), C.byref(sp), buf, 64, C.byref(n), stats)
            seen.append([int(rc), int(n.value), bool((buf[0].x, buf[0].y) == (s.x, s.y)), [int(stats[0]), int(stats[1])],
                         int(ctx.lib.bl_astar_debug_last_kernel(ctx.h))])
        return seen
    finally:
        ctx.close()


def _check_capacity(bl, seen, want, want_kernel):
    for rc, n, first_is_start, stats, kernel in seen:
        assert rc == bl._capi.BL_ERR_CAPACITY and n == 1 and first_is_start and kernel == want_kernel, seen
        assert tuple(stats) == tuple(want), (stats, want)


def _capacity_want(oracle):
    case = next(c for c in ec.CORRIDOR_CASES if c.name == CAPACITY_CASE)
    r = ec.reference(oracle, case)
    m = ec.model(r["dist"], ec.world(case.world).origin, case.start, case.goal, case.params, cap=CAPACITY)
    assert m["capacity_at"] is not None and m["capacity_at"][1] + 1 - m["capacity_at"][0] == CAPACITY
    return m["capacity_at"]


# ---------------------------------------------------------------------------------------------------------------- the default form
@pytest.mark.parametrize("group", list(GROUPS))
def test_astar_edge_cases_equal_oracle(oracle, gpu_ctx, group):
    import botlab_amd as bl
    cases = _group(group)
    passed, failure = _run(bl, gpu_ctx, _expected(oracle, cases), 2)
    assert failure is None, failure
    assert passed == [c.name for c in cases]


def test_astar_capacity_count_is_k_astars(oracle):
    """BL_ERR_CAPACITY with the 1-pose path, at the count of k_astar's C++ loop: the pop of the refusing iteration counted, the refused
    push not (the model's cap=16384 result) -- the same on every run"""
    import botlab_amd as bl
    case = next(c for c in ec.CORRIDOR_CASES if c.name == CAPACITY_CASE)
    _check_capacity(bl, _capacity_run(bl, _expected(oracle, [case])), _capacity_want(oracle), 2)


def test_astar_batch_equals_single_searches(oracle, gpu_ctx):
    """search_for_path_batch from one start on the H 15 corridor with an 8-cell tooth at column 40: goals that are found without a
    refused push (D 3262), found with 13 094 refused (D 3270), drained after 24 952 and after 335 pops (D 3271, 3273) and cut at the
    first expansion (D 3277).  Each result equals the single search's and the oracle's."""
    import botlab_amd as bl
    cases = [ec._corridor_case("batch_d%d" % D, 15, "wall", 40, 8, D, None, None) for D in (3262, 3270, 3271, 3273, 3277)]
    refs = [ec.reference(oracle, c) for c in cases]
    assert [len(r["path"]) > 1 for r in refs] == [True, True, False, False, False]
    assert refs[2]["stats"] == (24952, 24951) and refs[3]["stats"] == (335, 334) and refs[4]["stats"] == (1, 0)
    w = ec.world(cases[0].world)
    g = bl.OccupancyGrid.from_cells(w.cells, w.origin, ec.MPC, cellsPerMeter=helpers.CPM_DEFAULT, ctx=gpu_ctx)
    d = bl.ObstacleDistanceGrid(ctx=gpu_ctx)
    d.setDistances(g)
    assert np.array_equal(d.cells().view(np.uint32), refs[0]["dist"].view(np.uint32))
    sp = bl._capi.SearchParams(*ec.FLAT)
    start = bl.make_pose(*cases[0].start, 0.3)
    goals = [bl.make_pose(*c.goal, 0.0) for c in cases]
    paths, stats = bl.search_for_path_batch(start, goals, d, sp, return_stats=True)
    for c, r, path, st, goal in zip(cases, refs, paths, stats, goals):
        single, sst = bl.search_for_path(start, goal, d, sp, return_stats=True, cap=4096)
        as_bytes = lambda ps: np.array([(p.utime, p.x, p.y, p.theta) for p in ps], dtype=POSE_DTYPE).tobytes()
        assert tuple(st) == tuple(sst) == r["stats"], (c.name, st, sst, r["stats"])
        assert as_bytes(path) == as_bytes(single) == r["path"].tobytes(), c.name


# ---------------------------------------------------------------------------------------------------------------- the other forms
def _edges_in_child(in_path, out_path, want_kernel):
    import json
    import botlab_amd as bl
    expected = pickle.load(open(in_path, "rb"))
    out = dict(passed=[], failure=None, capacity=None)
    json.dump(out, open(out_path, "w"))
    out["passed"], out["failure"] = _run(bl, bl.default_context(), expected, want_kernel)
    if out["failure"] is None:
        out["capacity"] = _capacity_run(bl, expected)
    json.dump(out, open(out_path, "w"))


_child_died = []


@pytest.mark.parametrize("env", ["BOTLAB_ASTAR_NO_TURBO", "BOTLAB_ASTAR_V1", "BOTLAB_ASTAR_DUO=0", "BOTLAB_ASTAR_SMALL_LDS=1",
                                 "BOTLAB_ASTAR_SMALL_LDS=3"])
def test_astar_edge_cases_in_the_other_forms_of_the_search(oracle, tmp_path, env):
    """every case, and the capacity count, through k_astar2's C++ iteration alone, through k_astar, through the one-wave straight-line
    loops, and with the 40 KB footprint on one wave and on three (there the drained and the cut lists cross into the deep regime from
    4 095 entries on).  k_astar2 must have run in every form but BOTLAB_ASTAR_V1, k_astar there."""
    import json
    import botlab_amd as bl
    assert not _child_died, "an earlier child process ended abnormally: %s" % _child_died
    cases = ec.CORRIDOR_CASES + ec.TWIN_CASES + _group("exits_and_rings")
    want_kernel = 1 if env == "BOTLAB_ASTAR_V1" else 2
    inp, out = str(tmp_path / "expected.pickle"), str(tmp_path / "res.json")
    pickle.dump(_expected(oracle, cases), open(inp, "wb"))
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_astar_edges as t; t._edges_in_child(%r, %r, %d)"
            % (here, os.path.dirname(here), inp, out, want_kernel))
    e = dict(os.environ)
    k, _, v = env.partition("=")
    e[k] = v or "1"
    rc = subprocess.call([sys.executable, "-c", code], env=e)
    if rc != 0:
        _child_died.append((env, rc))
    res = json.load(open(out)) if os.path.exists(out) else None
    assert rc == 0, (env, rc, res)
    assert res["failure"] is None, (env, res["failure"], len(res["passed"]))
    assert res["passed"] == [c.name for c in cases]
    _check_capacity(bl, res["capacity"], _capacity_want(oracle), want_kernel)
