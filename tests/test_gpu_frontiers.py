"""Row f3: find_map_frontiers, the batched search_for_path and plan_path_to_frontier on the GPU
against the oracle's restatement of src/planning/frontiers.cpp / motion_planner.cpp.  Everything here is integer / index
work or float arithmetic restated operation by operation, so the bar is bit-exact: same frontiers in the same order,
same cells in the same order, same goal, same path."""
import ctypes as C

import numpy as np
import pytest

import botlab_amd as bl
import helpers
import oracle_lib

pytestmark = pytest.mark.gpu


def _blob_map(seed, shape=(200, 200)):
    """Random partially explored map: free blobs (strongly negative), weak values -7..1 along their rim (exercises the
    [-5, 0] frontier test), occupied blobs, unknown (0) elsewhere."""
    from scipy.ndimage import gaussian_filter
    rng = np.random.default_rng(seed)
    f = gaussian_filter(rng.normal(size=shape), 4)
    g = gaussian_filter(rng.normal(size=shape), 3)
    c = np.zeros(shape, np.int8)
    c[f > 0.02] = -20
    rim = (f > 0.0) & (f <= 0.02)
    c[rim] = rng.integers(-7, 2, size=int(rim.sum()))
    c[g > 0.09] = 60
    return c


def _frame(shape):
    h, w = shape
    return (np.float32(-w * 0.05 / 2), np.float32(-h * 0.05 / 2)), np.float32(0.05)


def _sweep_kernel_is(fr, k):
    """which kernels grew the frontiers (bl_frontiers_debug_sweep_kernel) -- checked only when no switch forces another form"""
    import os
    if "BOTLAB_FRONTIER_GROW_V1" not in os.environ:
        assert fr.sweep_kernel() == k, (fr.sweep_kernel(), k)


def _same_frontiers(got, exp):
    assert len(got) == len(exp), (len(got), len(exp))
    for k, (a, b) in enumerate(zip(got, exp)):
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), f"frontier {k} differs"


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4, 5])
def test_find_map_frontiers_random_maps(oracle, gpu_ctx, seed):
    shape = (200, 200) if seed < 4 else (150, 333)
    cells = _blob_map(seed, shape)
    origin, mpc = _frame(shape)
    grid = bl.OccupancyGrid.from_cells(cells, origin, mpc, cellsPerMeter=helpers.CPM_DEFAULT, ctx=gpu_ctx)
    rng = np.random.default_rng(100 + seed)
    ys, xs = np.nonzero(cells < -5)
    robots = []
    for _ in range(3):                                     # robots in free space
        k = rng.integers(len(xs))
        robots.append((float(origin[0]) + (xs[k] + 0.5) * 0.05, float(origin[1]) + (ys[k] + 0.5) * 0.05))
    ys2, xs2 = np.nonzero((cells >= -5) & (cells <= 0))    # a robot standing on a frontier-valued / unknown cell
    k = rng.integers(len(xs2))
    robots.append((float(origin[0]) + (xs2[k] + 0.5) * 0.05, float(origin[1]) + (ys2[k] + 0.5) * 0.05))
    robots.append((float(origin[0]) - 0.02, float(origin[1]) + 2.0))        # just outside the grid, next to column 0
    robots.append((1000.0, 1000.0))                                          # far outside
    total = 0
    for (rx, ry) in robots:
        for min_len in (0.35, 0.1):
            exp = oracle.find_frontiers(cells, mpc, helpers.CPM_DEFAULT, origin, oracle.pose(rx, ry, 0.0), min_len)
            got = bl.find_map_frontiers(grid, bl.make_pose(rx, ry, 0.0), min_len).cells()
            _same_frontiers(got, exp)
            total += len(exp)
    assert total > 10


@pytest.mark.parametrize("seed,shape", [(11, (400, 420)), (12, (700, 333)), (13, (1000, 1000)), (14, (401, 419)), (15, (333, 1021))])      # (the last two: cell counts that are no multiple of 4 -- k_frontier_touches reads four class bytes at a time)
def test_find_map_frontiers_random_maps_beyond_lds(oracle, gpu_ctx, seed, shape):
    """Grids whose class bytes do not fit LDS take the multi-launch form: classification over the whole device, the flood by one
    workgroup, the touches collected by all workgroups, the frontiers grown by one wave with an LDS visited set.  Random blob maps
    have dozens to hundreds of small frontiers (the fallbacks of that form: the next test)."""
    cells = _blob_map(seed, shape)
    origin, mpc = _frame(shape)
    grid = bl.OccupancyGrid.from_cells(cells, origin, mpc, cellsPerMeter=helpers.CPM_DEFAULT, ctx=gpu_ctx)
    rng = np.random.default_rng(300 + seed)
    ys, xs = np.nonzero(cells < -5)
    total = 0
    for _ in range(3):
        k = rng.integers(len(xs))
        rx, ry = float(origin[0]) + (xs[k] + 0.5) * 0.05, float(origin[1]) + (ys[k] + 0.5) * 0.05
        exp = oracle.find_frontiers(cells, mpc, helpers.CPM_DEFAULT, origin, oracle.pose(rx, ry, 0.0), 0.1)
        fr = bl.find_map_frontiers(grid, bl.make_pose(rx, ry, 0.0), 0.1)
        _sweep_kernel_is(fr, 2)                            # a ninth of a blob map's cells are frontier-class: more than k_frontier_grow2's set holds
        _same_frontiers(fr.cells(), exp)
        total += len(exp)
    assert total > 3


@pytest.mark.parametrize("seed,shape", [(21, (320, 330)), (22, (330, 320)), (25, (310, 340))])
def test_find_map_frontiers_random_maps_just_beyond_lds_through_the_cell_set(oracle, gpu_ctx, seed, shape):
    """Random blob maps small enough for k_frontier_grow2's set (about 12 000 frontier-class cells, reachable or not; 16 384 fit) and
    too large for the one-workgroup form (96 K cells): dozens of small frontiers, blobs and rims of every shape, grown from the LDS
    set -- same lists as the oracle's."""
    cells = _blob_map(seed, shape)
    origin, mpc = _frame(shape)
    grid = bl.OccupancyGrid.from_cells(cells, origin, mpc, cellsPerMeter=helpers.CPM_DEFAULT, ctx=gpu_ctx)
    rng = np.random.default_rng(500 + seed)
    ys, xs = np.nonzero(cells < -5)
    total = 0
    for _ in range(6):
        k = rng.integers(len(xs))
        rx, ry = float(origin[0]) + (xs[k] + 0.5) * 0.05, float(origin[1]) + (ys[k] + 0.5) * 0.05
        for min_len in (0.1, 0.35):
            exp = oracle.find_frontiers(cells, mpc, helpers.CPM_DEFAULT, origin, oracle.pose(rx, ry, 0.0), min_len)
            fr = bl.find_map_frontiers(grid, bl.make_pose(rx, ry, 0.0), min_len)
            _sweep_kernel_is(fr, 3)
            _same_frontiers(fr.cells(), exp)
            total += len(exp)
    assert total > 10


@pytest.mark.parametrize("case", ["all_free", "all_unknown", "robot_outside", "robot_on_unknown", "robot_on_frontier_value", "walls_only"])
def test_find_map_frontiers_degenerate_maps_beyond_lds(oracle, gpu_ctx, case):
    """The multi-launch form on maps that have no frontier at all, no free space at all, or a robot that does not stand in free
    space (the flood then starts from a cell it may not enter): same lists (mostly empty) as the oracle's."""
    shape = (700, 1000)
    origin, mpc = _frame(shape)
    cells = np.zeros(shape, np.int8)
    rx, ry = 0.0, 0.0
    if case == "all_free":
        cells[:] = -60
    elif case == "walls_only":
        cells[:] = 80
    elif case == "robot_outside":
        cells[100:600, 100:900] = -60
        rx, ry = float(origin[0]) - 3.0, 0.0
    elif case == "robot_on_unknown":
        cells[100:600, 100:900] = -60
        rx, ry = float(origin[0]) + 50.5 * 0.05, float(origin[1]) + 350.5 * 0.05          # in the unknown margin, next to nothing
    elif case == "robot_on_frontier_value":
        cells[100:600, 100:900] = -60
        cells[350, 99] = -3                                                                  # a weak cell on the rim: class "frontier"
        rx, ry = float(origin[0]) + 99.5 * 0.05, float(origin[1]) + 350.5 * 0.05
    grid = bl.OccupancyGrid.from_cells(cells, origin, mpc, cellsPerMeter=helpers.CPM_DEFAULT, ctx=gpu_ctx)
    for min_len in (0.1, 0.35):
        exp = oracle.find_frontiers(cells, mpc, helpers.CPM_DEFAULT, origin, oracle.pose(rx, ry, 0.0), min_len)
        got = bl.find_map_frontiers(grid, bl.make_pose(rx, ry, 0.0), min_len).cells()
        _same_frontiers(got, exp)


@pytest.mark.parametrize("S,free", [(2600, 2400), (4400, 4200)])
def test_find_map_frontiers_one_frontier_larger_than_the_visited_set(oracle, gpu_ctx, S, free):
    """A free square in unknown space: ONE frontier of 4 x `free` cells.  2400: more cells than the grow kernel's LDS visited set
    holds (half of 16 384 slots) -- it undoes its marks and the one-workgroup sweep takes over.  4200: more touches (16 800) than
    the grow kernel keeps -- the one-workgroup sweep from the start.  Same list as the oracle's either way."""
    cells = np.zeros((S, S), np.int8)
    cells[100:100 + free, 100:100 + free] = -50
    origin, mpc = _frame((S, S))
    grid = bl.OccupancyGrid.from_cells(cells, origin, mpc, cellsPerMeter=helpers.CPM_DEFAULT, ctx=gpu_ctx)
    rx, ry = float(origin[0]) + 300.5 * 0.05, float(origin[1]) + 1200.5 * 0.05
    exp = oracle.find_frontiers(cells, mpc, helpers.CPM_DEFAULT, origin, oracle.pose(rx, ry, 0.0), 0.1)
    fr = bl.find_map_frontiers(grid, bl.make_pose(rx, ry, 0.0), 0.1)
    assert len(exp) == 1 and len(exp[0]) > 8192
    _sweep_kernel_is(fr, 3 if free == 2400 else 1)          # 9 600 cells fit k_frontier_grow2's set (k_frontier_grow's visited set they do not: the child runs below); 16 800 touches fit neither
    _same_frontiers(fr.cells(), exp)


def test_find_map_frontiers_more_frontier_cells_than_the_lds_set_holds(oracle, gpu_ctx):
    """k_frontier_grow2 keeps ALL frontier-class cells of the grid in one LDS set (16 384 at most).  Here 25 600: a reachable free
    square (one frontier of 8 000 cells) and 22 free squares the flood never reaches -- the sweep goes to k_frontier_grow (visited
    set only, classes from global memory).  Same list as the oracle's."""
    S = 3000
    cells = np.zeros((S, S), np.int8)
    cells[100:2100, 100:2100] = -50
    for j in range(11):
        for i in range(2):
            cells[100 + 250 * j:300 + 250 * j, 2300 + 300 * i:2500 + 300 * i] = -50
    origin, mpc = _frame((S, S))
    grid = bl.OccupancyGrid.from_cells(cells, origin, mpc, cellsPerMeter=helpers.CPM_DEFAULT, ctx=gpu_ctx)
    rx, ry = float(origin[0]) + 300.5 * 0.05, float(origin[1]) + 1200.5 * 0.05
    exp = oracle.find_frontiers(cells, mpc, helpers.CPM_DEFAULT, origin, oracle.pose(rx, ry, 0.0), 0.1)
    fr = bl.find_map_frontiers(grid, bl.make_pose(rx, ry, 0.0), 0.1)
    assert len(exp) == 1 and len(exp[0]) == 8000
    _sweep_kernel_is(fr, 2)
    _same_frontiers(fr.cells(), exp)


def test_find_map_frontiers_a_grid_width_that_crowded_the_lds_set(oracle, gpu_ctx):
    """The cells of a COLUMN are an arithmetic progression of cell indices with stride W.  Under a multiplicative home alone
    (index * 2654435761 >> 17) their homes step by W * 2654435761 mod 2^32 -- 0.63 slots at W = 10 946, a Fibonacci number (the
    multiplier is the golden ratio's): a vertical frontier of 600 cells needs 600 slots where 380 homes lie, and k_frontier_grow2
    (and k_frontier_grow's visited set behind it) overflowed their home regions and handed the sweep down to the one-workgroup form.
    k_frontier_grow2's home now mixes once more; the map stays as a test.  Same list as the oracle's."""
    W, H = 10946, 800
    cells = np.zeros((H, W), np.int8)
    cells[100:700, 200:500] = -50
    origin, mpc = _frame((H, W))
    grid = bl.OccupancyGrid.from_cells(cells, origin, mpc, cellsPerMeter=helpers.CPM_DEFAULT, ctx=gpu_ctx)
    rx, ry = float(origin[0]) + 300.5 * 0.05, float(origin[1]) + 400.5 * 0.05
    exp = oracle.find_frontiers(cells, mpc, helpers.CPM_DEFAULT, origin, oracle.pose(rx, ry, 0.0), 0.1)
    fr = bl.find_map_frontiers(grid, bl.make_pose(rx, ry, 0.0), 0.1)
    assert len(exp) == 1 and len(exp[0]) == 1800
    _sweep_kernel_is(fr, 3)
    _same_frontiers(fr.cells(), exp)


@pytest.mark.parametrize("shape", [(8, 16384), (16384, 8)])
def test_find_map_frontiers_a_side_beyond_the_lds_flood(oracle, gpu_ctx, shape):
    """k_frontier_flood packs a cell's coordinates into 14 bits each: a grid with a side above 16 380 cells floods through
    k_frontiers<false> instead, and only such a grid does.  131 072 cells (the multi-launch form), unknown but for a free corridor four
    cells wide along the long side with an unknown rim all round; three occupied bars close three of its four lanes each, so the flood
    bends.  The robot stands in the corridor at mid-length.  Same list as the oracle's."""
    H, W = shape
    long_side = max(H, W)
    c = np.zeros((8, long_side), np.int8)                  # laid out along x; transposed below for the tall grid
    c[2:6, 2:long_side - 2] = -50
    c[2:5, long_side // 2 + 300] = 60
    c[3:6, long_side // 2 - 700] = 60
    c[2:5, 1000] = 60
    cells = np.ascontiguousarray(c if W > H else c.T)
    assert cells.shape == shape
    origin, mpc = _frame(shape)
    grid = bl.OccupancyGrid.from_cells(cells, origin, mpc, cellsPerMeter=helpers.CPM_DEFAULT, ctx=gpu_ctx)
    cx, cy = (long_side // 2, 4) if W > H else (4, long_side // 2)
    assert cells[cy, cx] == -50
    rx, ry = float(origin[0]) + (cx + 0.5) * 0.05, float(origin[1]) + (cy + 0.5) * 0.05
    exp = oracle.find_frontiers(cells, mpc, helpers.CPM_DEFAULT, origin, oracle.pose(rx, ry, 0.0), 0.1)
    fr = bl.find_map_frontiers(grid, bl.make_pose(rx, ry, 0.0), 0.1)
    assert len(exp) >= 1
    _same_frontiers(fr.cells(), exp)


def test_find_map_frontiers_through_the_grow_kernel_without_the_cell_set():
    """BOTLAB_FRONTIER_GROW_V1: every sweep of the multi-launch form through k_frontier_grow (the form k_frontier_grow2 hands over to
    when the grid holds more frontier-class cells than its LDS set) -- the tests of that form again, in a child process."""
    import os
    import subprocess
    import sys
    for form in ("1", "2"):                                # 1: from the start; 2: k_frontier_grow2 builds its set, then gives up
        e = dict(os.environ)
        e["BOTLAB_FRONTIER_GROW_V1"] = form
        subprocess.check_call([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                               "-k", "beyond_lds or larger_than_the_visited_set"], env=e)


def test_find_map_frontiers_cut_reference_map(oracle, maps, gpu_ctx):
    m = maps["obstacle_slam_10mx10m_5cm"]
    cells = m["cells"].copy()
    cells[:, 110:] = 0                                     # the right part of the arena has not been seen yet
    grid = bl.OccupancyGrid.from_cells(cells, m["origin"], m["mpc"], cellsPerMeter=helpers.CPM_DEFAULT, ctx=gpu_ctx)
    exp = oracle.find_frontiers(cells, m["mpc"], helpers.CPM_DEFAULT, m["origin"], oracle.pose(-0.75, 0.2, 0.0))
    fr = bl.find_map_frontiers(grid, bl.make_pose(-0.75, 0.2, 0.0))
    _same_frontiers(fr.cells(), exp)
    assert len(exp) >= 2
    # a finished map has no frontier (every shipped map is closed)
    full = bl.OccupancyGrid.from_cells(m["cells"], m["origin"], m["mpc"], cellsPerMeter=helpers.CPM_DEFAULT, ctx=gpu_ctx)
    assert len(bl.find_map_frontiers(full, bl.make_pose(-0.75, 0.2, 0.0))) == 0


def test_batched_searches_equal_single_searches(maps, gpu_ctx):
    cases = helpers.load_astar_cases()
    m = maps["astar_maze"]
    grid = bl.OccupancyGrid.from_cells(m["cells"], m["origin"], m["mpc"], cellsPerMeter=helpers.CPM_DEFAULT, ctx=gpu_ctx)
    pl = bl.MotionPlanner(bl.MotionPlannerParams(0.1), ctx=gpu_ctx)
    pl.setMap(grid)
    start = bl.make_pose(*cases["maze"][0]["start"], 0.3)
    goals = [bl.make_pose(*row["goal"], 0.0) for row in cases["maze"]]
    rng = np.random.default_rng(5)
    for _ in range(30):                                    # anywhere, mostly invalid goals (walls, unknown space, off the grid)
        goals.append(bl.make_pose(float(rng.uniform(-5.2, 5.2)), float(rng.uniform(-5.2, 5.2)), 0.0))
    ys, xs = np.nonzero(pl.distances_.cells() > 0.12)
    for k in rng.integers(len(xs), size=40):               # goals with clearance; with the 4 + 30 above: more than one launch
        goals.append(bl.make_pose(float(m["origin"][0]) + (xs[k] + 0.3) * 0.05, float(m["origin"][1]) + (ys[k] + 0.6) * 0.05, 0.0))
    paths, stats = bl.search_for_path_batch(start, goals, pl.distances_, pl.searchParams_, return_stats=True)
    found = 0
    for g, p, st in zip(goals, paths, stats):
        ref, rst = bl.search_for_path(start, g, pl.distances_, pl.searchParams_, return_stats=True)
        assert len(ref) == len(p) and tuple(rst) == tuple(st)
        assert all((a.utime, a.x, a.y, a.theta) == (b.utime, b.x, b.y, b.theta) for a, b in zip(ref, p))
        found += len(p) > 1
    assert found >= 10


def test_dist_gather_and_is_path_safe(oracle, maps, gpu_ctx):
    m = maps["obstacle_slam_10mx10m_5cm"]
    grid = bl.OccupancyGrid.from_cells(m["cells"], m["origin"], m["mpc"], cellsPerMeter=helpers.CPM_DEFAULT, ctx=gpu_ctx)
    pl = bl.MotionPlanner(ctx=gpu_ctx)
    pl.setMap(grid)
    dist = pl.distances_.cells()
    rng = np.random.default_rng(2)
    q = rng.integers(-3, 204, size=(500, 2)).astype(np.int32)
    out = np.zeros(500, np.float32)
    bl._capi.check(gpu_ctx.lib.bl_dist_gather(pl.distances_.h, q.ctypes.data, 500, out.ctypes.data))
    inside = (q[:, 0] >= 0) & (q[:, 0] < 200) & (q[:, 1] >= 0) & (q[:, 1] < 200)
    assert np.all(np.isnan(out[~inside])) and (~inside).sum() > 5
    assert np.array_equal(out[inside], dist[q[inside, 1], q[inside, 0]])
    start = bl.make_pose(-0.75, 0.2, 0.0)
    n_safe = 0
    for goal in ((-0.35, 0.2), (-0.75, 0.9), (0.0, 0.0), (-0.6, 0.25)):
        path = pl.planPath(start, bl.make_pose(goal[0], goal[1], 0.0))
        arr = (oracle_lib.OPose * len(path))(*[oracle_lib.OPose(p.utime, p.x, p.y, p.theta) for p in path])
        d = oracle.grid(np.ascontiguousarray(dist, dtype=np.float32), m["mpc"], helpers.CPM_DEFAULT, m["origin"])
        exp = bool(oracle.lib.orc_is_path_safe(arr, len(path), C.byref(d), pl.searchParams_.minDistanceToObstacle))
        assert pl.isPathSafe(path) == exp
        n_safe += exp
    assert n_safe >= 1


def _plan_both(oracle, cells, origin, mpc, robot, ctx, num_frontiers=None, prev_goal=None, radius=0.2):
    grid = bl.OccupancyGrid.from_cells(cells, origin, mpc, cellsPerMeter=helpers.CPM_DEFAULT, ctx=ctx)
    pl = bl.MotionPlanner(bl.MotionPlannerParams(radius), ctx=ctx)
    pl.setMap(grid)
    fr = bl.find_map_frontiers(grid, bl.make_pose(*robot))
    lists = fr.cells()
    pl.setNumFrontiers(len(lists) if num_frontiers is None else num_frontiers)
    if prev_goal is not None:
        pl.setPrevGoal(bl.make_pose(*prev_goal))
    path, goal, stats = bl.plan_path_to_frontier(fr, bl.make_pose(*robot), grid, pl, return_info=True)
    dist = oracle.set_distances(cells, mpc, helpers.CPM_DEFAULT, origin)
    exp_fr = oracle.find_frontiers(cells, mpc, helpers.CPM_DEFAULT, origin, oracle.pose(*robot))
    _same_frontiers(lists, exp_fr)
    sp = pl.searchParams_
    pg = None if prev_goal is None else oracle.pose(*prev_goal)
    epath, egoal, est = oracle.plan_path_to_frontier(exp_fr, oracle.pose(*robot), dist, mpc, helpers.CPM_DEFAULT, origin, radius,
                                                     sp.minDistanceToObstacle, sp.maxDistanceWithCost, sp.distanceCostExponent,
                                                     num_frontiers=pl.num_frontiers, prev_goal=pg)
    assert len(path) == len(epath), (len(path), len(epath))
    for a, b in zip(path, epath):
        assert (a.utime, a.x, a.y, a.theta) == (int(b["utime"]), b["x"], b["y"], b["theta"])
    if len(epath) > 1:
        assert (goal.x, goal.y, goal.theta) == egoal
    return path, lists, stats


def test_plan_path_to_frontier_cut_map(oracle, maps, gpu_ctx):
    m = maps["obstacle_slam_10mx10m_5cm"]
    cells = m["cells"].copy()
    cells[:, 110:] = 0
    path, lists, stats = _plan_both(oracle, cells, m["origin"], m["mpc"], (-0.75, 0.2, 0.4), gpu_ctx)
    assert len(lists) >= 2 and len(path) > 3 and stats[2] >= 1
    # prev_goal next to the frontier: every nearby candidate is rejected by isValidGoal until the ring is 0.4 m away
    mid = lists[0][(len(lists[0]) - 1) // 2]
    path2, _, _ = _plan_both(oracle, cells, m["origin"], m["mpc"], (-0.75, 0.2, 0.4), gpu_ctx, prev_goal=(float(mid[0]), float(mid[1]), 0.0))
    assert len(path2) > 3
    # no frontier at all: the empty path
    full = bl.OccupancyGrid.from_cells(m["cells"], m["origin"], m["mpc"], cellsPerMeter=helpers.CPM_DEFAULT, ctx=gpu_ctx)
    pl = bl.MotionPlanner(ctx=gpu_ctx)
    pl.setMap(full)
    assert bl.plan_path_to_frontier(bl.find_map_frontiers(full, bl.make_pose(-0.75, 0.2, 0.0)), bl.make_pose(-0.75, 0.2, 0.0), full, pl) == []


@pytest.mark.parametrize("seed", [0, 2, 5])
def test_plan_path_to_frontier_random_maps(oracle, gpu_ctx, seed):
    shape = (200, 200)
    cells = _blob_map(seed, shape)
    cells[cells == 60] = 0                                 # keep the free blobs roomy enough for a 0.1 m robot
    origin, mpc = _frame(shape)
    dist = oracle.set_distances(cells, mpc, helpers.CPM_DEFAULT, origin)
    ys, xs = np.nonzero(dist > 0.35)
    rng = np.random.default_rng(seed)
    planned = 0
    for _ in range(3):
        k = rng.integers(len(xs))
        robot = (float(origin[0]) + (xs[k] + 0.5) * 0.05, float(origin[1]) + (ys[k] + 0.5) * 0.05, 0.7)
        path, lists, stats = _plan_both(oracle, cells, origin, mpc, robot, gpu_ctx, radius=0.1)
        planned += len(path) > 1
    assert planned >= 1


def test_plan_path_to_frontier_unreachable_gives_failure_path(oracle, gpu_ctx):
    """D8: no candidate goal is ever valid (the robot radius exceeds every clearance) -> the sweep is cut after its
    second wrap and the 1-pose failure path comes back, on both sides."""
    shape = (120, 120)
    cells = np.zeros(shape, np.int8)
    cells[50:70, 50:70] = -30
    origin, mpc = _frame(shape)
    path, lists, stats = _plan_both(oracle, cells, origin, mpc, (0.0, 0.0, 0.0), gpu_ctx, radius=2.0)
    assert len(lists) >= 1 and len(path) == 1 and stats[2] == 0


def test_cpp_planning_dropin_matches_oracle(oracle, maps, tmp_path):
    """include/botlab/planning_dropin.hpp (MotionPlanner, find_map_frontiers, plan_path_to_frontier with the reference's
    signatures) driven like Exploration::executeExploringMap, against the oracle."""
    import os
    import struct
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "tests", "cpp", "planning_test")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-I" + os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "planning_test.cpp"),
                           "-L" + os.path.join(root, "botlab_amd"), "-lbotlab_hip", "-Wl,-rpath," + os.path.join(root, "botlab_amd"), "-o", exe])
    m = maps["obstacle_slam_10mx10m_5cm"]
    cells = m["cells"].copy()
    cells[:, 110:] = 0
    map_path, outp = str(tmp_path / "in.map"), str(tmp_path / "out.bin")
    with open(map_path, "w") as f:                          # .map text format (occupancy_grid.cpp:111-136)
        f.write(f"{m['origin'][0]:g} {m['origin'][1]:g} 200 200 {m['mpc']:g}\n")
        for row in cells:
            f.write(" ".join(str(int(v)) for v in row) + " \n")
    robot = (-0.75, 0.2, 0.4)
    out = subprocess.check_output([exe, map_path, repr(robot[0]), repr(robot[1]), repr(robot[2]), "0.2", outp]).decode()
    assert "planning_test ok" in out
    raw = open(outp, "rb").read()
    off = 0
    nf = struct.unpack_from("<i", raw, off)[0]; off += 4
    got = []
    for _ in range(nf):
        n = struct.unpack_from("<i", raw, off)[0]; off += 4
        got.append(np.frombuffer(raw, np.float32, 2 * n, off).reshape(n, 2)); off += 8 * n
    plen, safe, valid = struct.unpack_from("<iii", raw, off); off += 12
    path = [struct.unpack_from("<qfff", raw, off + 20 * i) for i in range(plen)]; off += 20 * plen
    failed_len = struct.unpack_from("<i", raw, off)[0]; off += 4
    ex_out = struct.unpack_from("<6i", raw, off); off += 24
    ex_target = struct.unpack_from("<ff", raw, off)
    rp = oracle.pose(np.float32(robot[0]), np.float32(robot[1]), np.float32(robot[2]), utime=42)
    exp_fr = oracle.find_frontiers(cells, m["mpc"], helpers.CPM_DEFAULT, m["origin"], rp)
    _same_frontiers(got, exp_fr)
    dist = oracle.set_distances(cells, m["mpc"], helpers.CPM_DEFAULT, m["origin"])
    epath, egoal, _ = oracle.plan_path_to_frontier(exp_fr, rp, dist, m["mpc"], helpers.CPM_DEFAULT, m["origin"], 0.2, 0.2, 2.0, 1.0,
                                                   num_frontiers=len(exp_fr))
    assert plen == len(epath) > 3
    for a, b in zip(path, epath):
        assert a[1:] == (b["x"], b["y"], b["theta"])
    assert path[0][0] == 42 and safe == 1 and valid == 1 and failed_len == 1
    # ExploringMapT: the same two calls on the oracle's composition
    oex = oracle_lib.OracleExploringMap(oracle, 0.2)
    n1, _ = oex.execute(cells, m["mpc"], helpers.CPM_DEFAULT, m["origin"], rp); s1, l1 = oex.status, len(oex.path)
    n2, _ = oex.execute(cells, m["mpc"], helpers.CPM_DEFAULT, m["origin"], rp)
    assert ex_out == (n1, s1, l1, n2, oex.status, len(oex.path))
    assert (np.float32(ex_target[0]), np.float32(ex_target[1])) == oex.target


def test_exploring_map_step_matches_oracle(oracle, maps, gpu_ctx):
    """Exploration::executeExploringMap (exploration.cpp:277-369) as a sequence: the map is uncovered strip by strip while
    the robot follows the planned paths -- next state, status, frontiers, path and target agree with the oracle at every
    step; then the fully known map (no frontier: RETURNING_HOME) and a map whose frontiers cannot be reached (D10: FAILED)."""
    import oracle_lib
    m = maps["obstacle_slam_10mx10m_5cm"]
    cpm = helpers.CPM_DEFAULT
    pl = bl.MotionPlanner(bl.MotionPlannerParams(0.2), ctx=gpu_ctx)
    ex = bl.ExploringMap(pl)
    oex = oracle_lib.OracleExploringMap(oracle, 0.2)
    robot = (-0.75, 0.2, 0.4)
    states = []
    for cut in (110, 110, 125, 140, 200):
        cells = m["cells"].copy()
        cells[:, cut:] = 0
        grid = bl.OccupancyGrid.from_cells(cells, m["origin"], m["mpc"], cellsPerMeter=cpm, ctx=gpu_ctx)
        nxt = ex.execute(grid, bl.make_pose(*robot))
        enxt, efr = oex.execute(cells, m["mpc"], cpm, m["origin"], oracle.pose(*robot))
        _same_frontiers(ex.frontiers_.cells(), efr)
        assert (nxt, ex.status) == (enxt, oex.status), (cut, nxt, ex.status, enxt, oex.status)
        assert len(ex.currentPath_) == len(oex.path)
        for a, b in zip(ex.currentPath_, oex.path):
            assert (a.utime, a.x, a.y, a.theta) == (int(b["utime"]), b["x"], b["y"], b["theta"])
        assert (np.float32(ex.currentTarget_.x), np.float32(ex.currentTarget_.y)) == oex.target
        states.append(nxt)
        if len(ex.currentPath_) > 1:                       # drive most of the way along the path (inside / outside the 0.5 m rule)
            p = ex.currentPath_[(3 * len(ex.currentPath_)) // 4] if cut != 125 else ex.currentPath_[1]
            robot = (float(p.x), float(p.y), float(p.theta))
    assert states[0] == bl.host.STATE_EXPLORING_MAP and states[-1] == bl.host.STATE_RETURNING_HOME
    # frontiers that no goal can reach: a robot wider than every clearance
    shape = (120, 120)
    cells = np.zeros(shape, np.int8)
    cells[50:70, 50:70] = -30
    origin, mpc = _frame(shape)
    pl2 = bl.MotionPlanner(bl.MotionPlannerParams(2.0), ctx=gpu_ctx)
    ex2 = bl.ExploringMap(pl2)
    oex2 = oracle_lib.OracleExploringMap(oracle, 2.0)
    grid = bl.OccupancyGrid.from_cells(cells, origin, mpc, cellsPerMeter=cpm, ctx=gpu_ctx)
    rp = (float(origin[0]) + 60.5 * 0.05, float(origin[1]) + 60.5 * 0.05, 0.0)
    nxt = ex2.execute(grid, bl.make_pose(*rp))
    enxt, _ = oex2.execute(cells, mpc, cpm, origin, oracle.pose(*rp))
    assert nxt == enxt == bl.host.STATE_FAILED_EXPLORATION and ex2.status == oex2.status == bl.host.STATUS_FAILED
