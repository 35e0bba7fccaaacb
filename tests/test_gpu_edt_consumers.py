"""The consumers of a Euclidean distance grid on the GPU -- the navigation field, the local planner over it, the path shortcut and
MotionPlanner.setMetricClearance -- against the models they already have (tests/nav_field_model.py, local_plan_model.py,
path_shortcut_model.py), fed with the Euclidean codes and table of tests/edt_model.py."""
import functools

import numpy as np
import pytest

import botlab_amd as bl
from botlab_amd import _capi
import edt_model as em
import helpers
import local_plan_model as lpm
import nav_field_model as nm
import path_shortcut_model as psm
import test_edt_model_cpu as cpu
import test_nav_field_model_cpu as navcpu

pytestmark = pytest.mark.gpu
CPM = helpers.CPM_DEFAULT
F32 = np.float32
R = 64
P = nm.Params(0.2, 2.0, 1.0, obstacle_gain=50, reach_cells=0)
FIELD_MAPS = ("obstacle_slam_10mx10m_5cm", "astar_convex")


def _c_params(p):
    return _capi.NavFieldParams(p.minDistanceToObstacle, p.maxDistanceWithCost, p.distanceCostExponent, p.obstacle_gain, p.reach_cells)


@functools.lru_cache(maxsize=None)
def _model(name):
    """(codes, table, trav, pen, goals, field) of a golden map by the models, once."""
    cells = helpers.load_reference_maps()[name]["cells"]
    code = em.codes(cells, R)
    f = em.table(R, 0.05)
    trav, pen = nm.tables(f, P)
    goals = [navcpu._far_cell(code, trav)]
    return code, f, trav, pen, goals, nm.dijkstra(code, trav, pen, goals, 0)


_dev = {}


def _device(name, maps, ctx):
    """(map, L1 grid, Euclidean grid) of a golden map on the device, once per module."""
    if name not in _dev:
        m = maps[name]
        g = bl.OccupancyGrid.from_cells(m["cells"], m["origin"], m["mpc"], cellsPerMeter=CPM, ctx=ctx)
        l1 = bl.ObstacleDistanceGrid(ctx=ctx)
        l1.setDistances(g)
        eu = bl.ObstacleDistanceGrid(ctx=ctx, metric="euclidean", max_cells=R)
        eu.setDistances(g)
        assert np.array_equal(eu.codes(), _model(name)[0]) and eu.table().tobytes() == _model(name)[1].tobytes()
        _dev[name] = (g, l1, eu)
    return _dev[name]


def _starts(m, w, h, n, seed):
    rng = np.random.default_rng(seed)
    tuples = []
    for i in range(n):
        x, y = rng.uniform(-1.5, w + 1.5), rng.uniform(-1.5, h + 1.5)
        tuples.append((500 + i, F32(float(m["origin"][0]) + x * float(m["mpc"])), F32(float(m["origin"][1]) + y * float(m["mpc"])), F32(rng.uniform(-3, 3))))
    return tuples


@pytest.mark.parametrize("name", FIELD_MAPS)
def test_field_and_paths_equal_the_model(maps, gpu_ctx, name):
    code, f, trav, pen, goals, field = _model(name)
    m = maps[name]
    _, _, eu = _device(name, maps, gpu_ctx)
    nf = bl.NavigationField(gpu_ctx)
    nf.compute(eu, _c_params(P), goals)
    got = nf.cells()
    assert got.dtype == np.uint32 and got.tobytes() == field.tobytes(), int((got != field).sum())
    dt, dp = nf.tables()
    assert len(dt) == R * R + 2 and np.array_equal(dt, trav) and np.array_equal(dp, pen)
    assert int((field != nm.UNREACHED).sum()) > 500
    h, w = code.shape
    tuples = _starts(m, w, h, 300, 9)
    (buf, lens), labels, costs = nf.paths([bl.make_pose(t[1], t[2], t[3], utime=t[0]) for t in tuples], cap_each=2048, raw=True)
    cache = nm.descend_cache(code, trav, pen, goals, 0)
    longest = 0
    for i, t in enumerate(tuples):
        poses, label, cost = nm.descend(field, code, trav, pen, goals, 0, t, m["origin"], m["mpc"], CPM, _cache=cache)
        assert lens[i] == len(poses) and labels[i] == label and costs[i] == cost, (i, lens[i], len(poses), costs[i], cost)
        for k in ("utime", "x", "y", "theta"):
            assert buf[i, :lens[i]][k].tobytes() == poses[k].tobytes(), (i, k)
        longest = max(longest, len(poses))
        if len(poses) > 1:
            # every cell of the path, the start's included, is farther than 0.2 m from every obstacle: by the table's own rule, and so
            # in integers (17 is the first squared distance whose float exceeds 0.2 m; 16 is 0.2 m exactly)
            q = psm.pose_cells(poses, m["origin"], CPM, w, h)
            c = code[q[:, 1], q[:, 0]]
            assert trav[c].all() and int(c.min()) >= 17, i
    assert longest > 10
    nf.close()


def _gap_device(ctx, offset):
    g = bl.OccupancyGrid.from_cells(cpu.gap_cells(offset), (F32(-1.0), F32(-1.0)), F32(0.05), cellsPerMeter=CPM, ctx=ctx)
    l1 = bl.ObstacleDistanceGrid(ctx=ctx)
    eu = bl.ObstacleDistanceGrid(ctx=ctx, metric="euclidean", max_cells=cpu.GAP_R)
    l1.setDistances(g)
    eu.setDistances(g)
    return g, l1, eu


def test_diagonal_gap_is_closed_in_metres(gpu_ctx):
    """Two wall ends 5 cells apart in x and in y: 10 cells wide by the L1 grid, 0.354 m wide in truth -- no passage for a 0.2 m robot.
    A consumer that silently read the L1 grid would reach the start."""
    sx, sy = cpu.GAP_START
    start = bl.make_pose(-1.0 + (sx + 0.5) * 0.05, -1.0 + (sy + 0.5) * 0.05, 0.0)
    nf = bl.NavigationField(gpu_ctx)
    for offset in (5, 7):
        m_l1, m_eu = cpu.gap_fields(offset)
        g, l1, eu = _gap_device(gpu_ctx, offset)
        assert np.array_equal(eu.codes(), em.codes(cpu.gap_cells(offset), cpu.GAP_R))
        nf.compute(l1, _c_params(cpu.GAP_PARAMS), [cpu.GAP_GOAL])
        f_l1 = nf.cells()
        paths_l1, _, costs_l1 = nf.paths([start])
        nf.compute(eu, _c_params(cpu.GAP_PARAMS), [cpu.GAP_GOAL])
        f_eu = nf.cells()
        paths_eu, _, costs_eu = nf.paths([start])
        assert f_l1.tobytes() == m_l1.tobytes() and f_eu.tobytes() == m_eu.tobytes()
        if offset == 5:
            assert int(f_l1[sy, sx]) == cpu.GAP_L1_FIELD_AT_START == 646 and len(paths_l1[0]) > 1 and int(costs_l1[0]) == 646
            assert int(f_eu[sy, sx]) == nm.UNREACHED and len(paths_eu[0]) == 1 and int(costs_eu[0]) == nm.UNREACHED
        else:
            assert int(f_l1[sy, sx]) != nm.UNREACHED and int(f_eu[sy, sx]) != nm.UNREACHED
            assert len(paths_l1[0]) > 1 and len(paths_eu[0]) > 1 and int(costs_eu[0]) == int(m_eu[sy, sx])
        for x in (l1, eu, g):
            x.close()
    nf.close()


def test_shortcut_equals_the_model_on_the_euclidean_grid(maps, gpu_ctx):
    name = FIELD_MAPS[0]
    code, f, trav, pen, goals, field = _model(name)
    m = maps[name]
    g, l1, eu = _device(name, maps, gpu_ctx)
    h, w = code.shape
    # one path from the Euclidean field, and the L1 field's path over the same map: its cells need not be clear in metres, its own
    # steps stay edges
    l1c = nm.l1_distances(m["cells"])
    lt, lp = nm.tables(nm.dist_table(w, h), P)
    l1_field = nm.dijkstra(l1c, lt, lp, goals, 0)
    cells = []
    for fld, dist, tr, pe in ((field, code, trav, pen), (l1_field, l1c, lt, lp)):
        cache = nm.descend_cache(dist, tr, pe, goals, 0)
        tcell = cache[0]
        reach = np.argwhere(tcell & (fld != nm.UNREACHED))
        far_yx = reach[int(np.argmax(fld[reach[:, 0], reach[:, 1]]))]
        steps = nm.descend_cells(fld, tcell, cache[1], cache[2], (int(far_yx[1]), int(far_yx[0])))
        cells.append(np.array([(int(far_yx[1]), int(far_yx[0]))] + [(x, y) for x, y, _ in steps], np.int64))
    assert len(cells[0]) > 30 and len(cells[1]) > 30
    for clearance, span in ((0.2, 64), (0.3, 16), (10.0, 64)):
        okc = psm.ok_cells(code, psm.ok_table(f, clearance))
        p = psm.Params(clearance, span, 1024)
        sc = bl.PathShortcut(gpu_ctx, clearance=clearance, max_span=span, waypoint_cost=1024)
        keeps, costs = sc.cells(eu, cells)
        for k, q in enumerate(cells):
            ek, ec, ein = psm.shortcut(okc, q, p)
            assert np.array_equal(keeps[k], ek) and (int(costs[k, 0]), int(costs[k, 1])) == (ec, ein), (clearance, k)
            if clearance == 10.0:
                assert len(ek) == len(q)                                            # no cell is that clear: the path comes back unchanged
            head = q[:300]
            assert np.array_equal(sc.visible(eu, head), psm.visible_matrix(okc, head, span)), (clearance, k)
        if clearance == 0.2:
            assert len(keeps[0]) < len(cells[0])
            # the L1 grid answers otherwise for the same cells: the consumer read the grid it was given
            okl = psm.ok_cells(l1c, psm.ok_table(nm.dist_table(w, h), clearance))
            assert not np.array_equal(okl, okc)
            kl, _ = sc.cells(l1, cells)
            assert np.array_equal(kl[1], psm.shortcut(okl, cells[1], p)[0])
        sc.close()


def test_local_planner_over_a_euclidean_field_equals_the_model(maps, gpu_ctx):
    name = FIELD_MAPS[0]
    code, f, trav, pen, goals, field = _model(name)
    m = maps[name]
    _, _, eu = _device(name, maps, gpu_ctx)
    nf = bl.NavigationField(gpu_ctx)
    nf.compute(eu, _c_params(P), goals)
    world = lpm.World(field, code, trav, pen, m["origin"], m["mpc"], CPM)
    p = lpm.Params(v_min=-0.1, v_max=0.5, w_max=2.0, acc_v=1.0, acc_w=6.0, dt_control=0.1, dt_sim=0.05, n_v=6, n_w=11, n_steps=14, w_field=3, w_heading=2,
                   w_clear=2, w_speed=1)
    lp = bl.LocalPlanner(gpu_ctx)
    lp.set_params(p.v_min, p.v_max, p.w_max, p.acc_v, p.acc_w, p.dt_control, p.dt_sim, p.n_v, p.n_w, p.n_steps, p.w_field, p.w_heading, p.w_clear,
                  p.w_speed)
    reached = np.argwhere(world.tcell & (field != nm.UNREACHED))
    rng = np.random.default_rng(4)
    edge = np.argwhere(world.tcell & (code == 17))                                  # cells at the very edge of the metric clearance
    picks = [reached[i] for i in rng.choice(len(reached), 4, replace=False)] + [edge[0], edge[len(edge) // 2]]
    states = []
    for k, (y, x) in enumerate(picks):
        pose = (F32(float(m["origin"][0]) + (x + 0.5) * float(m["mpc"])), F32(float(m["origin"][1]) + (y + 0.5) * float(m["mpc"])), F32(-3.0 + k))
        states.append((pose, F32(0.1 * (k % 3)), F32(0.3 * (k % 2))))
    states.append(((F32(40.0), F32(0.0), F32(0.0)), F32(0.0), F32(0.0)))                 # off the field
    got = lp.commands(nf, [(bl.make_pose(s[0][0], s[0][1], s[0][2], utime=7), s[1], s[2]) for s in states])
    admissible = 0
    for k, (pose, v, w) in enumerate(states):
        exp, _ = lpm.command(world, p, pose, v, w)
        assert all(got[k][c].tobytes() == exp[c].tobytes() for c in ("trans_v", "angular_v", "index", "n_admissible", "cost", "flags")), (k, got[k], exp)
        admissible += int(exp["n_admissible"])
    assert admissible > 0
    lp.close()
    nf.close()


def _same_path(a, b):
    key = lambda q: [(int(p.utime), F32(p.x).tobytes(), F32(p.y).tobytes(), F32(p.theta).tobytes()) for p in q]
    return key(a) == key(b)


def test_motion_planner_metric_clearance(maps, gpu_ctx):
    name = FIELD_MAPS[0]
    code, f, trav, pen, _, _ = _model(name)
    m = maps[name]
    g, _, _ = _device(name, maps, gpu_ctx)
    h, w = code.shape
    plain, off, on = (bl.MotionPlanner(ctx=gpu_ctx) for _ in range(3))
    off.setMetricClearance(32)
    off.setMetricClearance(None)
    on.setMetricClearance(R)
    for mp in (plain, off, on):
        mp.setMap(g)
    assert plain.metricDistances() is None and off.metricDistances() is None
    assert on.metricDistances().metric() == ("euclidean", R) and np.array_equal(on.metricDistances().codes(), code)
    # a start and a goal that both grids call clear, far apart; and a goal only the L1 grid calls clear
    l1c = nm.l1_distances(m["cells"])
    lt, _ = nm.tables(nm.dist_table(w, h), P)
    both = np.argwhere(nm.cell_tables(code, trav, pen)[0])
    centre = lambda yx: (F32(float(m["origin"][0]) + (int(yx[1]) + 0.5) * float(m["mpc"])), F32(float(m["origin"][1]) + (int(yx[0]) + 0.5) * float(m["mpc"])))
    a, b = both[0], both[-1]
    only_l1 = np.argwhere(nm.cell_tables(l1c, lt, np.zeros(len(lt), np.int32))[0] & ~nm.cell_tables(code, trav, pen)[0])[0]
    start = bl.make_pose(*centre(a), 0.25, utime=31)
    for goal_yx in (b, only_l1):
        goal = bl.make_pose(*centre(goal_yx), 0.0)
        ref = plain.planPath(start, goal)
        ref_opt = plain.planPathOptimal(start, goal)
        ref_short = plain.shortcutPath(ref_opt)
        assert _same_path(off.planPath(start, goal), ref) and _same_path(on.planPath(start, goal), ref)       # the search stays on the L1 grid
        assert _same_path(off.planPathOptimal(start, goal), ref_opt) and _same_path(off.shortcutPath(ref_opt), ref_short)
        assert plain.isValidGoal(goal) and on.isValidGoal(goal)                                               # isValidGoal too
        assert on.isPathSafe(ref) == plain.isPathSafe(ref)
        # the model on the metric grid: the goal test is isValidGoal's expression on f[code]
        gc = nm.pose_cell((goal.x, goal.y), m["origin"], CPM, w, h)
        got, cost = on.planPathOptimal(start, goal, return_cost=True)
        if not float(em.floats(code, f)[gc[1], gc[0]]) > 0.2:
            assert goal_yx is only_l1 and len(got) == 1 and cost == nm.UNREACHED
            assert len(ref_opt) > 1                                                                           # the L1 grid let it through
            continue
        goals = [gc]
        field = nm.dijkstra(code, trav, pen, goals, 0)
        poses, _, ecost = nm.descend(field, code, trav, pen, goals, 0, (31, start.x, start.y, start.theta), m["origin"], m["mpc"], CPM)
        assert len(got) == len(poses) > 1 and cost == ecost
        for k in ("x", "y", "theta"):
            assert np.array([getattr(q, k) for q in got], np.float32).tobytes() == poses[k].tobytes(), k
        okc = psm.ok_cells(code, psm.ok_table(f, 0.2))
        exp_short, _, _ = psm.shortcut_poses(okc, poses, m["origin"], CPM, psm.Params(0.2, 64, 1024))
        short = on.shortcutPath(got)
        assert len(short) == len(exp_short) < len(got)
        for k in ("x", "y", "theta"):
            assert np.array([getattr(q, k) for q in short], np.float32).tobytes() == exp_short[k].tobytes(), k
        assert _same_path(on.planPathShortcut(start, goal), short)
    on.setMetricClearance(None)                                                                               # and off again: as if never on
    assert _same_path(on.planPathOptimal(start, bl.make_pose(*centre(b), 0.0)), plain.planPathOptimal(start, bl.make_pose(*centre(b), 0.0)))
