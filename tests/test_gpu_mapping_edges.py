"""Mapping::updateMap on the device (bl_mapping.hip, k_map_update) against the CPU oracle, bit for bit after every update, on the
hand-built inputs of tests/mapping_cases.py: each reaches one form of the kernel -- byte or dword window pass, one window or strips,
segment walk or serial walk, the ray counts where the forms change, counters that saturate, walks chosen cell by cell, the edges of
the frame, stamps outside the interval -- and proves on the CPU that it does (mapping_cases.evaluate) before the device is asked.
Then the replanner snapshot the map kernel leaves behind, for the grids that miss its early form: the fused and the riding call
against the call-by-call form."""
import numpy as np
import pytest

import mapping_cases as mc
import oracle_lib
import botlab_amd as bl
from botlab_amd._capi import BL_ERR_ARG, BotlabHipError

pytestmark = pytest.mark.gpu


def _differences(got, ref):
    ys, xs = np.nonzero(got != ref)
    return f"{len(xs)} cells differ, first (x, y, got, want): " + str([(int(x), int(y), int(got[y, x]), int(ref[y, x])) for x, y in zip(xs[:8], ys[:8])])


def _run(case, oracle, ctx):
    """The case on the device; the grid equals the oracle's after every update."""
    refs, _ = mc.evaluate(case, oracle)
    g = bl.OccupancyGrid.from_cells(case.start, case.origin, case.mpc, ctx=ctx)
    assert g.cpm == case.cpm and g.mpc == case.mpc
    mapper = bl.Mapping(case.max_laser, case.hit, case.miss, ctx=ctx)
    for k, (scan, p) in enumerate(case.updates):
        mapper.updateMap(scan, bl.make_pose(p[0], p[1], p[2], utime=p[3]), g)
        got = g.cells()
        assert np.array_equal(got, refs[k]), f"{case.name}, update {k}: " + _differences(got, refs[k])
    return g, mapper


@pytest.mark.parametrize("name", list(mc.BUILDERS))
def test_map_update_equals_oracle(oracle, gpu_ctx, name):
    g, mapper = _run(mc.get(name, oracle), oracle, gpu_ctx)
    mapper.close(); g.close()


@pytest.mark.parametrize("form", ["pair", "one", "serial"])
@pytest.mark.parametrize("hit,miss", mc.SATURATION_ODDS)
def test_counter_halves_and_saturation(oracle, gpu_ctx, form, hit, miss):
    """Hundreds of rays ending in two neighbouring cells of one counter dword (or 1024 in one cell), cells that are end cells and
    crossed cells at once, start values at and next to both ends of int8, odds that saturate in one step or change nothing."""
    for shift in range(7):
        g, mapper = _run(mc.counters(oracle, form, hit, miss, shift), oracle, gpu_ctx)
        mapper.close(); g.close()


def test_scan_longer_than_the_kernel_takes_is_refused(oracle, gpu_ctx):
    """num_ranges = 8193 is an argument error whatever the ranges hold; the grid and the mapper stay as they were: the next update
    interpolates from the pose of the last accepted one."""
    case = mc.get("ray_count_65_of_102", oracle)
    refs, _ = mc.evaluate(case, oracle)
    g, mapper = _run(case, oracle, gpu_ctx)
    om = oracle_lib.OracleMapping(oracle, case.max_laser, case.hit, case.miss)
    ref = case.start.copy()
    for scan, p in case.updates:
        om.update(scan, oracle.pose(p[0], p[1], p[2], utime=p[3]), ref, case.mpc, case.cpm, case.origin)
    assert np.array_equal(ref, refs[-1])
    n = mc.MAX_RAYS + 1
    rng = np.random.default_rng(8193)
    t = case.updates[-1][1][3] + 100_000
    for ranges in (rng.uniform(0.2, 4.0, n), np.full(n, 0.1)):
        long_scan = bl.LidarScan(ranges, rng.uniform(-3, 3, n), np.full(n, t, np.int64), utime=t)
        with pytest.raises(BotlabHipError, match=f"status {BL_ERR_ARG}"):
            mapper.updateMap(long_scan, bl.make_pose(0.5, 0.0, 0.4, utime=t), g)
        assert np.array_equal(g.cells(), ref)
    scan = bl.LidarScan(long_scan.ranges[:mc.MAX_RAYS] + np.float32(2.0), long_scan.thetas[:mc.MAX_RAYS], np.full(mc.MAX_RAYS, t - 30_000, np.int64), utime=t)
    mapper.updateMap(scan, bl.make_pose(0.5, 0.0, 0.4, utime=t), g)
    om.update(scan, oracle.pose(0.5, 0.0, 0.4, utime=t), ref, case.mpc, case.cpm, case.origin)
    got = g.cells()
    assert np.array_equal(got, ref), _differences(got, ref)
    assert not np.array_equal(ref, refs[-1])
    mapper.close(); g.close()


# ------------------------------------------------------------------ the snapshot the map kernel leaves for the replanner
def _snapshot_run(form, ctx, W, H, rays, robot_cell, goal_cell):
    mpc = np.float32(0.05)
    origin = (np.float32(-0.5 * W * 0.05), np.float32(-0.5 * H * 0.05))
    g = bl.OccupancyGrid.from_cells(np.zeros((H, W), np.int8), origin, mpc, ctx=ctx)
    at = lambda c: (float(origin[0]) + c[0] * 0.05, float(origin[1]) + c[1] * 0.05)
    x0, y0 = at(robot_cell)
    goal = bl.make_pose(*at(goal_cell), 0.0)
    d = np.arange(rays) * (2 * np.pi / rays)
    pf = bl.ParticleFilter(500, ctx=ctx)
    pf.initializeFilterAtPose(bl.make_pose(x0, y0, 0.0, utime=1_000_000), seed=5)
    pf.setNoiseSeed(9)
    mapper = bl.Mapping(5.0, 4, 6, ctx=ctx)                     # miss odds 6: a crossed cell is free (and no source of distances) at once
    planner = bl.AsyncPlanner(ctx=ctx, lanes=1, batch=1)
    rec, pending = [], 0

    def fetch():
        path, stats = planner.fetch(return_stats=True)
        rec.append(([(p.utime, p.x, p.y, p.theta) for p in path], stats))

    for k in range(6):
        t = 1_100_000 + k * 100_000
        sc = bl.LidarScan(1.5 + 0.4 * np.sin(3 * d + 0.2 * k), -d, t - 100_000 + (np.arange(rays, dtype=np.int64) + 1) * 100_000 // rays, utime=t)
        odo = bl.make_pose(x0 + 0.02 * (k + 1), y0 + 0.01 * (k + 1), 0.03 * (k + 1), utime=t)
        if form == "riding":
            pf.updateBegin(odo, sc, g, 1000 + k)
            planner.submit_with_map_update_finishing(mapper, sc, pf, t, g, goal)
        else:
            pf.updateFilter(odo, sc, g, rand_value=1000 + k, want_pose=False)
            if form == "fused":
                planner.submit_with_map_update(mapper, sc, pf.poseDevicePtr(), t, g, goal)
            else:
                mapper.updateMapDevicePose(sc, pf.poseDevicePtr(), t, g)
                planner.submit(g, pf.poseDevicePtr(), goal)
        pending += 1
        if pending > 2:
            fetch(); pending -= 1
    while pending:
        fetch(); pending -= 1
    cells = g.cells().copy()
    planner.close(); mapper.close(); pf.close(); g.close()
    return rec, cells


@pytest.mark.parametrize("W,H,rays,where", [(203, 197, 290, "corner"),     # n % 16 == 7, byte rows: the copy loop and its tail
                                            (300, 300, 290, "centre"),     # more than 64 KB, dword rows: the copy loop
                                            (512, 512, 290, "centre"),     # 256 K cells exactly: still copied in the kernel
                                            (516, 512, 290, "centre"),     # the first size over it: a snapshot launch of its own
                                            (200, 200, 1500, "centre")])   # the serial walk misses the early form too
def test_snapshot_forms_agree_beyond_the_early_copy(gpu_ctx, W, H, rays, where):
    """The map update that also leaves the replanner's snapshot (fused), the one that ends the filter update as well (riding) and the
    three separate calls give the same paths, search counts, start poses and map.  The snapshot cannot be read from outside: a cell
    it misses shows in the paths and counts of the searches that run on it.  In the corner case the robot uncovers the last cells of
    the grid and the goal lies two cells from them: while they are unknown (a snapshot whose tail was not copied keeps them so) the
    goal is invalid and the path has one pose."""
    if where == "corner":
        robot, goal = (W - 10.5, H - 8.5), (W - 3.5, H - 2.5)
    else:
        robot, goal = (W / 2 + 0.5, H / 2 + 0.5), (W / 2 + 10.5, H / 2 + 6.5)
    out = {f: _snapshot_run(f, gpu_ctx, W, H, rays, robot, goal) for f in ("async", "fused", "riding")}
    rec, cells = out["async"]
    assert len(rec) == 6 and max(len(r[0]) for r in rec) > 3 and max(r[1][0] for r in rec) > 3      # real searches
    if where == "corner":
        assert (cells.ravel()[-7:] < 0).all()                   # the last seven cells (0 at the start): uncovered, all free
        assert len(rec[-1][0]) > 3
    assert (cells != 0).sum() > 1000
    for f in ("fused", "riding"):
        assert out[f][0] == rec, f
        assert np.array_equal(out[f][1], cells), f
