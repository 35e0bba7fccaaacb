"""Scan history and map rebuild on the device (bl_scanlog_*, botlab_amd.ScanHistory) against the definition: K sequential
OracleMapping.update calls (tests/map_rebuild_model.truth), byte for byte, on the cases of tests/map_rebuild_cases.py -- scan counts
around the chunk size, pose jumps, saturation and order, grid shapes, the time rule, poses and windows, another frame -- and the
log itself: device poses, the ring, refused scans, bad arguments.  The stats of every rebuild (chunks, pairs) must be the model's, which
shows the path an input took."""
import ctypes as C

import numpy as np
import pytest

import botlab_amd as bl
import map_rebuild_cases as cases
import map_rebuild_model as mm
from botlab_amd import _capi

pytestmark = pytest.mark.gpu
BL_ERR_ARG, BL_ERR_STATE = 2, 4


def _pose(p):
    return bl.make_pose(p[0], p[1], p[2], utime=p[3])


def _fields(poses):
    """(utime, x, y, theta) of a POSE_DTYPE array, without its padding."""
    return [(int(q["utime"]), q["x"], q["y"], q["theta"]) for q in poses]


def _grid(ctx, case, cells=None):
    g = bl.OccupancyGrid.from_cells(case.base if cells is None else cells, case.origin, case.mpc, ctx=ctx)
    assert g.cpm == case.cpm
    return g


def _log(ctx, entries, capacity=None, max_rays=None):
    need = max(max(s.num_ranges for s, _ in entries), 1)
    log = bl.ScanHistory(capacity or len(entries), max_rays or need, ctx=ctx)
    for s, p in entries:
        log.append(s, _pose(p))
    return log


def _rebuild(log, case, out, base, poses="case"):
    poses = case.poses if poses == "case" else poses
    log.rebuild(out, case.max_laser, case.hit, case.miss, first=case.first, count=case.count,
                poses=None if poses is None else [_pose(p) for p in poses], prev_pose=None if case.prev is None else _pose(case.prev), base=base)


@pytest.mark.parametrize("name", sorted(cases.BUILDERS))
def test_rebuild_equals_sequential_updates(gpu_ctx, oracle, name):
    case = cases.get(name, oracle)
    res = cases.evaluate(case, oracle)
    log = _log(gpu_ctx, case.entries)
    base = _grid(gpu_ctx, case)
    out = _grid(gpu_ctx, case, np.full_like(case.base, 55))      # whatever `out` held is gone
    try:
        _rebuild(log, case, out, base)
        got = out.cells()
        st = log.stats()
        print(name, st)
        assert np.array_equal(base.cells(), case.base)           # the base is only read
        assert np.array_equal(got, res["truth"]), f"{(got != res['truth']).sum()} cells differ"
        assert (st.scans, st.chunks, st.pairs, st.tiles) == (res["info"]["scans"], res["chunks"], res["pairs"], res["info"]["tiles"])
        assert st.chunk_scans == mm.CHUNK and st.tile_cells == mm.TILE and st.scratch_bytes == st.pairs * mm.TILE * mm.TILE * 4
        assert len(log) == len(case.entries)
    finally:
        log.close(); base.close(); out.close()


@pytest.mark.parametrize("name", ["counts_17_latch", "equal_utime", "saturation_127_127_127", "jump_8m"])
def test_base_may_be_out_itself_or_absent(gpu_ctx, oracle, name):
    case = cases.get(name, oracle)
    res = cases.evaluate(case, oracle)
    scans, poses = case.window()
    zero = mm.truth(oracle, scans, poses, case.prev, np.zeros_like(case.base), case.mpc, case.cpm, case.origin, case.max_laser, case.hit, case.miss)
    log = _log(gpu_ctx, case.entries)
    out = _grid(gpu_ctx, case)
    try:
        _rebuild(log, case, out, out)                            # base == out
        assert np.array_equal(out.cells(), res["truth"])
        _rebuild(log, case, out, None)                           # all zero, whatever `out` holds now
        assert np.array_equal(out.cells(), zero) and not np.array_equal(zero, res["truth"])
    finally:
        log.close(); out.close()


def test_recorded_poses_passed_poses_and_set_poses(gpu_ctx, oracle):
    case = cases.get("other_poses", oracle)
    res = cases.evaluate(case, oracle)
    scans = [s for s, _ in case.entries]
    recorded = [p for _, p in case.entries]
    at_recorded = mm.truth(oracle, scans, recorded, None, case.base, case.mpc, case.cpm, case.origin, case.max_laser, case.hit, case.miss)
    log = _log(gpu_ctx, case.entries)
    base, out = _grid(gpu_ctx, case), _grid(gpu_ctx, case)
    try:
        _rebuild(log, case, out, base, poses=None)
        assert np.array_equal(out.cells(), at_recorded)
        _rebuild(log, case, out, base)                           # the case's poses, passed
        assert np.array_equal(out.cells(), res["truth"])
        got = log.poses()
        assert _fields(got) == [(p[3], np.float32(p[0]), np.float32(p[1]), np.float32(p[2])) for p in recorded]
        log.set_poses(3, [_pose(p) for p in case.poses[3:]])     # a corrected trajectory, kept
        log.set_poses(0, [_pose(p) for p in case.poses[:3]])
        _rebuild(log, case, out, base, poses=None)
        assert np.array_equal(out.cells(), res["truth"])
        assert _fields(log.poses(5, 2)) == _fields(bl.host._pose_array([_pose(p) for p in case.poses[5:7]]))
    finally:
        log.close(); base.close(); out.close()


def test_poses_read_from_the_device_equal_the_host_form(gpu_ctx, oracle):
    import torch
    case = cases.get("counts_17_latch", oracle)
    res = cases.evaluate(case, oracle)
    host = _log(gpu_ctx, case.entries)
    dev = bl.ScanHistory(len(case.entries), 290, ctx=gpu_ctx)
    out = _grid(gpu_ctx, case)
    try:
        for s, p in case.entries:
            q = bl.make_pose(p[0], p[1], p[2], utime=777)        # the utime in device memory is not the one recorded
            t = torch.from_numpy(np.frombuffer(bytes(q), np.uint8).copy()).cuda()
            torch.cuda.synchronize()
            dev.append_device_pose(s, t.data_ptr(), p[3])
            gpu_ctx.sync()                                       # (the tensor may go once the append has run)
        assert _fields(dev.poses()) == _fields(host.poses()) and len(dev) == len(case.entries)
        _rebuild(dev, case, out, out)
        assert np.array_equal(out.cells(), res["truth"])
    finally:
        host.close(); dev.close(); out.close()


def test_ring_drops_the_oldest_and_a_window_is_primed(gpu_ctx, oracle):
    whole, ent = cases.ring_all(oracle)
    window, _ = cases.ring_window(oracle)
    assert len(ent) == cases.RING_APPENDS and len(whole.entries) == cases.RING_CAPACITY
    log = _log(gpu_ctx, ent, capacity=cases.RING_CAPACITY)
    base, out = _grid(gpu_ctx, whole), _grid(gpu_ctx, whole)
    try:
        assert len(log) == cases.RING_CAPACITY
        held = ent[cases.RING_APPENDS - cases.RING_CAPACITY:]
        assert [int(t) for t in log.poses()["utime"]] == [p[3] for _, p in held]          # index 0 is the oldest retained scan
        for i, (s, _) in enumerate(held):
            r, th, tm = log.scan(i)
            keep = s.ranges > mm.MIN_RANGE
            assert np.array_equal(r, s.ranges[keep]) and np.array_equal(th, s.thetas[keep]) and np.array_equal(tm, s.times[keep])
        _rebuild(log, whole, out, base)
        assert np.array_equal(out.cells(), cases.evaluate(whole, oracle)["truth"])
        assert window.first == len(log) - cases.RING_WINDOW and window.prev == held[window.first - 1][1]
        _rebuild(log, window, out, base)
        assert np.array_equal(out.cells(), cases.evaluate(window, oracle)["truth"])
    finally:
        log.close(); base.close(); out.close()


def test_kept_rays_are_what_the_log_holds_and_too_many_are_refused(gpu_ctx, oracle):
    case = cases.get("zero_kept", oracle)
    log = _log(gpu_ctx, case.entries)
    small = bl.ScanHistory(4, 290, ctx=gpu_ctx)
    full = bl.ScanHistory(2, 8192, ctx=gpu_ctx)
    try:
        assert [len(log.scan(i)[0]) for i in range(len(log))] == [290, 290, 0, 290, 290]
        s, p = case.entries[0]
        r = np.concatenate([s.ranges, np.full(10, 0.1, np.float32)])        # 300 ranges, 290 kept: taken
        th, tm = np.concatenate([s.thetas, s.thetas[:10]]), np.concatenate([s.times, s.times[:10]])
        small.append(bl.LidarScan(r, th, tm, utime=s.utime), _pose(p))
        r[-1] = 1.0                                                          # 291 kept: refused, the log as it was
        with pytest.raises(bl.BotlabHipError):
            small.append(bl.LidarScan(r, th, tm, utime=s.utime), _pose(p))
        assert len(small) == 1 and len(small.scan(0)[0]) == 290
        big = cases.get("ray_count_8192", oracle).entries[0][0]
        full.append(big, _pose(p))
        over = bl.LidarScan(np.append(big.ranges, np.float32(1.0)), np.append(big.thetas, np.float32(0.0)), np.append(big.times, big.times[-1]), utime=big.utime)
        assert over.num_ranges == 8193
        with pytest.raises(bl.BotlabHipError):
            full.append(over, _pose(p))
        assert len(full) == 1 and len(full.scan(0)[0]) == 8192
    finally:
        log.close(); small.close(); full.close()


def test_bad_arguments_leave_out_and_the_log_untouched(gpu_ctx, oracle):
    case = cases.get("counts_2_latch", oracle)
    lib = gpu_ctx.lib
    log = _log(gpu_ctx, case.entries)
    mark = np.full_like(case.base, 55)
    out, base = _grid(gpu_ctx, case, mark), _grid(gpu_ctx, case)
    wide = bl.OccupancyGrid.from_cells(np.zeros((case.height, case.width + 1), np.int8), case.origin, case.mpc, ctx=gpu_ctx)
    moved = bl.OccupancyGrid.from_cells(case.base, (case.origin[0] + 1.0, case.origin[1]), case.mpc, ctx=gpu_ctx)
    other = bl.Context(0)
    foreign = bl.OccupancyGrid.from_cells(case.base, case.origin, case.mpc, ctx=other)
    stats = _capi.ScanLogStats()
    n = len(log)
    before = _fields(log.poses())
    try:
        assert lib.bl_scanlog_last_stats(log.h, C.byref(stats)) == BL_ERR_STATE           # no rebuild yet

        def refused(first, count, hit, miss, b, o, poses=None):
            return lib.bl_scanlog_rebuild(log.h, first, count, poses, None, 5.0, hit, miss, b, o)

        assert refused(0, 0, 3, 1, base.h, out.h) == BL_ERR_ARG
        assert refused(-1, 2, 3, 1, base.h, out.h) == BL_ERR_ARG
        assert refused(0, n + 1, 3, 1, base.h, out.h) == BL_ERR_ARG
        assert refused(n, 1, 3, 1, base.h, out.h) == BL_ERR_ARG
        assert refused(0, n, -1, 1, base.h, out.h) == BL_ERR_ARG
        assert refused(0, n, 3, -1, base.h, out.h) == BL_ERR_ARG
        assert refused(0, n, 3, 1, wide.h, out.h) == BL_ERR_ARG                            # a base of another shape
        assert refused(0, n, 3, 1, moved.h, out.h) == BL_ERR_ARG                           # ... of another frame
        assert refused(0, n, 3, 1, base.h, None) == BL_ERR_ARG
        assert refused(0, n, 3, 1, None, foreign.h) == BL_ERR_ARG                          # a grid of another ctx
        q = bl.host._pose_array([_pose(case.entries[0][1])])
        assert lib.bl_scanlog_get_poses(log.h, 0, n + 1, q.ctypes.data) == BL_ERR_ARG
        assert lib.bl_scanlog_set_poses(log.h, n, 1, q.ctypes.data) == BL_ERR_ARG
        assert lib.bl_scanlog_set_poses(log.h, 0, 1, None) == BL_ERR_ARG
        assert lib.bl_scanlog_get_scan(log.h, n, None, None, None, None) == BL_ERR_ARG
        assert lib.bl_scanlog_last_stats(log.h, C.byref(stats)) == BL_ERR_STATE
        assert np.array_equal(out.cells(), mark) and np.array_equal(base.cells(), case.base)
        assert len(log) == n and _fields(log.poses()) == before
        _rebuild(log, case, out, base)                           # and the same objects still work
        assert np.array_equal(out.cells(), cases.evaluate(case, oracle)["truth"])
    finally:
        log.close(); out.close(); base.close(); wide.close(); moved.close(); foreign.close(); other.close()
