"""The obstacle layer on the device (bl_obslayer_*, botlab_amd/csrc/bl_obslayer.hip) against its model
(tests/obstacle_layer_model.py), value for value after every step of a script: the class of every ray, count, last, n, the stats, the
list of live cells and the composed grid."""
import math

import numpy as np
import pytest

import botlab_amd as bl
from botlab_amd import synth
import helpers
import obstacle_layer_model as om
import test_obstacle_layer_model_cpu as cpu

pytestmark = pytest.mark.gpu
F32 = np.float32


class Device:
    """A script's map and layer on the device."""

    def __init__(self, ctx, script):
        w, h = script.shape
        self.script = script
        self.params = dict(script.params)
        self.grid = bl.OccupancyGrid.from_cells(script.cells, script.origin, script.mpc, cellsPerMeter=script.cpm, ctx=ctx)
        self.out = bl.OccupancyGrid.from_cells(np.zeros_like(script.cells), (F32(7.0), F32(7.0)), script.mpc, cellsPerMeter=script.cpm, ctx=ctx)
        self.layer = bl.ObstacleLayer(w, h, ctx=ctx, **self.params)

    def step(self, st):
        """The outcome of one step: "ok", "arg" or "state"."""
        try:
            if st[0] == "update":
                self.layer.update(self.grid, bl.LidarScan(st[1], st[2], np.zeros(len(st[1]), np.int64)), bl.make_pose(*st[3]))
            elif st[0] == "upload":
                self.layer.upload(st[1], st[2], st[3])
            elif st[0] == "params":
                p = dict(self.params, **st[1])
                self.layer.setParams(**p)
                self.params = p
            else:
                self.layer.reset()
        except bl.BotlabHipError as e:
            return {"status 2": "arg", "status 4": "state"}[[k for k in ("status 2", "status 4") if k in str(e)][0]]
        return "ok"

    def snapshot(self):
        count, last, n = self.layer.download()
        self.layer.compose(self.grid, self.out)
        assert (self.out.mpc, self.out.cpm, self.out.origin) == (self.grid.mpc, self.grid.cpm, self.grid.origin)
        return dict(classes=self.layer.classes(), count=count, last=last, n=n, stats=self.layer.stats(), live=self.layer.live_cells(),
                    composed=self.out.cells())

    def close(self):
        for x in (self.layer, self.out, self.grid):
            x.close()


def same(got, exp, where):
    assert got["n"] == exp["n"], where
    for k in ("classes", "count", "last", "live", "composed"):
        assert got[k].dtype == exp[k].dtype and got[k].shape == exp[k].shape, (where, k, got[k].shape, exp[k].shape)
        bad = np.flatnonzero(got[k].ravel() != exp[k].ravel())
        assert len(bad) == 0, (where, k, len(bad), int(bad[0]), got[k].ravel()[bad[0]], exp[k].ravel()[bad[0]])
    assert got["stats"] == exp["stats"], (where, got["stats"], exp["stats"])


def run_both(ctx, script, every=True):
    """The script on the device beside the model; every step's outcome and (every: each step's, else the last step's) snapshot equal."""
    model = cpu.run_model(script)
    dev = Device(ctx, script)
    try:
        for k, st in enumerate(script.steps):
            res = dev.step(st)
            assert res == model[k][0], (k, st[0], res, model[k][0])
            if every or k == len(script.steps) - 1:
                same(dev.snapshot(), model[k][1], (k, st[0]))
    finally:
        dev.close()
    return model


@pytest.mark.parametrize("w,h,tol", [(37, 23, 0), (37, 23, 1), (37, 23, 3), (64, 64, 1), (131, 67, 1), (131, 67, 16)])
def test_conditions_equal_the_model(gpu_ctx, w, h, tol):
    model = run_both(gpu_ctx, cpu.conditions_script(w, h, tol))
    if (w, h) == (37, 23):
        assert set(model[0][1]["classes"].tolist()) == {0, 1, 2, 3, 4}


@pytest.mark.parametrize("w,h", [(37, 23), (64, 64), (131, 67)])
def test_lifecycle_equals_the_model(gpu_ctx, w, h):
    model = run_both(gpu_ctx, cpu.lifecycle_script(w, h))
    assert model[18][0] == "state" and int(model[15][1]["count"].max()) == 255


def test_half_metre_cells_and_the_ray_that_stays_in_its_cell(gpu_ctx):
    run_both(gpu_ctx, cpu.coarse_script())


@pytest.mark.parametrize("rays,invalid", [(0, 0), (1, 0), (63, 0), (64, 0), (65, 3), (290, 0), (4096, 7), (4097, 0)])
def test_ray_counts(gpu_ctx, rays, invalid):
    model = run_both(gpu_ctx, cpu.ray_count_script(rays, extra_invalid=invalid))
    assert model[0][0] == ("arg" if rays > 4096 else "ok") and model[0][1]["stats"]["valid"] == (rays if rays <= 4096 else 0)


def test_shipped_map_five_updates_from_moving_poses(gpu_ctx, maps):
    m = maps["obstacle_slam_10mx10m_5cm"]
    cells = m["cells"]
    truth = np.where(cells > 0, 127, -127).astype(np.int8)
    free = np.argwhere(cells[80:120, 60:100] < 0)
    by, bx = free[len(free) // 2] + (80, 60)
    truth[by - 2:by + 3, bx - 2:bx + 3] = 127                                 # what the map does not know
    s = cpu.Script(cells, origin=m["origin"], mpc=m["mpc"], cpm=helpers.CPM_DEFAULT, max_range=5.0, min_hits=2, ttl_scans=3)
    poses = synth.square_trajectory((-0.75, 0.2, 0.0), 5, step_len=0.04, side=0.8)
    for k in range(1, 6):
        scan = synth.raycast_scan(truth, m["origin"], 0.05, poses[k], poses[k], 1000 * k, max_range=5.0)
        s.steps.append(("update", scan.ranges, scan.thetas, tuple(F32(v) for v in poses[k])))
    model = run_both(gpu_ctx, s)
    print("shipped map: rays by class", model[-1][1]["stats"]["classes"], "live", model[-1][1]["stats"]["live"])
    assert model[-1][1]["stats"]["classes"][om.EXPLAINED] > 100


def test_long_walks_on_a_large_grid(gpu_ctx):
    rng = np.random.default_rng(17)
    w = h = 1000
    cells = np.where(rng.random((h, w)) < 1e-3, 100, -100).astype(np.int8)
    s = cpu.Script(cells, origin=(F32(-25.0), F32(-25.0)), max_range=10.0, tol_cells=2)
    for k, (cx, cy) in enumerate(((500.3, 499.7), (120.5, 880.5), (995.5, 3.5))):      # the middle, and two poses whose walks leave the grid
        r = rng.uniform(9.0, 9.6, 290).astype(np.float32)
        t = (2 * math.pi * np.arange(290) / 290).astype(np.float32)
        s.steps.append(("update", r, t, s.pose_at(cx, cy, 0.1 * k)))
    model = run_both(gpu_ctx, s)
    st = model[-1][1]["stats"]
    print("1000 x 1000, walks of ~190 cells:", st)
    assert st["clr"] > 5000


def _transform(ctx, cells, script, metric):
    """The distance grid of `cells` by a fresh transform of a fresh grid."""
    g = bl.OccupancyGrid.from_cells(cells, script.origin, script.mpc, cellsPerMeter=script.cpm, ctx=ctx)
    d = bl.ObstacleDistanceGrid(ctx=ctx, metric=metric, max_cells=20) if metric == "euclidean" else bl.ObstacleDistanceGrid(ctx=ctx)
    try:
        d.setDistances(g)
        return d.cells()
    finally:
        d.close()
        g.close()


def test_composed_grid_through_the_distance_grids_twice(gpu_ctx):
    s = cpu.conditions_script(131, 67, 1)
    model = cpu.run_model(s)
    dev = Device(gpu_ctx, s)
    l1 = bl.ObstacleDistanceGrid(ctx=gpu_ctx)
    eu = bl.ObstacleDistanceGrid(ctx=gpu_ctx, metric="euclidean", max_cells=20)
    planner = bl.MotionPlanner(ctx=gpu_ctx)
    try:
        seen = []
        for k in (0, 1, 2, 3):                                             # after the fourth step other cells are live than after the first
            assert dev.step(s.steps[k]) == "ok"
            if k in (0, 3):
                exp = model[k][1]["composed"]
                seen.append(exp)
                dev.layer.compose(dev.grid, dev.out)
                assert np.array_equal(dev.out.cells(), exp)
                for d, metric in ((l1, "l1"), (eu, "euclidean")):
                    d.setDistances(dev.out)                                # the same grid object both times: a new lineage each compose
                    assert np.array_equal(d.cells().view(np.uint32), _transform(gpu_ctx, exp, s, metric).view(np.uint32)), (k, metric)
                planner.setMapWithObstacles(dev.grid, dev.layer)
                assert np.array_equal(planner.distances_.cells().view(np.uint32), _transform(gpu_ctx, exp, s, "l1").view(np.uint32)), k
                assert np.array_equal(dev.grid.cells(), s.cells)           # the map itself is untouched
        assert not np.array_equal(seen[0], seen[1]) and (seen[0] == 127).any() and (seen[1] == 127).any()
    finally:
        for x in (l1, eu):
            x.close()
        dev.close()


def test_upload_download_round_trip_and_live_list_cap(gpu_ctx):
    rng = np.random.default_rng(23)
    w, h = 131, 67
    s = cpu.Script(cpu.open_cells(w, h), ttl_scans=40, min_hits=3)
    dev = Device(gpu_ctx, s)
    try:
        count = rng.integers(0, 8, (h, w)).astype(np.uint8)
        last = rng.integers(0, 100, (h, w)).astype(np.uint32)
        dev.layer.upload(count, last, 90)
        c, l, n = dev.layer.download()
        assert np.array_equal(c, count) and np.array_equal(l, last) and n == 90
        m = om.Layer(w, h, **s.params)
        m.upload(count, last, 90)
        live = dev.layer.live_cells()
        assert len(live) > 300 and np.array_equal(live, m.live_cells())
        assert np.array_equal(dev.layer.live_cells(cap=5), live[:5]) and len(dev.layer.live_cells(cap=0)) == 0
        st = dev.layer.stats()
        assert (st["n"], st["hs"], st["clr"], st["live"]) == (90, 0, 0, len(live))
        dev.layer.compose(dev.grid, dev.out)
        assert np.array_equal(dev.out.cells(), m.compose(s.cells))
        dev.layer.update(dev.grid, bl.LidarScan(np.zeros(0, F32), np.zeros(0, F32), np.zeros(0, np.int64)), bl.make_pose(*s.pose_at(5.5, 5.5)))
        um, cm = dev.layer.lastDeviceMs()
        assert um >= 0 and cm > 0
    finally:
        dev.close()


def test_error_returns(gpu_ctx):
    s = cpu.conditions_script(37, 23, 1)
    dev = Device(gpu_ctx, s)
    other = bl.OccupancyGrid.from_cells(np.zeros((23, 38), np.int8), s.origin, s.mpc, cellsPerMeter=s.cpm, ctx=gpu_ctx)
    try:
        assert dev.step(s.steps[0]) == "ok"
        before = dev.snapshot()
        scan = bl.LidarScan(s.steps[0][1], s.steps[0][2], np.zeros(len(s.steps[0][1]), np.int64))
        pose = bl.make_pose(*s.steps[0][3])
        with pytest.raises(bl.BotlabHipError, match="status 2"):
            dev.layer.update(other, scan, pose)                            # a map of another shape
        with pytest.raises(bl.BotlabHipError, match="status 2"):
            dev.layer.compose(dev.grid, dev.grid)                          # into the map itself
        with pytest.raises(bl.BotlabHipError, match="status 2"):
            dev.layer.compose(dev.grid, other)
        for bad in (dict(max_range=float("nan")), dict(max_range=float("inf")), dict(occ_min=0), dict(tol_cells=-1), dict(ttl_scans=0),
                    dict(min_hits=256)):
            with pytest.raises(bl.BotlabHipError, match="status 2"):
                dev.layer.setParams(**dict(dev.params, **bad))
        same(dev.snapshot(), before, "after the refused calls")
        with pytest.raises(bl.BotlabHipError, match="status 2"):
            bl.ObstacleLayer(0, 5, ctx=gpu_ctx)
    finally:
        other.close()
        dev.close()
