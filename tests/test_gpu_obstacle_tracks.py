"""The obstacle tracks on the device (bl_obstracks_*, botlab_amd/csrc/bl_obstracks.hip) against their model
(tests/obstacle_tracks_model.py), value for value after every step of a script: the slots, the blobs, the label of every live cell,
the stats, and the composed grid after every compose."""
import numpy as np
import pytest

import botlab_amd as bl
from botlab_amd import synth
import helpers
import obstacle_tracks_model as tm
import test_obstacle_tracks_model_cpu as cpu

pytestmark = pytest.mark.gpu
F32 = np.float32


class Device:
    """A script's map, layer and tracker on the device."""

    def __init__(self, ctx, script):
        w, h = script.shape
        self.script = script
        self.params = dict(script.params)
        self.grid = bl.OccupancyGrid.from_cells(script.cells, script.origin, script.mpc, cellsPerMeter=script.cpm, ctx=ctx)
        self.out = bl.OccupancyGrid.from_cells(np.zeros_like(script.cells), (F32(7.0), F32(7.0)), script.mpc, cellsPerMeter=script.cpm, ctx=ctx)
        self.out2 = bl.OccupancyGrid.from_cells(np.zeros_like(script.cells), (F32(7.0), F32(7.0)), script.mpc, cellsPerMeter=script.cpm, ctx=ctx)
        self.layer = bl.ObstacleLayer(w, h, ctx=ctx, **script.layer)
        self.tracker = bl.ObstacleTracker(self.layer, **self.params)

    def step(self, st):
        """(outcome, composed grid or None); outcome "ok", "arg" or "state"."""
        composed = None
        try:
            if st[0] == "layer":
                self.layer.upload(st[1], st[2], st[3])
            elif st[0] == "scan":
                self.layer.update(self.grid, bl.LidarScan(st[1], st[2], np.zeros(len(st[1]), np.int64)), bl.make_pose(*st[3]))
            elif st[0] == "layer_reset":
                self.layer.reset()
            elif st[0] == "update":
                self.tracker.update()
            elif st[0] == "compose":
                self.tracker.compose(self.grid, self.out, horizon=st[1], robot_cell=st[2], keep_clear=st[3])
                assert (self.out.mpc, self.out.cpm, self.out.origin) == (self.grid.mpc, self.grid.cpm, self.grid.origin)
                composed = self.out.cells()
            elif st[0] == "params":
                p = dict(self.params, **st[1])
                self.tracker.setParams(**p)
                self.params = p
            elif st[0] == "reset":
                self.tracker.reset()
            elif st[0] == "upload":
                self.tracker.upload(st[1], st[2], st[3], st[4])
            elif st[0] == "roundtrip":
                slots, state = self.tracker.download()
                self.tracker.upload(slots, state["n"], state["next_id"], state["fresh"])
            else:
                raise AssertionError(st[0])
        except bl.BotlabHipError as e:
            return {"status 2": "arg", "status 4": "state"}[[k for k in ("status 2", "status 4") if k in str(e)][0]], None
        return "ok", composed

    def snapshot(self):
        return dict(tracks=self.tracker.tracks(), blobs=self.tracker.blobs(), labels=self.tracker.labels(), stats=self.tracker.stats(),
                    live=self.layer.live_cells())

    def close(self):
        for x in (self.tracker, self.layer, self.out2, self.out, self.grid):
            x.close()


def same_records(got, exp, where):
    assert got.shape == exp.shape, (where, got.shape, exp.shape)
    for name in exp.dtype.names:
        bad = np.flatnonzero(got[name] != exp[name])
        assert len(bad) == 0, (where, name, len(bad), int(bad[0]), got[name][bad[0]], exp[name][bad[0]])


def same(got, exp, where):
    assert got["stats"] == exp["stats"], (where, got["stats"], exp["stats"])
    same_records(got["tracks"], exp["tracks"], (where, "tracks"))
    same_records(got["blobs"], exp["blobs"], (where, "blobs"))
    for k in ("labels", "live"):
        assert got[k].dtype == exp[k].dtype and got[k].shape == exp[k].shape, (where, k, got[k].shape, exp[k].shape)
        assert np.array_equal(got[k], exp[k]), (where, k)


def run_both(ctx, script, model):
    """The script on the device beside the model's results: every step's outcome and snapshot equal, every composed grid equal."""
    dev = Device(ctx, script)
    try:
        for k, st in enumerate(script.steps):
            res, composed = dev.step(st)
            assert res == model[k][0], (k, st[0], res, model[k][0])
            if st[0] != "layer" or k == len(script.steps) - 1:
                same(dev.snapshot(), model[k][1], (k, st[0]))
            if composed is not None:
                exp = model[k][1]["composed"]
                bad = np.flatnonzero(composed.ravel() != exp.ravel())
                assert len(bad) == 0, (k, st, len(bad), int(bad[0]), composed.ravel()[bad[0]], exp.ravel()[bad[0]])
                if st[1] == 0:                          # horizon 0: the layer's own compose, byte for byte
                    dev.layer.compose(dev.grid, dev.out2)
                    assert np.array_equal(dev.out2.cells(), composed)
    finally:
        dev.close()


@pytest.mark.parametrize("w,h", cpu.SIZES)
@pytest.mark.parametrize("name", [n for n, _ in cpu.ALL])
def test_script_equals_the_model(gpu_ctx, name, w, h):
    script, model, _ = cpu.model_of(name, w, h)
    run_both(gpu_ctx, script, model)


@pytest.mark.parametrize("w,h", cpu.SIZES)
def test_reversed_rays_give_the_same_output(gpu_ctx, w, h):
    for script in cpu.reversed_scan_scripts(w, h):
        run_both(gpu_ctx, script, cpu.run_model(script))


def test_the_most_live_cells_and_one_more(gpu_ctx):
    script = cpu.large_script()
    run_both(gpu_ctx, script, cpu.run_model(script))


def moving_box_script(maps):
    """The shipped 200 x 200 map and a 4 x 4 box that the map does not know, moving 0.6 cell per update for 40 updates."""
    m = maps["obstacle_slam_10mx10m_5cm"]
    cells = m["cells"]
    s = cpu.Script(200, 200, cells=cells, layer=dict(max_range=5.0, min_hits=1, ttl_scans=2, tol_cells=1), confirm_hits=3, gate_cells=3)
    s.origin, s.mpc, s.cpm = m["origin"], m["mpc"], helpers.CPM_DEFAULT
    base = np.where(cells > 0, 127, -127).astype(np.int8)
    pose = (-0.75, 0.2, 0.0)
    free = np.argwhere(cells[80:120, 60:100] < 0)
    by, bx = free[len(free) // 2] + (80, 60)
    for k in range(40):
        truth = base.copy()
        x = bx - 12 + int(np.floor(0.6 * k))
        truth[by - 2:by + 2, x:x + 4] = 127
        scan = synth.raycast_scan(truth, m["origin"], 0.05, pose, pose, 1000 * k, max_range=5.0)
        s.add("scan", scan.ranges, scan.thetas, tuple(F32(v) for v in pose))
        s.add("update")
    s.add("compose", 8, (0, 0), -1)
    return s


def test_shipped_map_a_moving_box_keeps_one_id(gpu_ctx, maps):
    script = moving_box_script(maps)
    model = cpu.run_model(script)
    ids = []
    for st, (res, snap) in zip(script.steps, model):
        if st[0] == "update":
            conf = snap["tracks"][(snap["tracks"]["flags"] & tm.CONFIRMED) != 0]
            ids.append(set(int(i) for i in conf["id"]))
    first = next(k for k, i in enumerate(ids) if i)
    print("the box: confirmed at update", first, "ids", sorted(set().union(*ids)), "last velocity",
          [(int(t["vx"]), int(t["vy"])) for t in model[-2][1]["tracks"]])
    assert all(i == ids[first] and len(i) == 1 for i in ids[first:]), ids
    run_both(gpu_ctx, script, model)


def test_refusals_that_need_no_script(gpu_ctx):
    ctx = gpu_ctx
    layer = bl.ObstacleLayer(37, 23, ctx=ctx)
    other = bl.ObstacleLayer(38, 23, ctx=ctx)
    tr = bl.ObstacleTracker(layer)
    try:
        with pytest.raises(bl.BotlabHipError, match="status 4"):
            tr.lastDeviceMs()
        tr.layer = other
        with pytest.raises(bl.BotlabHipError, match="status 2"):
            tr.update()
        tr.layer = layer
        tr.update()
        assert tr.stats()["live_cells"] == 0 and len(tr.tracks()) == 0 and len(tr.blobs()) == 0 and len(tr.labels()) == 0
        with pytest.raises(bl.BotlabHipError, match="status 2"):
            bl.ObstacleTracker(layer, min_cells=5, max_cells=4)
        x, y, vx, vy = bl.track_to_metric(dict(px=256 * 10 + 128, py=1024, vx=-128, vy=64), type("G", (), dict(origin=(-1.0, -2.0), mpc=0.05)), 0.1)
        assert (x, y, vx, vy) == tm.track_metric(dict(px=256 * 10 + 128, py=1024, vx=-128, vy=64), (-1.0, -2.0), 0.05, 0.1)
    finally:
        tr.close()
        other.close()
        layer.close()
