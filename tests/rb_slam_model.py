"""The model of the Rao-Blackwellized grid SLAM (bl_rbslam_*, include/botlab_hip.h), built from the reference's per-particle entry
points in the CPU oracle: orc_action_update, orc_action_apply_noise, orc_likelihood on one particle with its own grid, and
OracleMapping.  TEST INFRASTRUCTURE: the device must agree with it bit for bit.

One update(odometry, scan, rand_value, noise):
  1. Moved?  ActionModel::updateAction on the odometry (orc_action_update).
  2. If moved and a resampling is DUE: low-variance resampling by the library's integer-prefix rule, adaptive_model.resample_integer
     with M = P on the weight units u; a child takes its source's pose, parent pose AND map; all cumulative scores reset to 0.
  3. If moved, action: applyAction per particle with the given noise (orc_action_apply_noise); the parent pose becomes the old pose,
     the pose's utime becomes the odometry's.
  4. If moved, weigh: h_p = 2 * SensorModel::likelihood of the scan for particle p against its own map (orc_likelihood; an exact
     integer), the moving scan interpolated between parent pose and pose.  c_p = min(c_p + h_p, SCORE_MAX), u_p = max(1000 c_p, 2).
  5. Best particle: the largest u_p, ties to the lowest index.
  6. Map: every particle's map receives Mapping::updateMap(scan, pose_p, map_p) with previousPose_ = parent_pose_p: a fresh
     OracleMapping per particle and step, primed with the parent pose (the oracle's mapper cannot be cloned; its first update only
     latches the pose and changes no cell).  The very first update of a run latches and changes no cell.  Not moved: steps 2-5 are
     skipped and the mapper is primed with pose_p itself -- literally OracleMapping.update(scan, pose_p) twice, the first on a
     scratch grid.
Resampling is DUE iff den * S^2 <= num * P * Q in exact integers, S = sum u, Q = sum u^2 over the units of the last weighing; nothing
is due before the first weighing.
A moved update whose odometry utime equals the poses' utime needs no rule of the model's own: the oracle's interpolate_pose_by_time
returns the end pose when both utimes are equal, which is the header's "equal utimes: the pose itself".

Helpers for the tests of the edges (tests/test_rb_slam_edges_cpu.py): watermark() marks a map with its particle's index, ray_cells()
and window_box() give the window of an update, window_tiles() cuts it by k_rb_map's rule and launch_tiles() restates the host's
gridDim.y of bl_rbslam_update.  None of them takes part in update()."""
import ctypes as C
import math

import numpy as np

import adaptive_model as am
import oracle_lib

SCORE_MAX = 1 << 33
STDS = (0.05, 0.005, 0.05)                  # ActionModel::update's rot1Std, transStd, rot2Std


def units_of(cum):
    return np.maximum(1000 * np.asarray(cum, dtype=np.int64), 2).astype(np.uint64)


def due(units, num, den):
    u = [int(v) for v in units]
    S, Q = sum(u), sum(v * v for v in u)
    return den * S * S <= num * len(u) * Q


def watermark(p, n):
    """n int8 values that name particle p (p < 2^14): two cells hold its index, the others a pattern seeded by it."""
    v = ((np.arange(n, dtype=np.int64) * (2 * int(p) + 1) + 37 * int(p)) % 251 - 125).astype(np.int8)
    v[0], v[1] = int(p) & 127, int(p) >> 7
    return v


def set_watermarks(maps, block):
    """Writes watermark(p) into maps[p][block] for every p; block: a pair of slices no ray may reach."""
    for p in range(len(maps)):
        shape = maps[p][block].shape
        maps[p][block] = watermark(p, shape[0] * shape[1]).reshape(shape)


def watermark_owner(cells, block):
    b = cells[block].ravel()
    p = int(b[0]) | (int(b[1]) << 7)
    return p if np.array_equal(b, watermark(p, b.size)) else -1


def ray_cells(orc, scan, begin, end, origin, cpm, max_laser):
    """(x0, y0, x1, y1) int cells of the rays Mapping::updateMap traces (range <= max_laser), from the oracle's MovingLaserScan;
    the cell arithmetic is mapping.cpp:45-49 in float32."""
    rays = orc.moving_scan(scan, begin, end)
    rays = rays[rays[:, 2] <= np.float32(max_laser)]
    cpm = np.float32(cpm)
    sx = ((rays[:, 0].astype(np.float64) - np.float64(np.float32(origin[0]))) * np.float64(cpm)).astype(np.float32)
    sy = ((rays[:, 1].astype(np.float64) - np.float64(np.float32(origin[1]))) * np.float64(cpm)).astype(np.float32)
    ex = (rays[:, 2] * np.cos(rays[:, 3]).astype(np.float32) * cpm + sx).astype(np.float32)
    ey = (rays[:, 2] * np.sin(rays[:, 3]).astype(np.float32) * cpm + sy).astype(np.float32)
    return np.stack([np.trunc(sx), np.trunc(sy), np.trunc(ex), np.trunc(ey)], axis=1).astype(np.int64)


def window_box(cells, W, H):
    """k_rb_map's window: the bounding box of all start and end cells, clipped to the grid, dword-aligned when W % 4 == 0.
    (x0, y0, x1, y1) inclusive, or None when nothing falls into the grid."""
    if len(cells) == 0:
        return None
    x0, x1 = max(int(min(cells[:, 0].min(), cells[:, 2].min())), 0), min(int(max(cells[:, 0].max(), cells[:, 2].max())), W - 1)
    y0, y1 = max(int(min(cells[:, 1].min(), cells[:, 3].min())), 0), min(int(max(cells[:, 1].max(), cells[:, 3].max())), H - 1)
    if x1 < x0 or y1 < y0:
        return None
    if W % 4 == 0:
        x0, x1 = x0 & ~3, x1 | 3
    return x0, y0, x1, y1


MAP_COUNTERS, MAP_TILE_W = 20480, 256       # RB_MAP_COUNTERS, RB_MAP_TILE_W (bl_rbslam.hip)


def window_tiles(box):
    """(ntx, nty) of k_rb_map's cut: tiles of min(ww, 256) columns and min(wh, 20480 // tw) rows."""
    ww, wh = box[2] - box[0] + 1, box[3] - box[1] + 1
    tw = min(ww, MAP_TILE_W)
    th = min(wh, MAP_COUNTERS // tw)
    return -(-ww // tw), -(-wh // th)


def launch_tiles(scan, max_laser, cpm, W, H):
    """gridDim.y of k_rb_map as bl_rbslam_update sizes it: the tiles of a square window of 2 * ceil(reach * cpm) + 8 cells, reach =
    min(largest kept range of the scan, max_laser), clipped to the grid; between 1 and 64."""
    kept = scan.ranges[scan.ranges > np.float32(0.15)]
    reach = min(np.float32(kept.max()) if len(kept) else np.float32(0.0), np.float32(max_laser))
    side = 2 * int(math.ceil(np.float32(reach * np.float32(cpm)))) + 8
    ww, wh = min(side, W), min(side, H)
    tw = min(ww, MAP_TILE_W)
    th = max(min(MAP_COUNTERS // max(tw, 1), wh), 1)
    return max(1, min(64, -(-ww // tw) * -(-wh // th)))


def started_model(orc, P, shape, mpc, cpm, origin, max_laser, hit, miss, num, den, start, spread=None):
    """A model initialised at the pose `start` (utime 1000); spread: the seed of distinct start poses, 0.01 apart in x, y and theta."""
    mdl = RBSlamModel(orc, P, shape, mpc, cpm, origin, max_laser, hit, miss, num, den)
    mdl.init_at_pose(start[0], start[1], start[2], 1000)
    if spread is not None:
        rng = np.random.default_rng(spread)
        p = mdl.parts.copy()
        p["x"] += rng.normal(0, 0.01, P).astype(np.float32); p["y"] += rng.normal(0, 0.01, P).astype(np.float32)
        p["theta"] += rng.normal(0, 0.01, P).astype(np.float32)
        p["p_x"], p["p_y"], p["p_theta"] = p["x"], p["y"], p["theta"]
        mdl.set_particles(p)
    return mdl


class RBSlamModel:
    def __init__(self, orc, P, shape, mpc, cpm, origin, max_laser, hit, miss, num=1, den=2):
        self.o, self.P = orc, int(P)
        self.mpc, self.cpm, self.origin = np.float32(mpc), np.float32(cpm), origin
        self.max_laser, self.hit, self.miss = max_laser, hit, miss
        self.num, self.den = int(num), int(den)
        self.maps = np.zeros((self.P,) + tuple(shape), np.int8)
        self.scratch = np.zeros(shape, np.int8)
        self.parts = np.zeros(self.P, oracle_lib.PARTICLE_DTYPE)
        self.cum = np.zeros(self.P, np.int64)
        self.units = units_of(self.cum)
        self.weighed = False
        self.latched = False
        self.best = 0
        self.idx = np.arange(self.P, dtype=np.int32)
        self.like = np.zeros(self.P, np.int32)
        self.action = orc.lib.orc_action_create()
        self.probe = oracle_lib.OraclePF(orc, 2)          # a twin ActionModel whose rot1 / trans / rot2 can be read (draw_noise)

    def __del__(self):
        if getattr(self, "action", None):
            self.o.lib.orc_action_destroy(self.action)
            self.action = None

    def set_particles(self, parts, cum=None):
        self.parts = np.ascontiguousarray(parts).copy()
        self.cum = np.zeros(self.P, np.int64) if cum is None else np.asarray(cum, np.int64).copy()
        self.units = units_of(self.cum)
        self.weighed = cum is not None
        self.best = int(np.argmax(self.units))

    def init_at_pose(self, x, y, theta, utime):
        """Every particle at the pose (the device's own draw has no CPU counterpart; tests upload particles)."""
        p = np.zeros(self.P, oracle_lib.PARTICLE_DTYPE)
        p["x"], p["y"], p["theta"], p["utime"] = np.float32(x), np.float32(y), np.float32(theta), utime
        p["p_x"], p["p_y"], p["p_theta"], p["p_utime"] = p["x"], p["y"], p["theta"], utime
        p["weight"] = 1.0 / self.P
        self.set_particles(p)

    def _pose_of(self, p, parent=False):
        q = self.parts[p]
        if parent:
            return self.o.pose(q["p_x"], q["p_y"], q["p_theta"], utime=int(q["p_utime"]))
        return self.o.pose(q["x"], q["y"], q["theta"], utime=int(q["utime"]))

    def draw_noise(self, odom, rng, stds=STDS):
        """3 P samples of (rot1, trans, rot2) for the update that `odom` will cause: call BEFORE update() with the same odometry."""
        op = self.o.pose(odom[0], odom[1], odom[2], utime=odom[3])
        self.probe.update_action_only(op, np.zeros(6, np.float32))
        st = (C.c_double * 3)()
        mv = C.c_int()
        self.o.lib.orc_pf_action_state(self.probe.h, st, C.byref(mv))
        noise = np.empty((self.P, 3), np.float32)
        for j in range(3):
            noise[:, j] = (st[j] + stds[j] * rng.standard_normal(self.P)).astype(np.float32)
        return noise

    def _integrate(self, scan, p, begin):
        om = oracle_lib.OracleMapping(self.o, self.max_laser, self.hit, self.miss)
        om.update(scan, begin, self.scratch, self.mpc, self.cpm, self.origin)     # latches `begin`; changes no cell
        om.update(scan, self._pose_of(p), self.maps[p], self.mpc, self.cpm, self.origin)

    def update(self, odom, scan, rand_value, noise):
        """odom: (x, y, theta, utime).  Returns dict(moved, resampled, best, pose, S, Q)."""
        o, P = self.o, self.P
        op = o.pose(odom[0], odom[1], odom[2], utime=odom[3])
        moved = bool(o.lib.orc_action_update(self.action, C.byref(op)))
        resampled = False
        if moved:
            self.idx = np.arange(P, dtype=np.int32)
            if self.weighed and due(self.units, self.num, self.den):
                resampled = True
                self.idx = am.resample_integer(self.units, rand_value, P).astype(np.int32)
                self.parts = self.parts[self.idx].copy()
                self.maps = self.maps[self.idx].copy()
                self.cum[:] = 0
            nz = np.ascontiguousarray(noise, np.float32).reshape(P, 3)
            o.lib.orc_action_apply_noise(self.action, self.parts.ctypes.data, P, nz.ctypes.data)
            self.parts["utime"] = odom[3]
            l = o.lidar(scan)
            raw = np.zeros(1, np.float64)
            for p in range(P):
                g = o.grid(self.maps[p], self.mpc, self.cpm, self.origin)
                o.lib.orc_likelihood(self.parts.ctypes.data + p * self.parts.dtype.itemsize, 1, C.byref(l), C.byref(g), raw.ctypes.data)
                h = int(round(2.0 * raw[0]))
                assert h == 2.0 * raw[0]
                self.like[p] = h
            self.cum = np.minimum(self.cum + self.like.astype(np.int64), SCORE_MAX)
            self.units = units_of(self.cum)
            self.weighed = True
            self.best = int(np.argmax(self.units))           # the first of equals
            self.parts["weight"] = self.units.astype(np.float64) / float(int(self.units.sum(dtype=np.uint64)))
        if self.latched:
            for p in range(P):
                self._integrate(scan, p, self._pose_of(p, parent=True) if moved else self._pose_of(p))
        self.latched = True
        u = [int(v) for v in self.units]
        b = self.parts[self.best]
        return dict(moved=moved, resampled=resampled, best=self.best, pose=(float(b["x"]), float(b["y"]), float(b["theta"]), int(b["utime"])),
                    S=sum(u), Q=sum(v * v for v in u))
