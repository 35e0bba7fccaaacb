"""The model of the Rao-Blackwellized grid SLAM with scan-matched proposals (bl_rbslam_set_scan_matching, include/botlab_hip.h):
rb_slam_model.RBSlamModel with step 3b between the action and the weighing of a moved update.  TEST INFRASTRUCTURE: the device must
agree with it bit for bit.

  3b. For every particle p: scan_match_model.match of the scan against self.maps[p] around the pose the action left.  If the best
      score reaches min_score and (di, dj, dk) != (0, 0, 0) the particle takes the matched pose; otherwise its pose stays bit for
      bit.  utime and parent pose are untouched.  Steps 4-6 then run on the new pose.
The per-particle (di, dj, dk, score, score_centre, ties, accepted) of the last matched update are kept in self.match.

window_path() restates the host's choice between the staged window (0) and the direct read (1) from the header's rule, and
window_of() the window of one particle, for the tests' conditions on their inputs."""
import ctypes as C
import math

import numpy as np

import adaptive_model as am
import rb_slam_model as rbm
import scan_match_model as smm

MAX_N, MAX_NTHETA, MAX_RAYS = 8, 16, 4096           # BL_RBSLAM_MATCH_MAX_N, _MAX_NTHETA, _MAX_RAYS
WINDOW_BYTES = 120 * 1024                           # BL_RBSLAM_MATCH_WINDOW_BYTES
MATCH_FIELDS = ("di", "dj", "dk", "score", "score_centre", "ties", "accepted")
F32 = np.float32


def check_params(nx, ny, ntheta, dtheta):
    return 0 <= nx <= MAX_N and 0 <= ny <= MAX_N and 0 <= ntheta <= MAX_NTHETA and bool(F32(dtheta) > 0)


def reach_cells(scan, max_range, cpm):
    """ceilf(longest valid range * cells_per_meter) in float; 0 without a valid ray."""
    ranges, _ = smm.valid_rays(scan.ranges, scan.thetas, max_range)
    if len(ranges) == 0:
        return 0
    return int(math.ceil(F32(ranges.max() * F32(cpm))))


def window_path(scan, max_range, cpm, W, H, nx, ny):
    """The header's rule: 0 iff the bound of the window fits BL_RBSLAM_MATCH_WINDOW_BYTES."""
    reach = reach_cells(scan, max_range, cpm)
    bw = min(2 * (reach + nx + 1) + 1 + 3, W)
    bh = min(2 * (reach + ny + 1) + 1, H)
    return 0 if ((bw + 3) & ~3) * bh <= WINDOW_BYTES else 1


def window_of(pose_xy, origin, cpm, reach, nx, ny, W, H):
    """(x0, y0, x1, y1) inclusive of one particle's window before and after clipping to the grid: (unclipped, clipped)."""
    sx, sy = smm.grid_position(pose_xy[0], pose_xy[1], origin, cpm)
    cx, cy = int(np.trunc(sx)), int(np.trunc(sy))
    raw = (cx - (reach + nx + 1), cy - (reach + ny + 1), cx + (reach + nx + 1), cy + (reach + ny + 1))
    return raw, (max(raw[0], 0), max(raw[1], 0), min(raw[2], W - 1), min(raw[3], H - 1))


class RBSlamMatchModel(rbm.RBSlamModel):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.matching = None
        self.match = None

    def set_scan_matching(self, nx=2, ny=2, ntheta=4, dtheta=math.radians(0.5), max_range=8.0, min_score=0):
        """None as nx: off.  A refused setting leaves the previous one in force and returns False."""
        if nx is None:
            self.matching = None
            return True
        if not check_params(nx, ny, ntheta, dtheta):
            return False
        self.matching = dict(nx=int(nx), ny=int(ny), ntheta=int(ntheta), dtheta=F32(dtheta), max_range=F32(max_range), min_score=int(min_score))
        return True

    def _match_all(self, scan):
        q = self.matching
        out = {f: np.zeros(self.P, np.int32) for f in MATCH_FIELDS}
        for p in range(self.P):
            c = self.parts[p]
            r = smm.match(self.maps[p], self.origin, self.mpc, self.cpm, scan.ranges, scan.thetas, (c["x"], c["y"], c["theta"]), q["nx"], q["ny"],
                          q["ntheta"], q["dtheta"], q["max_range"], q["min_score"])
            for f in MATCH_FIELDS:
                out[f][p] = r[f]
            if r["accepted"] and (r["di"], r["dj"], r["dk"]) != (0, 0, 0):
                self.parts["x"][p], self.parts["y"][p], self.parts["theta"][p] = r["x"], r["y"], r["theta"]
        self.match = out

    def update(self, odom, scan, rand_value, noise):
        """rb_slam_model.RBSlamModel.update with step 3b; the other steps are restated from it line for line."""
        if self.matching is None:
            return super().update(odom, scan, rand_value, noise)
        ranges, _ = smm.valid_rays(scan.ranges, scan.thetas, self.matching["max_range"])
        if len(ranges) > MAX_RAYS:
            raise ValueError("more than %d valid rays" % MAX_RAYS)      # refused before the ActionModel latches the odometry
        o, P = self.o, self.P
        op = o.pose(odom[0], odom[1], odom[2], utime=odom[3])
        moved = bool(o.lib.orc_action_update(self.action, C.byref(op)))
        resampled = False
        if moved:
            self.idx = np.arange(P, dtype=np.int32)
            if self.weighed and rbm.due(self.units, self.num, self.den):
                resampled = True
                self.idx = am.resample_integer(self.units, rand_value, P).astype(np.int32)
                self.parts = self.parts[self.idx].copy()
                self.maps = self.maps[self.idx].copy()
                self.cum[:] = 0
            nz = np.ascontiguousarray(noise, np.float32).reshape(P, 3)
            o.lib.orc_action_apply_noise(self.action, self.parts.ctypes.data, P, nz.ctypes.data)
            self.parts["utime"] = odom[3]
            self._match_all(scan)                                       # step 3b
            l = o.lidar(scan)
            raw = np.zeros(1, np.float64)
            for p in range(P):
                g = o.grid(self.maps[p], self.mpc, self.cpm, self.origin)
                o.lib.orc_likelihood(self.parts.ctypes.data + p * self.parts.dtype.itemsize, 1, C.byref(l), C.byref(g), raw.ctypes.data)
                h = int(round(2.0 * raw[0]))
                assert h == 2.0 * raw[0]
                self.like[p] = h
            self.cum = np.minimum(self.cum + self.like.astype(np.int64), rbm.SCORE_MAX)
            self.units = rbm.units_of(self.cum)
            self.weighed = True
            self.best = int(np.argmax(self.units))
            self.parts["weight"] = self.units.astype(np.float64) / float(int(self.units.sum(dtype=np.uint64)))
        if self.latched:
            for p in range(P):
                self._integrate(scan, p, self._pose_of(p, parent=True) if moved else self._pose_of(p))
        self.latched = True
        u = [int(v) for v in self.units]
        b = self.parts[self.best]
        return dict(moved=moved, resampled=resampled, best=self.best, pose=(float(b["x"]), float(b["y"]), float(b["theta"]), int(b["utime"])),
                    S=sum(u), Q=sum(v * v for v in u))


def started_model(orc, P, shape, mpc, cpm, origin, max_laser, hit, miss, num, den, start, spread=None):
    """rb_slam_model.started_model for the matching model."""
    mdl = RBSlamMatchModel(orc, P, shape, mpc, cpm, origin, max_laser, hit, miss, num, den)
    mdl.init_at_pose(start[0], start[1], start[2], 1000)
    if spread is not None:
        rng = np.random.default_rng(spread)
        p = mdl.parts.copy()
        p["x"] += rng.normal(0, 0.01, P).astype(np.float32); p["y"] += rng.normal(0, 0.01, P).astype(np.float32)
        p["theta"] += rng.normal(0, 0.01, P).astype(np.float32)
        p["p_x"], p["p_y"], p["p_theta"] = p["x"], p["y"], p["theta"]
        mdl.set_particles(p)
    return mdl
