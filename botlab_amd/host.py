"""Host-side mirror of the reference's C++ surfaces for the hot path, over the C ABI of libbotlab_hip.so.

Same names, argument meaning and error behaviour as the reference classes (the C++ drop-in with identical signatures
lives in include/botlab/; this module is what the parity tests and bench.py drive):

  OccupancyGrid          src/slam/occupancy_grid.hpp:51-209
  Mapping                src/slam/mapping.hpp:25-34
  ParticleFilter         src/slam/particle_filter.hpp:38-77
  ObstacleDistanceGrid   src/planning/obstacle_distance_grid.hpp:28-96
  search_for_path        src/planning/astar.hpp:58-61
  MotionPlanner          src/planning/motion_planner.hpp:89-130 (setMap / planPath / isValidGoal / setParams)

All arithmetic runs in the HIP library; nothing here computes a result on the CPU.
"""
import ctypes as C
import math

import numpy as np

from . import _capi
from ._capi import Lidar, Particle, Pose, SearchParams, check

_libc = C.CDLL(None)
_libc.rand.restype = C.c_int

PARTICLE_DTYPE = np.dtype([("utime", "<i8"), ("x", "<f4"), ("y", "<f4"), ("theta", "<f4"), ("_pad0", "<f4"),
                           ("p_utime", "<i8"), ("p_x", "<f4"), ("p_y", "<f4"), ("p_theta", "<f4"), ("_pad1", "<f4"),
                           ("weight", "<f8")])
POSE_DTYPE = np.dtype([("utime", "<i8"), ("x", "<f4"), ("y", "<f4"), ("theta", "<f4"), ("_pad", "<f4")])
assert PARTICLE_DTYPE.itemsize == 56 and POSE_DTYPE.itemsize == 24


def make_pose(x=0.0, y=0.0, theta=0.0, utime=0):
    return Pose(int(utime), float(np.float32(x)), float(np.float32(y)), float(np.float32(theta)))


class LidarScan:
    """lidar_t (lcmtypes/lidar_t.lcm): utime, ranges[], thetas[], times[]."""

    def __init__(self, ranges, thetas, times, utime=0):
        self.ranges = np.ascontiguousarray(ranges, dtype=np.float32)
        self.thetas = np.ascontiguousarray(thetas, dtype=np.float32)
        self.times = np.ascontiguousarray(times, dtype=np.int64)
        assert self.ranges.shape == self.thetas.shape == self.times.shape and self.ranges.ndim == 1
        self.utime = int(utime)
        self.num_ranges = int(self.ranges.size)

    def as_c(self):
        return Lidar(self.utime, self.num_ranges, self.ranges.ctypes.data_as(C.POINTER(C.c_float)),
                     self.thetas.ctypes.data_as(C.POINTER(C.c_float)), self.times.ctypes.data_as(C.POINTER(C.c_int64)),
                     None)


class Context:
    """One HIP stream's worth of state on one device (bl_ctx)."""

    def __init__(self, device=0, stream=None):
        self.lib = _capi.load()
        h = C.c_void_p()
        check(self.lib.bl_ctx_create(int(device), C.c_void_p(stream) if stream else None, C.byref(h)))
        self.h = h
        self.device = device

    def scanPrefetch(self, scan):
        """Hands the NEXT lidar scan over early: the next map kernel of this context copies it to the device beside its own
        work, and the update that later brings the same scan launches no fetch kernel (bl_scan_prefetch)."""
        c = scan.as_c()
        check(self.lib.bl_scan_prefetch(self.h, C.byref(c)))

    def sync(self):
        check(self.lib.bl_ctx_sync(self.h))

    def timing_enable(self, on=True, kernels=None):
        """kernels: iterable of BL_K_* ids to time (default: all)."""
        flag = 0 if not on else (1 if kernels is None else sum(1 << k for k in kernels))
        if flag == 1 and kernels is not None:      # only kernel 0 requested: bit 0 alone is spelled 1 | (1 << 31)
            flag = 1 | (1 << 30)
        check(self.lib.bl_ctx_timing_enable(self.h, flag))

    def timing_stride(self, every):
        """Time only every `every`-th launch of each enabled kernel."""
        check(self.lib.bl_ctx_timing_stride(self.h, int(every)))

    def timing_reset(self):
        check(self.lib.bl_ctx_timing_reset(self.h))

    def timing_get(self, kernel_id):
        ms, n = C.c_double(), C.c_int64()
        check(self.lib.bl_ctx_timing_get(self.h, kernel_id, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def close(self):
        if self.h:
            self.lib.bl_ctx_destroy(self.h)
            self.h = None


_default_ctx = None


def default_context():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


class OccupancyGrid:
    """Device-resident int8 log-odds grid (occupancy_grid.hpp).  Float members follow the reference's float32
    arithmetic (occupancy_grid.cpp:19-36)."""

    def __init__(self, widthInMeters=None, heightInMeters=None, metersPerCell=0.05, ctx=None, _raw=None):
        self.ctx = ctx or default_context()
        lib = self.ctx.lib
        if _raw is not None:
            width, height, mpc, cpm, ox, oy = _raw
        else:
            assert widthInMeters > 0 and heightInMeters > 0            # occupancy_grid.cpp:25-28
            mpc = np.float32(metersPerCell)
            assert mpc <= np.float32(widthInMeters) and mpc <= np.float32(heightInMeters)
            cpm = np.float32(1.0) / mpc
            width = int(np.float32(widthInMeters) * cpm)
            height = int(np.float32(heightInMeters) * cpm)
            ox = -np.float32(widthInMeters) / np.float32(2.0)
            oy = -np.float32(heightInMeters) / np.float32(2.0)
        self.width, self.height = int(width), int(height)
        self.mpc, self.cpm = np.float32(mpc), np.float32(cpm)
        self.origin = (np.float32(ox), np.float32(oy))
        h = C.c_void_p()
        check(lib.bl_grid_create(self.ctx.h, self.width, self.height, self.mpc, self.cpm, self.origin[0], self.origin[1],
                                 C.byref(h)))
        self.h = h

    @classmethod
    def from_cells(cls, cells, origin, metersPerCell, cellsPerMeter=None, ctx=None):
        """loadFromFile / fromLCM equivalent: cells is an (H, W) int8 array.  loadFromFile keeps the cellsPerMeter_ of
        the default constructor (20.0f, occupancy_grid.cpp:9-16,138-175); fromLCM sets 1.0f/mpc (:99-108)."""
        cells = np.ascontiguousarray(cells, dtype=np.int8)
        hgt, wid = cells.shape
        mpc = np.float32(metersPerCell)
        cpm = np.float32(cellsPerMeter) if cellsPerMeter is not None else np.float32(1.0) / mpc
        g = cls(ctx=ctx, _raw=(wid, hgt, mpc, cpm, np.float32(origin[0]), np.float32(origin[1])))
        g.upload(cells)
        return g

    # accessors (occupancy_grid.hpp:80-91)
    def widthInCells(self): return self.width
    def heightInCells(self): return self.height
    def metersPerCell(self): return self.mpc
    def cellsPerMeter(self): return self.cpm
    def originInGlobalFrame(self): return self.origin
    def isCellInGrid(self, x, y): return 0 <= x < self.width and 0 <= y < self.height

    def upload(self, cells):
        cells = np.ascontiguousarray(cells, dtype=np.int8)
        assert cells.shape == (self.height, self.width)
        check(self.ctx.lib.bl_grid_upload(self.h, cells.ctypes.data))

    def cells(self):
        out = np.empty((self.height, self.width), dtype=np.int8)
        check(self.ctx.lib.bl_grid_download(self.h, out.ctypes.data))
        return out

    def reset(self):
        check(self.ctx.lib.bl_grid_reset(self.h))

    def logOdds(self, x, y):
        """Host read of one cell (downloads the grid; test convenience only)."""
        return int(self.cells()[y, x]) if self.isCellInGrid(x, y) else 0

    def saveToFile(self, filename):
        """ASCII .map format (occupancy_grid.cpp:111-136)."""
        c = self.cells()
        with open(filename, "w") as f:
            f.write(f"{_fmt(self.origin[0])} {_fmt(self.origin[1])} {self.width} {self.height} {_fmt(self.mpc)}\n")
            for y in range(self.height):
                f.write(" ".join(str(int(v)) for v in c[y]) + " \n")
        return True

    @classmethod
    def loadFromFile(cls, filename, ctx=None):
        with open(filename) as f:
            tok = f.read().split()
        ox, oy, w, h, mpc = np.float32(tok[0]), np.float32(tok[1]), int(tok[2]), int(tok[3]), np.float32(tok[4])
        cells = np.array(tok[5:5 + w * h], dtype=np.int64).astype(np.int8).reshape(h, w)
        return cls.from_cells(cells, (ox, oy), mpc, cellsPerMeter=np.float32(1.0 / np.float64(np.float32(0.05))), ctx=ctx)

    def close(self):
        if self.h:
            if getattr(self, "owns_handle", True):                     # (a LikelihoodField's grid belongs to the field)
                self.ctx.lib.bl_grid_destroy(self.h)
            self.h = None


def _fmt(v):
    return np.format_float_positional(np.float32(v), precision=6, unique=True, trim="-")


class Mapping:
    """Mapping(maxLaserDistance, hitOdds, missOdds).updateMap(scan, pose, map) (mapping.hpp:25-34)."""

    def __init__(self, maxLaserDistance, hitOdds, missOdds, ctx=None):
        self.ctx = ctx or default_context()
        h = C.c_void_p()
        check(self.ctx.lib.bl_mapping_create(self.ctx.h, np.float32(maxLaserDistance), int(hitOdds), int(missOdds), C.byref(h)))
        self.h = h

    def updateMap(self, scan, pose, grid):
        ls = scan.as_c()
        check(self.ctx.lib.bl_mapping_update(self.h, C.byref(ls), C.byref(pose), grid.h))

    def updateMapDevicePose(self, scan, d_pose_ptr, pose_utime, grid):
        ls = scan.as_c()
        check(self.ctx.lib.bl_mapping_update_dev_pose(self.h, C.byref(ls), d_pose_ptr, int(pose_utime), grid.h))

    def updateMapFinishingFilter(self, scan, pf, pose_utime, grid):
        """pf.updateEnd(want_pose=False) + updateMapDevicePose(scan, pf.poseDevicePtr(), ...) in ONE launch: the end of the
        filter update (pose estimate + weight prefix) rides in the map kernel (bl_mapping_update_finishing_pf)."""
        ls = scan.as_c()
        check(self.ctx.lib.bl_mapping_update_finishing_pf(self.h, C.byref(ls), pf.h, int(pose_utime), grid.h))

    def close(self):
        if self.h:
            self.ctx.lib.bl_mapping_destroy(self.h)
            self.h = None


def spread_stds(s):
    """(position std, heading std) of a spread: sqrt of the larger eigenvalue of [[var_x, cov_xy], [cov_xy, var_y]] and
    sqrt(-2 ln R), as OccupancyGridSLAMT's convergence test (include/botlab/slam_driver.hpp) forms them."""
    a, b, c = s["var_x"], s["cov_xy"], s["var_y"]
    h = 0.5 * (a + c)
    lam = h + math.sqrt(max(0.0, 0.25 * (a - c) * (a - c) + b * b))
    r = s["theta_resultant"]
    th = math.sqrt(-2.0 * math.log(r)) if r > 0.0 else math.inf
    return math.sqrt(max(0.0, lam)), th


# kidnapped-robot recovery defaults (ParticleFilter.setRecovery): AMCL's averaging rates; ratio and max_fraction calibrated on the
# CPU reference filter (tests/test_recovery_model_cpu.py)
RECOVERY_ALPHA_SLOW, RECOVERY_ALPHA_FAST = 0.001, 0.1
RECOVERY_RATIO, RECOVERY_MAX_FRACTION = 0.9, 0.1

# adaptive particle count defaults (ParticleFilter.setAdaptive): AMCL's epsilon, the 0.99 quantile, the reference's 200 particles as
# the floor; bins calibrated on the CPU reference filter (tests/test_adaptive_model_cpu.py)
ADAPTIVE_MIN_PARTICLES, ADAPTIVE_EPSILON, ADAPTIVE_Z = 200, 0.01, 2.326
ADAPTIVE_BIN_XY, ADAPTIVE_BIN_THETA = 0.1, math.radians(10.0)


class ParticleFilter:
    """ParticleFilter(numParticles) (particle_filter.hpp:38-77).  shard=(lo, hi) keeps only those particles' private
    state on this device (botlab_amd.sharded drives the exchange)."""

    def __init__(self, numParticles, ctx=None, shard=None):
        assert numParticles > 1                                         # particle_filter.cpp:11
        self.ctx = ctx or default_context()
        self.N = int(numParticles)
        self.lo, self.hi = shard if shard else (0, self.N)
        h = C.c_void_p()
        check(self.ctx.lib.bl_pf_create(self.ctx.h, self.N, self.lo, self.hi, C.byref(h)))
        self.h = h
        self._adaptive_used = False       # the particle count may differ from N once adaptive mode has been on

    def _counts(self):
        """(active, next): particles in the current record, particles the next resampling update draws."""
        if not self._adaptive_used:
            return self.hi - self.lo, self.hi - self.lo
        s = self.adaptiveState()
        return s["active"], s["next"]

    def initializeFilterAtPose(self, pose, seed=None):
        if seed is None:                                                # reference: std::random_device
            seed = int.from_bytes(np.random.bytes(8), "little")
        check(self.ctx.lib.bl_pf_init_at_pose(self.h, C.byref(pose), C.c_uint64(seed)))

    def initializeFilterUniformly(self, grid, distances=None, minDistance=0.0, utime=0, seed=None):
        """Global localization: particles spread uniformly over the free cells of `grid` (log-odds < 0) and, with an
        ObstacleDistanceGrid of the same shape, only where its distance is > minDistance (bl_pf_init_uniform)."""
        if seed is None:
            seed = int.from_bytes(np.random.bytes(8), "little")
        check(self.ctx.lib.bl_pf_init_uniform(self.h, grid.h, distances.h if distances is not None else None,
                                              np.float32(minDistance), int(utime), C.c_uint64(seed)))

    def spread(self):
        """Spread of the posterior (bl_pf_spread): dict of n_eff, mean_x, mean_y, var_x, var_y, cov_xy, theta_resultant,
        units_sum and units_sq (exact integers), and the derived position_std (square root of the covariance's larger
        eigenvalue, metres) and theta_std (circular standard deviation sqrt(-2 ln R), radians)."""
        out = _capi.PfSpread()
        check(self.ctx.lib.bl_pf_spread(self.h, C.byref(out)))
        d = {f: getattr(out, f) for f, _ in _capi.PfSpread._fields_ if not f.startswith("units_sq")}
        d["units_sq"] = (int(out.units_sq_hi) << 64) | int(out.units_sq_lo)
        d["position_std"], d["theta_std"] = spread_stds(d)
        return d

    def clusters(self, bin_xy, theta_bins, max_clusters, labels=False):
        """Pose hypotheses (bl_pf_clusters): the connected components of the occupied (bin_xy, bin_xy, 2 pi / theta_bins) bins,
        heaviest first.  Returns a dict of num_clusters, units_sum, active, params and clusters: a list of min(num_clusters,
        max_clusters) dicts of count, units, the exact sums sx, sy, sxx, syy, sxy, sc, ss (Python integers) and anchor (ix, iy, it);
        with labels=True also labels, one int32 per particle: the rank of its cluster, -1 beyond max_clusters.  bin_xy,
        theta_bins and any threshold on a cluster's share are untuned knobs."""
        p = _capi.PfClusterParams(float(bin_xy), int(theta_bins), int(max_clusters))
        out = _capi.PfClusters()
        lab = np.empty(self._counts()[0], np.int32) if labels else None
        check(self.ctx.lib.bl_pf_clusters(self.h, C.byref(p), C.byref(out), lab.ctypes.data if labels else None))
        cl = []
        for k in range(min(int(out.num_clusters), int(max_clusters))):
            c = out.clusters[k]
            e = {"count": int(c.count), "units": int(c.units), "anchor": (int(c.anchor_ix), int(c.anchor_iy), int(c.anchor_it))}
            e.update({n: getattr(c, n).value() for n in _capi.PF_CLUSTER_SUMS})
            cl.append(e)
        d = {"num_clusters": int(out.num_clusters), "units_sum": int(out.units_sum), "active": int(out.active), "clusters": cl,
             "params": (float(bin_xy), int(theta_bins), int(max_clusters)), "raw": out}
        if labels:
            d["labels"] = lab
        return d

    @staticmethod
    def cluster_pose(result, k=0):
        """bl_pf_cluster_pose of cluster k of a clusters() result: dict of share, mean_x, mean_y, var_x, var_y, cov_xy, theta,
        theta_resultant and the derived position_std and theta_std (spread()'s two formulas on the cluster's own moments); None for
        a cluster of 0 units or a rank the result does not hold."""
        if not 0 <= k < len(result["clusters"]):
            return None
        p = _capi.PfClusterParams(*result["params"])
        out = _capi.PfClusterPose()
        if not _capi.load().bl_pf_cluster_pose(C.byref(result["raw"].clusters[k]), C.c_uint64(result["units_sum"]), C.byref(p), C.byref(out)):
            return None
        d = {f: getattr(out, f) for f, _ in _capi.PfClusterPose._fields_}
        # (a resultant rounded above 1 -- every heading in one direction -- is a deviation of 0)
        d["position_std"], d["theta_std"] = spread_stds(dict(d, theta_resultant=min(1.0, d["theta_resultant"])))
        return d

    def setRecovery(self, grid, distances=None, minDistance=0.0, alphaSlow=RECOVERY_ALPHA_SLOW, alphaFast=RECOVERY_ALPHA_FAST,
                    ratio=RECOVERY_RATIO, maxFraction=RECOVERY_MAX_FRACTION, seed=None):
        """Kidnapped-robot recovery (augmented MCL, bl_pf_set_recovery): while the fast average of the mean particle weight falls below
        ratio times the slow one, up to maxFraction of the resampled particles are replaced by poses drawn uniformly over the free
        cells of `grid` as it stands now (log-odds < 0 and, with an ObstacleDistanceGrid, distance > minDistance).  grid=None turns
        recovery off."""
        if grid is None:
            check(self.ctx.lib.bl_pf_set_recovery(self.h, None, None, None))
            return
        if seed is None:
            seed = int.from_bytes(np.random.bytes(8), "little")
        p = _capi.PfRecoveryParams(float(alphaSlow), float(alphaFast), float(ratio), float(maxFraction), float(np.float32(minDistance)),
                                   int(seed) & 0xFFFFFFFFFFFFFFFF)
        check(self.ctx.lib.bl_pf_set_recovery(self.h, grid.h, distances.h if distances is not None else None, C.byref(p)))

    def recoveryState(self):
        """The recovery tracker (bl_pf_recovery_state): dict of w_slow, w_fast, w_avg, p_inject, updates, primed, injected_last,
        injected_total (all zero while recovery is off)."""
        out = _capi.PfRecoveryState()
        check(self.ctx.lib.bl_pf_recovery_state(self.h, C.byref(out)))
        return {f: getattr(out, f) for f, _ in _capi.PfRecoveryState._fields_ if f != "pad"}

    def setAdaptive(self, minParticles=ADAPTIVE_MIN_PARTICLES, epsilon=ADAPTIVE_EPSILON, z=ADAPTIVE_Z, binXY=ADAPTIVE_BIN_XY,
                    binTheta=ADAPTIVE_BIN_THETA):
        """Adaptive particle count (KLD-sampling, bl_pf_set_adaptive): every resampling update draws between minParticles and N
        particles, as many as the number of occupied (binXY, binXY, binTheta) bins of the resampled set needs for a KLD error
        below epsilon with quantile z.  minParticles=None turns it off (the next resampling update draws N again)."""
        if minParticles is None:
            check(self.ctx.lib.bl_pf_set_adaptive(self.h, None))
            return
        p = _capi.PfAdaptiveParams(int(minParticles), 0, float(epsilon), float(z), float(binXY), float(binTheta))
        check(self.ctx.lib.bl_pf_set_adaptive(self.h, C.byref(p)))
        self._adaptive_used = True

    def adaptiveState(self):
        """bl_pf_adaptive_state: dict of active, next, bins, k_sat, counts."""
        out = _capi.PfAdaptiveState()
        check(self.ctx.lib.bl_pf_adaptive_state(self.h, C.byref(out)))
        return {f: getattr(out, f) for f, _ in _capi.PfAdaptiveState._fields_}

    def numParticles(self):
        """Particles in the current record (N, or the adaptive count)."""
        return self._counts()[0]

    def setParticles(self, particles, units=None):
        """particles: structured array (PARTICLE_DTYPE) of all N particles."""
        p = np.ascontiguousarray(particles)
        assert p.dtype.itemsize == 56 and p.size == self.N
        u = None
        if units is not None:
            u = np.ascontiguousarray(units, dtype=np.uint32)
            assert u.size == self.N
        check(self.ctx.lib.bl_pf_set_particles(self.h, p.ctypes.data, u.ctypes.data if u is not None else None))

    def setNoiseSeed(self, seed):
        check(self.ctx.lib.bl_pf_set_noise_seed(self.h, C.c_uint64(seed)))

    def updateFilter(self, odometry, laser, grid, rand_value=None, noise=None, want_pose=True):
        """pose_xyt_t updateFilter(odometry, laser, map).  rand_value defaults to libc rand(), as the reference's
        resampler calls it (particle_filter.cpp:92); noise (3*N float32) replaces the Philox action noise."""
        if rand_value is None:
            rand_value = _libc.rand()
        ls = laser.as_c()
        nz = None
        if noise is not None:
            nz = np.ascontiguousarray(noise, dtype=np.float32)
            assert nz.size == 3 * (self._counts()[1] if self._adaptive_used else self.N)
        out = Pose()
        check(self.ctx.lib.bl_pf_update(self.h, C.byref(odometry), C.byref(ls), grid.h, int(rand_value),
                                        nz.ctypes.data if nz is not None else None, C.byref(out) if want_pose else None))
        return out if want_pose else None

    def updateBegin(self, odometry, laser, grid, rand_value, noise=None):
        ls = laser.as_c()
        nz = None
        if noise is not None:
            nz = np.ascontiguousarray(noise, dtype=np.float32)
        moved = C.c_int()
        check(self.ctx.lib.bl_pf_update_begin(self.h, C.byref(odometry), C.byref(ls), grid.h, int(rand_value),
                                              nz.ctypes.data if nz is not None else None, C.byref(moved)))
        return bool(moved.value)

    def updateEnd(self, want_pose=True):
        out = Pose()
        check(self.ctx.lib.bl_pf_update_end(self.h, C.byref(out) if want_pose else None))
        return out if want_pose else None

    def updateFilterActionOnly(self, odometry, noise=None):
        nz = None
        if noise is not None:
            nz = np.ascontiguousarray(noise, dtype=np.float32)
        out = Pose()
        check(self.ctx.lib.bl_pf_update_action_only(self.h, C.byref(odometry), nz.ctypes.data if nz is not None else None,
                                                    C.byref(out)))
        return out

    def poseEstimate(self):
        out = Pose()
        check(self.ctx.lib.bl_pf_pose_estimate(self.h, C.byref(out)))
        return out

    def poseDevicePtr(self):
        return self.ctx.lib.bl_pf_pose_device_ptr(self.h)

    def estimatePosteriorPose(self):
        """estimatePosteriorPose(posterior_) of the particles as they stand (particle_filter.cpp:144-160)."""
        out = Pose()
        check(self.ctx.lib.bl_pf_estimate_posterior_pose(self.h, C.byref(out)))
        return out

    def reweigh_beam(self, beam, grid, scan):
        """The beam model's weights in place of the current ones (BeamModel.reweigh): the beam-weighted posterior pose."""
        return beam.reweigh(self, grid, scan)

    def reweigh_beam_table(self, beam, table, scan):
        """The same with the expected ranges looked up in a built RangeTable (BeamModel.reweigh_table)."""
        return beam.reweigh_table(self, table, scan)

    def reweigh_beam_leap(self, beam, clearance, scan):
        """The same with the expected ranges found by leaps over a built ClearanceGrid (BeamModel.reweigh_leap)."""
        return beam.reweigh_leap(self, clearance, scan)

    def setStrictResampling(self, on=True):
        """Resample against the reference's own sequentially rounded cumulative weight (bl_pf_set_strict_resampling)."""
        check(self.ctx.lib.bl_pf_set_strict_resampling(self.h, 1 if on else 0))

    def debugResample(self, rand_value):
        """Source index of every output particle of resamplePosteriorDistribution for this rand() value (particle_filter.cpp:84-103)."""
        idx = np.empty(self._counts()[1] if self._adaptive_used else self.N, np.int32)
        check(self.ctx.lib.bl_pf_debug_resample(self.h, int(rand_value), idx.ctypes.data))
        return idx

    def debugUniformRuns(self):
        """Runs of the equal-weight cumulative in force for the next resampling (0: the weights are not known to be equal)."""
        n = C.c_int()
        check(self.ctx.lib.bl_pf_debug_uniform_runs(self.h, C.byref(n)))
        return n.value

    def debugEstimateStats(self):
        """Per axis (x, then y): generic replays, their phases, table replays, gaps walked the slow way."""
        out = np.zeros(8, np.uint32)
        check(self.ctx.lib.bl_pf_debug_estimate_stats(self.h, out.ctypes.data))
        return [int(v) for v in out]

    def debugLookahead(self):
        """(map updates that ran ahead of the exact pose, those of them that ran again) since the filter was created."""
        out = np.zeros(2, np.uint32)
        check(self.ctx.lib.bl_pf_debug_lookahead(self.h, out.ctypes.data))
        return int(out[0]), int(out[1])

    def particles(self):
        """particles_t.particles of the local shard as a structured array."""
        out = np.zeros(self._counts()[0], dtype=PARTICLE_DTYPE)
        check(self.ctx.lib.bl_pf_get_particles(self.h, out.ctypes.data))
        return out

    def debugEnable(self, on=True):
        check(self.ctx.lib.bl_pf_debug_enable(self.h, 1 if on else 0))

    def debugLast(self):
        n = self._counts()[0]
        idx = np.empty(n, np.int32)
        like = np.empty(n, np.int32)
        check(self.ctx.lib.bl_pf_debug_last(self.h, idx.ctypes.data, like.ctypes.data))
        return idx, like

    def close(self):
        if self.h:
            self.ctx.lib.bl_pf_destroy(self.h)
            self.h = None


def prior_from_sigmas(sigma_x, sigma_y, rho, sigma_theta, score_per_nat, meters_per_cell, dtheta):
    """The four coefficients of a scan match's motion prior (a_xx, a_xy, a_yy, a_tt) from a Gaussian on the motion: standard
    deviations sigma_x, sigma_y (metres, correlation rho, |rho| < 1) and sigma_theta (radians), all > 0 (inf: no prior on that
    axis); score_per_nat is the number of score units one nat of log-likelihood is worth.  The rule, in double arithmetic, the
    same as botlab_hip::scan_match_prior_from_sigmas: the Gaussian's information matrix in cells and heading steps
    (s_x = sigma_x / meters_per_cell, s_y likewise, s_t = sigma_theta / dtheta, q = 1 - rho^2: 1 / (q s_x^2), -rho / (q s_x s_y),
    1 / (q s_y^2), 1 / s_t^2) times 256 score_per_nat / 2, each rounded to nearest as floor(v + 0.5) and clamped to
    [0, 32767] (a_xy to [-32767, 32767]; NaN gives 0); then |a_xy| is lowered to floor(sqrt(a_xx a_yy)) if it exceeds it, so
    that the clamped form is still never negative."""
    sigma_x, sigma_y, rho, sigma_theta = float(sigma_x), float(sigma_y), float(rho), float(sigma_theta)
    if not (sigma_x > 0 and sigma_y > 0 and sigma_theta > 0 and abs(rho) < 1 and float(score_per_nat) >= 0):
        raise ValueError("prior_from_sigmas: sigmas must be > 0, |rho| < 1, score_per_nat >= 0")
    k = 128.0 * float(score_per_nat)
    sx, sy, st = sigma_x / float(meters_per_cell), sigma_y / float(meters_per_cell), sigma_theta / float(dtheta)
    q = 1.0 - rho * rho

    def coeff(v, lo):
        if v != v:
            return 0
        return int(math.floor(min(max(v, lo), 32767.0) + 0.5))     # the bounds are integers: clamping first rounds the same
    a_xx, a_yy = coeff(k * (1.0 / (q * sx * sx)), 0.0), coeff(k * (1.0 / (q * sy * sy)), 0.0)
    a_xy = coeff(k * (-rho / (q * sx * sy)), -32767.0)
    a_tt = coeff(k * (1.0 / (st * st)), 0.0)
    if a_xy * a_xy > a_xx * a_yy:
        a_xy = int(math.copysign(math.isqrt(a_xx * a_yy), a_xy))
    return a_xx, a_xy, a_yy, a_tt


class ScanMatcher:
    """Correlative scan matcher (bl_scanmatch_*, include/botlab_hip.h): the pose of a scan against the map from a bounded window of
    whole-cell shifts and heading steps around a centre pose, without odometry.  Off the filter's path: it reads the map only."""

    def __init__(self, ctx=None):
        self.ctx = ctx or default_context()
        h = C.c_void_p()
        check(self.ctx.lib.bl_scanmatch_create(self.ctx.h, C.byref(h)))
        self.h = h
        self._shape = None

    def match(self, scan, centre, grid, nx=4, ny=4, ntheta=12, dtheta=math.radians(0.5), max_range=8.0, min_score=0,
              keep_volume=False):
        """The best (di, dj, dk) of the window as a _capi.ScanMatchResult (pose, di, dj, dk, score, score_centre, ties, rays_used,
        accepted)."""
        ls = scan.as_c()
        params = _capi.ScanMatchParams(int(nx), int(ny), int(ntheta), float(np.float32(dtheta)), float(np.float32(max_range)),
                                       int(min_score), 1 if keep_volume else 0)
        res = _capi.ScanMatchResult()
        self._shape = None                 # a refused match keeps no volume either (the library forgets it as well)
        check(self.ctx.lib.bl_scanmatch_match(self.h, grid.h, C.byref(ls), C.byref(centre), C.byref(params), C.byref(res)))
        if keep_volume:
            self._shape = (2 * int(ntheta) + 1, 2 * int(ny) + 1, 2 * int(nx) + 1)
        return res

    def match_prior(self, scan, centre, grid, prior=(0, 0, 0, 0), half_life=None, nx=4, ny=4, ntheta=12, dtheta=math.radians(0.5),
                    max_range=8.0, min_score=0, keep_volume=False):
        """bl_scanmatch_match_prior: the match under a motion prior (a_xx, a_xy, a_yy, a_tt), e.g. from prior_from_sigmas.
        Returns (result, moments): a _capi.ScanMatchResult and, when half_life is given (1 .. 2^20), a _capi.ScanMatchMoments
        (the ten weighted sums, best_obj, pen_best, the sub-cell fractions; .covariance(mpc, dtheta), .refined_pose(...)), else
        None.  With half_life (or keep_volume) volume() then returns the objective volume."""
        ls = scan.as_c()
        params = _capi.ScanMatchParams(int(nx), int(ny), int(ntheta), float(np.float32(dtheta)), float(np.float32(max_range)),
                                       int(min_score), 1 if keep_volume else 0)
        want = half_life is not None
        pr = _capi.ScanMatchPrior(int(prior[0]), int(prior[1]), int(prior[2]), int(prior[3]), int(half_life) if want else 0,
                                  1 if want else 0)
        res = _capi.ScanMatchResult()
        mom = _capi.ScanMatchMoments() if want else None
        shape = self._shape                # a refused match with a prior changes nothing
        self._shape = None
        try:
            check(self.ctx.lib.bl_scanmatch_match_prior(self.h, grid.h, C.byref(ls), C.byref(centre), C.byref(params), C.byref(pr),
                                                        C.byref(res), C.byref(mom) if want else None))
        except _capi.BotlabHipError as e:
            if "status 2" in str(e):
                self._shape = shape
            raise
        if keep_volume or want:
            self._shape = (2 * int(ntheta) + 1, 2 * int(ny) + 1, 2 * int(nx) + 1)
        return res, mom

    def volume(self):
        """Scores [dk + ntheta][dj + ny][di + nx] of the last match (int32); it must have been run with keep_volume=True."""
        if self._shape is None:
            raise _capi.BotlabHipError("ScanMatcher.volume: the last match did not keep its score volume (status 4)")
        out = np.empty(self._shape, dtype=np.int32)
        check(self.ctx.lib.bl_scanmatch_volume(self.h, out.ctypes.data_as(C.c_void_p)))
        return out

    def match_wide(self, scan, centre, grid, nx, ny, ntheta, dtheta=math.radians(1.0), max_range=8.0, min_score=0, block_log2=0,
                   exhaustive=False):
        """bl_scanmatch_match_wide: the same definition over windows up to the whole map (nx, ny <= 4096, ntheta <= 720), exact,
        by scoring coarse blocks of 2^block_log2 cells a side first (0: the library chooses) and only the surviving blocks
        exactly; exhaustive=True scores every candidate.  Returns a _capi.ScanMatchResult."""
        ls = scan.as_c()
        params = _capi.ScanMatchWideParams(int(nx), int(ny), int(ntheta), float(np.float32(dtheta)), float(np.float32(max_range)),
                                           int(min_score), int(block_log2), 1 if exhaustive else 0)
        res = _capi.ScanMatchResult()
        check(self.ctx.lib.bl_scanmatch_match_wide(self.h, grid.h, C.byref(ls), C.byref(centre), C.byref(params), C.byref(res)))
        return res

    def wide_stats(self):
        """_capi.ScanMatchWideStats of the last wide match: candidates, blocks, blocks_kept, candidates_scored, block_log2, path."""
        st = _capi.ScanMatchWideStats()
        check(self.ctx.lib.bl_scanmatch_wide_stats(self.h, C.byref(st)))
        return st

    def debugPath(self):
        """0: the last match staged its map window in LDS; 1: it read the grid directly; -1: no match yet."""
        return int(self.ctx.lib.bl_scanmatch_debug_path(self.h))

    def close(self):
        if self.h:
            self.ctx.lib.bl_scanmatch_destroy(self.h)
            self.h = None


class ObstacleDistanceGrid:
    """ObstacleDistanceGrid().setDistances(map); operator()(x, y) (obstacle_distance_grid.hpp:28-96)."""

    def __init__(self, ctx=None, metric="l1", max_cells=64):
        """metric "l1": the reference's grid (0.1 per L1 cell), what the search reads.  metric "euclidean": the exact Euclidean
        transform in metres, capped at max_cells cells (bl_dist_create_euclidean), for the field, the local planner and the shortcut."""
        self.ctx = ctx or default_context()
        h = C.c_void_p()
        if metric == "l1":
            check(self.ctx.lib.bl_dist_create(self.ctx.h, C.byref(h)))
        elif metric == "euclidean":
            check(self.ctx.lib.bl_dist_create_euclidean(self.ctx.h, int(max_cells), C.byref(h)))
        else:
            raise ValueError("metric must be 'l1' or 'euclidean'")
        self.h = h
        self._host = None

    def setDistances(self, grid):
        check(self.ctx.lib.bl_dist_set_distances(self.h, grid.h))
        self._host = None

    def metric(self):
        """("l1", 0) or ("euclidean", max_cells) (bl_dist_metric)."""
        m, r = C.c_int(), C.c_int()
        check(self.ctx.lib.bl_dist_metric(self.h, C.byref(m), C.byref(r)))
        return ("euclidean" if m.value == _capi.BL_DIST_EUCLIDEAN else "l1"), r.value

    def codes(self):
        """n(c) as uint16 (h, w): the L1 distance in cells, or the capped squared Euclidean distance; 0xFFFF: the map has no source."""
        w, h = self.shape()
        out = np.empty((h, w), dtype=np.uint16)
        check(self.ctx.lib.bl_dist_download_codes(self.h, out.ctypes.data))
        return out

    def table(self):
        """The float table the codes index (bl_dist_table)."""
        n = C.c_int()
        check(self.ctx.lib.bl_dist_table(self.h, None, C.byref(n)))
        out = np.empty(n.value, dtype=np.float32)
        check(self.ctx.lib.bl_dist_table(self.h, out.ctypes.data, C.byref(n)))
        return out

    def forget(self):
        """The next setDistances transforms the whole map (bl_dist_forget)."""
        check(self.ctx.lib.bl_dist_forget(self.h))

    def stats(self):
        """How the transforms of this grid went out (bl_dist_debug_stats)."""
        v = (C.c_int64 * 6)()
        check(self.ctx.lib.bl_dist_debug_stats(self.h, v))
        return dict(incremental=v[0], full=v[1], unchanged=v[2], nothing=v[3], window=v[4], fallback=v[5])

    def bound(self):
        """(formed, D): the bound the next incremental transform dilates its window by (bl_dist_debug_bound)."""
        f, b = C.c_int(), C.c_uint()
        check(self.ctx.lib.bl_dist_debug_bound(self.h, C.byref(f), C.byref(b)))
        return bool(f.value), int(b.value)

    def fusedStats(self):
        """(gave_up, helped) of the one-launch whole-grid transform (bl_dist_debug_fused)."""
        v = (C.c_int64 * 2)()
        check(self.ctx.lib.bl_dist_debug_fused(self.h, v))
        return int(v[0]), int(v[1])

    def shape(self):
        w, h = C.c_int(), C.c_int()
        check(self.ctx.lib.bl_dist_shape(self.h, C.byref(w), C.byref(h)))
        return w.value, h.value

    def widthInCells(self): return self.shape()[0]
    def heightInCells(self): return self.shape()[1]

    def frame(self):
        v = [C.c_float() for _ in range(4)]
        check(self.ctx.lib.bl_dist_frame(self.h, *[C.byref(x) for x in v]))
        return tuple(np.float32(x.value) for x in v)      # mpc, cpm, ox, oy

    def cells(self):
        if self._host is None:
            w, h = self.shape()
            out = np.empty((h, w), dtype=np.float32)
            check(self.ctx.lib.bl_dist_download(self.h, out.ctypes.data))
            self._host = out
        return self._host

    def isCellInGrid(self, x, y):
        w, h = self.shape()
        return 0 <= x < w and 0 <= y < h

    def __call__(self, x, y):
        return self.cells()[y, x]

    def close(self):
        if self.h:
            self.ctx.lib.bl_dist_destroy(self.h)
            self.h = None


def search_for_path(start, goal, distances, params, return_stats=False, cap=1 << 20):
    """robot_path_t search_for_path(start, goal, distances, params) (astar.hpp:58-61).  Returns the list of poses
    (path_length == len(result); length 1 == no path)."""
    ctx = distances.ctx
    buf = (Pose * cap)()
    n = C.c_int()
    stats = (C.c_int64 * 2)()
    check(ctx.lib.bl_astar_search(ctx.h, distances.h, C.byref(start), C.byref(goal), C.byref(params), buf, cap, C.byref(n), stats))
    path = [Pose(p.utime, p.x, p.y, p.theta) for p in buf[:min(n.value, cap)]]
    if return_stats:
        return path, (stats[0], stats[1])
    return path


def search_for_path_begin(goal, distances, params, start=None, start_dev=None):
    """Asynchronous form: enqueue the search (start pose from the host, or read on the device from start_dev, e.g.
    ParticleFilter.poseDevicePtr()); fetch it with search_for_path_end."""
    ctx = distances.ctx
    if start_dev is not None:
        check(ctx.lib.bl_astar_search_async_dev_start(ctx.h, distances.h, start_dev, C.byref(goal), C.byref(params)))
    else:
        check(ctx.lib.bl_astar_search_async(ctx.h, distances.h, C.byref(start), C.byref(goal), C.byref(params)))


_path_bufs = {}


def search_for_path_end(distances, cap=4097, return_stats=False):
    ctx = distances.ctx
    buf = _path_bufs.get(cap)
    if buf is None:
        buf = _path_bufs[cap] = (Pose * cap)()
    n = C.c_int()
    stats = (C.c_int64 * 2)()
    check(ctx.lib.bl_astar_search_result(ctx.h, buf, cap, C.byref(n), stats))
    if n.value > cap:
        raise _capi.BotlabHipError(f"path of {n.value} poses does not fit the {cap}-pose buffer")
    path = [Pose(p.utime, p.x, p.y, p.theta) for p in buf[:n.value]]
    return (path, (stats[0], stats[1])) if return_stats else path


def search_for_path_batch(start, goals, distances, params, cap_each=4097, return_stats=False):
    """n independent search_for_path calls from one start, run concurrently on the device (bl_astar_search_batch).
    Returns a list of paths (each a list of poses)."""
    ctx = distances.ctx
    n = len(goals)
    g = (Pose * max(n, 1))(*goals)
    buf = (Pose * (max(n, 1) * cap_each))()
    lens = (C.c_int * max(n, 1))()
    stats = (C.c_int64 * (2 * max(n, 1)))()
    check(ctx.lib.bl_astar_search_batch(ctx.h, distances.h, C.byref(start), g, n, C.byref(params), buf, cap_each, lens, stats))
    paths = []
    for i in range(n):
        if lens[i] > cap_each:
            raise _capi.BotlabHipError(f"path {i} of {lens[i]} poses does not fit the {cap_each}-pose buffer")
        paths.append([Pose(p.utime, p.x, p.y, p.theta) for p in buf[i * cap_each:i * cap_each + lens[i]]])
    if return_stats:
        return paths, [(stats[2 * i], stats[2 * i + 1]) for i in range(n)]
    return paths


class Frontiers:
    """std::vector<frontier_t> (frontiers.hpp:17-20) as a library handle; .cells() gives the list of (n, 2) float32 arrays."""

    def __init__(self, ctx, h):
        self.ctx, self.h = ctx, h

    @classmethod
    def from_lists(cls, ctx, frontiers):
        offs = np.zeros(len(frontiers) + 1, np.int32)
        for k, f in enumerate(frontiers):
            offs[k + 1] = offs[k] + len(f)
        xy = np.ascontiguousarray(np.concatenate(frontiers) if len(frontiers) else np.zeros((0, 2)), dtype=np.float32)
        h = C.c_void_p()
        check(ctx.lib.bl_frontiers_from_host(offs.ctypes.data, len(frontiers), xy.ctypes.data, C.byref(h)))
        return cls(ctx, h)

    def __len__(self):
        return self.ctx.lib.bl_frontiers_count(self.h)

    def cells(self):
        n, tot = len(self), self.ctx.lib.bl_frontiers_total_cells(self.h)
        offs = np.zeros(n + 1, np.int32)
        xy = np.zeros((max(tot, 1), 2), np.float32)
        check(self.ctx.lib.bl_frontiers_get(self.h, offs.ctypes.data, xy.ctypes.data))
        return [xy[offs[k]:offs[k + 1]].copy() for k in range(n)]

    def stats(self):
        a, b = C.c_int(), C.c_int()
        check(self.ctx.lib.bl_frontiers_stats(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def sweep_kernel(self):
        """which kernels grew these frontiers (bl_frontiers_debug_sweep_kernel): 0 / 1 one workgroup (small / large grid),
        2 k_frontier_grow, 3 k_frontier_grow2"""
        return int(self.ctx.lib.bl_frontiers_debug_sweep_kernel(self.h))

    def close(self):
        if self.h:
            self.ctx.lib.bl_frontiers_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def find_map_frontiers(grid, robotPose, minFrontierLength=0.35):
    """find_map_frontiers (frontiers.hpp:34-36)."""
    h = C.c_void_p()
    check(grid.ctx.lib.bl_frontiers_find(grid.ctx.h, grid.h, C.byref(robotPose), float(minFrontierLength), C.byref(h)))
    return Frontiers(grid.ctx, h)


def plan_path_to_frontier(frontiers, robotPose, grid, planner, cap=1 << 16, return_info=False):
    """plan_path_to_frontier (frontiers.hpp:50-53).  `grid` is unused by the reference too; the planner's distance grid is."""
    ctx = planner.distances_.ctx
    if not isinstance(frontiers, Frontiers):
        frontiers = Frontiers.from_lists(ctx, frontiers)
    st = _capi.MotionPlannerState(planner.params_.robotRadius, planner.searchParams_, planner.num_frontiers, planner.prev_goal)
    buf = (Pose * cap)()
    n = C.c_int()
    goal = Pose()
    stats = (C.c_int64 * 3)()
    check(ctx.lib.bl_plan_path_to_frontier(ctx.h, frontiers.h, C.byref(robotPose), planner.distances_.h, C.byref(st), buf, cap,
                                           C.byref(n), C.byref(goal), stats))
    if n.value > cap:
        raise _capi.BotlabHipError(f"path of {n.value} poses does not fit the {cap}-pose buffer")
    path = [Pose(p.utime, p.x, p.y, p.theta) for p in buf[:n.value]]
    if return_info:
        return path, goal, (stats[0], stats[1], stats[2])
    return path


NAV_UNREACHED = 0xFFFFFFFF
NAV_OBSTACLE_GAIN = 50


def nav_params(searchParams, obstacle_gain=NAV_OBSTACLE_GAIN, reach_cells=0):
    """bl_navfield_params_t from a planner's SearchParams: the same three distances, the gain and the reach of a goal."""
    return _capi.NavFieldParams(searchParams.minDistanceToObstacle, searchParams.maxDistanceWithCost, searchParams.distanceCostExponent,
                                int(obstacle_gain), int(reach_cells))


class NavigationField:
    """The goal-rooted navigation field (bl_navfield_*, include/botlab_hip.h): the exact cost-to-go of every cell of a distance grid
    to a set of goal cells over 8-connected moves, and the cheapest paths read off it.  One compute answers every query against
    its goals."""

    def __init__(self, ctx=None):
        self.ctx = ctx or default_context()
        h = C.c_void_p()
        check(self.ctx.lib.bl_navfield_create(self.ctx.h, C.byref(h)))
        self.h = h
        self._dist = None

    def compute(self, distances, params, goal_cells):
        """goal_cells: (n, 2) integer cells (x, y).  `distances` must stay alive (and untransformed, for paths) while the field is used."""
        g = np.ascontiguousarray(np.asarray(goal_cells, dtype=np.int32).reshape(-1, 2))
        self._dist = distances
        check(self.ctx.lib.bl_navfield_compute(self.h, distances.h, C.byref(params), g.ctypes.data if len(g) else None, len(g)))

    def computeToPose(self, distances, params, goal):
        self._dist = distances
        check(self.ctx.lib.bl_navfield_compute_to_pose(self.h, distances.h, C.byref(params), C.byref(goal)))

    def paths(self, starts, cap_each=4097, raw=False):
        """One descent per start pose.  Returns (paths, labels, costs): paths as lists of Pose (raw=True: a (n, cap_each) POSE_DTYPE
        array and the lengths instead), the goal label each path reached (-1: none) and field(start)."""
        n = len(starts)
        s = (Pose * max(n, 1))(*starts)
        buf = np.zeros((max(n, 1), cap_each), dtype=POSE_DTYPE)
        lens = np.zeros(max(n, 1), np.int32)
        labels = np.zeros(max(n, 1), np.int32)
        costs = np.zeros(max(n, 1), np.uint32)
        check(self.ctx.lib.bl_navfield_paths(self.h, s, n, buf.ctypes.data, cap_each, lens.ctypes.data, labels.ctypes.data, costs.ctypes.data))
        if raw:                                          # lens[i] > cap_each: path i is cut off at cap_each poses
            return (buf[:n], lens[:n]), labels[:n], costs[:n]
        if n and int(lens[:n].max()) > cap_each:
            raise _capi.BotlabHipError(f"a path of {int(lens[:n].max())} poses does not fit the {cap_each}-pose buffer")
        out = [[Pose(int(p["utime"]), float(p["x"]), float(p["y"]), float(p["theta"])) for p in buf[i, :lens[i]]] for i in range(n)]
        return out, labels[:n], costs[:n]

    def gather(self, cells):
        q = np.ascontiguousarray(np.asarray(cells, dtype=np.int32).reshape(-1, 2))
        out = np.zeros(len(q), np.uint32)
        check(self.ctx.lib.bl_navfield_gather(self.h, q.ctypes.data if len(q) else None, len(q), out.ctypes.data if len(q) else None))
        return out

    def shape(self):
        w, h = C.c_int(), C.c_int()
        check(self.ctx.lib.bl_navfield_shape(self.h, C.byref(w), C.byref(h)))
        return w.value, h.value

    def cells(self):
        w, h = self.shape()
        out = np.empty((h, w), dtype=np.uint32)
        check(self.ctx.lib.bl_navfield_download(self.h, out.ctypes.data))
        return out

    def tables(self):
        """(traversable, penalty) per L1 distance n = 0 .. width + height."""
        n = C.c_int()
        check(self.ctx.lib.bl_navfield_tables(self.h, None, None, C.byref(n)))
        trav, pen = np.zeros(n.value, np.uint8), np.zeros(n.value, np.int32)
        check(self.ctx.lib.bl_navfield_tables(self.h, trav.ctypes.data, pen.ctypes.data, C.byref(n)))
        return trav, pen

    def stats(self):
        v = (C.c_int64 * 5)()
        check(self.ctx.lib.bl_navfield_stats(self.h, v))
        return dict(rounds=v[0], tile_sweeps=v[1], traversable=v[2], reached=v[3], goal_set=v[4])

    def close(self):
        if self.h:
            self.ctx.lib.bl_navfield_destroy(self.h)
            self.h = None


LOCALPLAN_REACHED, LOCALPLAN_OFF_FIELD, LOCALPLAN_BLOCKED = 1, 2, 4
LOCALPLAN_RESULT_DTYPE = np.dtype([("trans_v", "<f4"), ("angular_v", "<f4"), ("index", "<i4"), ("n_admissible", "<i4"), ("cost", "<i8"),
                                   ("flags", "<i4"), ("pad", "<i4")])
assert LOCALPLAN_RESULT_DTYPE.itemsize == 32


class LocalPlanner:
    """The local planner (bl_localplan_*, include/botlab_hip.h): the velocity command of the next control period, by rollout of every
    reachable (v, w) pair over a computed NavigationField.  A state is (pose, v, w): a Pose and the velocities the robot has now."""

    def __init__(self, ctx=None, **params):
        self.ctx = ctx or default_context()
        h = C.c_void_p()
        check(self.ctx.lib.bl_localplan_create(self.ctx.h, C.byref(h)))
        self.h = h
        self.params = None
        if params:
            self.set_params(**params)

    def set_params(self, v_min, v_max, w_max, acc_v, acc_w, dt_control, dt_sim, n_v, n_w, n_steps, w_field=1, w_heading=0, w_clear=0,
                   w_speed=0):
        p = _capi.LocalPlanParams(v_min, v_max, w_max, acc_v, acc_w, dt_control, dt_sim, int(n_v), int(n_w), int(n_steps), int(w_field),
                                  int(w_heading), int(w_clear), int(w_speed))
        check(self.ctx.lib.bl_localplan_set_params(self.h, C.byref(p)))
        self.params = p

    @staticmethod
    def _state(s):
        pose, v, w = s
        return _capi.LocalPlanState(pose, float(np.float32(v)), float(np.float32(w)))

    def _counts(self):
        if self.params is None:                              # the library's own refusal, with its message
            check(self.ctx.lib.bl_localplan_tables(self.h, C.byref(_capi.LocalPlanState()), None, None))
        return self.params.n_v, self.params.n_w, self.params.n_steps

    def commands(self, field, states):
        """One result per state, as a LOCALPLAN_RESULT_DTYPE array; all states in one launch sequence."""
        n = len(states)
        s = (_capi.LocalPlanState * max(n, 1))(*[self._state(q) for q in states])
        out = np.zeros(max(n, 1), dtype=LOCALPLAN_RESULT_DTYPE)
        check(self.ctx.lib.bl_localplan_commands(self.h, field.h, s, n, out.ctypes.data))
        return out[:n]

    def command(self, field, pose, v, w):
        """(trans_v, angular_v, flags) for one state: what a motion controller publishes as mbot_motor_command_t."""
        r = self.commands(field, [(pose, v, w)])[0]
        return float(r["trans_v"]), float(r["angular_v"]), int(r["flags"])

    def costs(self, field, state):
        """int64 [n_w, n_v]: the cost of every candidate of one state, INT64_MAX where it is inadmissible."""
        n_v, n_w, _ = self._counts()
        out = np.zeros((n_w, n_v), dtype=np.int64)
        check(self.ctx.lib.bl_localplan_debug_costs(self.h, field.h, C.byref(self._state(state)), out.ctypes.data))
        return out

    def rollout(self, field, state, c):
        """The n_steps poses of candidate c of one state, as a POSE_DTYPE array."""
        _, _, n_steps = self._counts()
        out = np.zeros(n_steps, dtype=POSE_DTYPE)
        check(self.ctx.lib.bl_localplan_debug_rollout(self.h, field.h, C.byref(self._state(state)), int(c), out.ctypes.data))
        return out

    def tables(self, state):
        """(v_i, w_j): the candidate tables of one state."""
        n_v, n_w, _ = self._counts()
        v, w = np.zeros(n_v, np.float32), np.zeros(n_w, np.float32)
        check(self.ctx.lib.bl_localplan_tables(self.h, C.byref(self._state(state)), v.ctypes.data, w.ctypes.data))
        return v, w

    def commands_moving(self, field, tracker, states, steps_per_update, margin_cells=0, lead_steps=0):
        """commands(field, states) with every rollout timed against the tracker's confirmed moving tracks: a candidate whose cell at
        step k lies in a track's box at step k is refused.  steps_per_update rollout steps of dt_sim make one tracker update;
        lead_steps of them have passed since the last one.  `field` is computed over tracker.composeStatic(...)."""
        n = len(states)
        s = (_capi.LocalPlanState * max(n, 1))(*[self._state(q) for q in states])
        m = _capi.LocalPlanMoving(int(steps_per_update), int(margin_cells), int(lead_steps), 0)
        out = np.zeros(max(n, 1), dtype=LOCALPLAN_RESULT_DTYPE)
        check(self.ctx.lib.bl_localplan_commands_moving(self.h, field.h, tracker.h, C.byref(m), s, n, out.ctypes.data))
        return out[:n]

    def command_moving(self, field, tracker, pose, v, w, steps_per_update, margin_cells=0, lead_steps=0):
        """(trans_v, angular_v, flags) for one state under the moving rule."""
        r = self.commands_moving(field, tracker, [(pose, v, w)], steps_per_update, margin_cells, lead_steps)[0]
        return float(r["trans_v"]), float(r["angular_v"]), int(r["flags"])

    def costs_moving(self, field, tracker, state, steps_per_update, margin_cells=0, lead_steps=0):
        """(int64 [n_w, n_v] costs under the moving rule, int32 [n_w, n_v] first_hit: the first step inside a moving box, 0: none)."""
        n_v, n_w, _ = self._counts()
        m = _capi.LocalPlanMoving(int(steps_per_update), int(margin_cells), int(lead_steps), 0)
        costs, first = np.zeros((n_w, n_v), dtype=np.int64), np.zeros((n_w, n_v), dtype=np.int32)
        check(self.ctx.lib.bl_localplan_debug_costs_moving(self.h, field.h, tracker.h, C.byref(m), C.byref(self._state(state)), costs.ctypes.data,
                                                           first.ctypes.data))
        return costs, first

    def debugPath(self):
        """0: the last launch staged the window in LDS; 1: it read the grids directly; -1 before the first."""
        return self.ctx.lib.bl_localplan_debug_path(self.h)

    def debugMovingPath(self):
        """Of the last moving call: 0 the boxes' table in LDS, 1 the boxes computed per step, 2 no used slot kept; -1 before the first."""
        return self.ctx.lib.bl_localplan_debug_moving_path(self.h)

    def lastDeviceMs(self):
        ms = C.c_float()
        check(self.ctx.lib.bl_localplan_last_device_ms(self.h, C.byref(ms)))
        return ms.value

    def close(self):
        if self.h:
            self.ctx.lib.bl_localplan_destroy(self.h)
            self.h = None


MPPI_FELL_BACK = 8
MPPI_RESULT_DTYPE = np.dtype([("trans_v", "<f4"), ("angular_v", "<f4"), ("index_best", "<i4"), ("n_admissible", "<i4"), ("cost_best", "<i8"),
                              ("cost_out", "<i8"), ("weight_sum", "<u8"), ("weight_sq_sum", "<u8"), ("flags", "<i4"), ("pad", "<i4")])
assert MPPI_RESULT_DTYPE.itemsize == 56


class MppiPlanner:
    """The sampling local planner (bl_mppi_*, include/botlab_hip.h): model-predictive path-integral control over a computed
    NavigationField.  K perturbed control sequences of T periods are rolled out and their softmin-weighted average is the new
    sequence; controls are int32 in units of 2^-16 (m/s, rad/s).  A state is (pose, v, w, tick, stream).  The planner holds one
    warm-start sequence for command() / advance(); plan() takes and returns sequences explicitly.  K, T, lambda, the noises and the
    weights are untuned knobs, and nothing here publishes the command."""

    def __init__(self, ctx=None, **params):
        self.ctx = ctx or default_context()
        h = C.c_void_p()
        check(self.ctx.lib.bl_mppi_create(self.ctx.h, C.byref(h)))
        self.h = h
        self.params = None
        self.seq = None                                      # int32 [T, 2]: the held nominal sequence
        self.tick = 0
        self.last = None                                     # the record of the last command()
        if params:
            self.set_params(**params)

    def set_params(self, v_min, v_max, w_max, acc_v, acc_w, dt_sim, noise_v, noise_w, n_samples, horizon, n_sub, lam, w_field=1, w_heading=0,
                   w_clear=0, seed=0):
        p = _capi.MppiParams(v_min, v_max, w_max, acc_v, acc_w, dt_sim, noise_v, noise_w, int(n_samples), int(horizon), int(n_sub), int(lam),
                             int(w_field), int(w_heading), int(w_clear), 0, int(seed))
        check(self.ctx.lib.bl_mppi_set_params(self.h, C.byref(p)))
        self.params = p
        self.seq = np.zeros((p.horizon, 2), np.int32)

    @staticmethod
    def _state(s):
        pose, v, w = s[0], s[1], s[2]
        tick, stream = (s[3], s[4]) if len(s) > 3 else (0, 0)
        return _capi.MppiState(_capi.LocalPlanState(pose, float(np.float32(v)), float(np.float32(w))), int(tick), int(stream))

    def _shape(self):
        if self.params is None:
            raise RuntimeError("MppiPlanner has no parameters (set_params first)")
        return self.params.n_samples, self.params.horizon, self.params.n_sub

    @staticmethod
    def _moving(tracker, moving):
        if tracker is None:
            return None, None
        steps_per_update, margin_cells, lead_steps = moving
        return tracker.h, C.byref(_capi.LocalPlanMoving(int(steps_per_update), int(margin_cells), int(lead_steps), 0))

    def plan(self, field, states, seq_in=None, tracker=None, moving=None):
        """(MPPI_RESULT_DTYPE [n], seq_out int32 [n, T, 2]) for n states (pose, v, w, tick, stream); seq_in int32 [n, T, 2] or None
        (zeros).  With a tracker, `moving` = (steps_per_update, margin_cells, lead_steps) times every rollout against its moving tracks."""
        n = len(states)
        T = self.params.horizon if self.params is not None else 1
        s = (_capi.MppiState * max(n, 1))(*[self._state(q) for q in states])
        out = np.zeros(max(n, 1), dtype=MPPI_RESULT_DTYPE)
        seq_out = np.zeros((max(n, 1), T, 2), np.int32)
        u = None
        if seq_in is not None:
            u = np.ascontiguousarray(seq_in, dtype=np.int32).reshape(n, T, 2)
        th, m = self._moving(tracker, moving)
        check(self.ctx.lib.bl_mppi_plan(self.h, field.h, th, m, s, n, u.ctypes.data if u is not None and n else None, seq_out.ctypes.data,
                                        out.ctypes.data))
        return out[:n], seq_out[:n]

    def command(self, field, pose, v, w, stream=0, tracker=None, moving=None):
        """(trans_v, angular_v, flags) for one state, warm-started from the held sequence; call advance() once the command is taken."""
        r, so = self.plan(field, [(pose, v, w, self.tick, stream)], self.seq[None], tracker, moving)
        self.last, self.seq = r[0], so[0].copy()
        return float(r[0]["trans_v"]), float(r[0]["angular_v"]), int(r[0]["flags"])

    def advance(self):
        """The next tick: the held sequence shifted by one period, its last control repeated; zeros after any flag but FELL_BACK."""
        flags = int(self.last["flags"]) if self.last is not None else 0
        if flags & ~MPPI_FELL_BACK:
            self.seq = np.zeros_like(self.seq)
        else:
            self.seq = np.concatenate([self.seq[1:], self.seq[-1:]], axis=0)
        self.tick += 1

    def debug_samples(self, field, state, seq_in=None, tracker=None, moving=None):
        """(costs int64 [K], first_hit int32 [K], seqs int32 [K, T, 2]) of one state's samples, INT64_MAX where inadmissible."""
        K, T, _ = self._shape()
        costs, first, seqs = np.zeros(K, np.int64), np.zeros(K, np.int32), np.zeros((K, T, 2), np.int32)
        u = np.ascontiguousarray(seq_in, dtype=np.int32).reshape(T, 2) if seq_in is not None else None
        th, m = self._moving(tracker, moving)
        check(self.ctx.lib.bl_mppi_debug_samples(self.h, field.h, th, m, C.byref(self._state(state)), u.ctypes.data if u is not None else None,
                                                 costs.ctypes.data, first.ctypes.data, seqs.ctypes.data))
        return costs, first, seqs

    def rollout(self, field, state, seq=None):
        """The T * n_sub poses of a sequence int32 [T, 2] (None: zeros), as a POSE_DTYPE array."""
        _, T, n_sub = self._shape()
        out = np.zeros(T * n_sub, dtype=POSE_DTYPE)
        u = np.ascontiguousarray(seq, dtype=np.int32).reshape(T, 2) if seq is not None else None
        check(self.ctx.lib.bl_mppi_debug_rollout(self.h, field.h, C.byref(self._state(state)), u.ctypes.data if u is not None else None,
                                                 out.ctypes.data))
        return out

    def weightTable(self):
        out = np.zeros(257, np.uint32)
        self.ctx.lib.bl_mppi_weight_table(out.ctypes.data)
        return out

    def debugPath(self):
        """0: the last rollout launch staged the window in LDS; 1: it read the grids directly; -1 before the first."""
        return self.ctx.lib.bl_mppi_debug_path(self.h)

    def lastDeviceMs(self):
        ms = C.c_float()
        check(self.ctx.lib.bl_mppi_last_device_ms(self.h, C.byref(ms)))
        return ms.value

    def close(self):
        if self.h:
            self.ctx.lib.bl_mppi_destroy(self.h)
            self.h = None


class PathShortcut:
    """Path shortcutting (bl_shortcut_*, include/botlab_hip.h): any-angle waypoints from grid paths -- all-pairs line of sight over a
    path's cells and the cheapest chain of segments over the visibility graph, in exact integers."""

    MAX_POINTS, MAX_PATHS, WINDOW_BYTES = 8192, 4096, 64 * 1024

    def __init__(self, ctx=None, **params):
        self.ctx = ctx or default_context()
        h = C.c_void_p()
        check(self.ctx.lib.bl_shortcut_create(self.ctx.h, C.byref(h)))
        self.h = h
        self.params = None
        if params:
            self.set_params(**params)

    def set_params(self, clearance, max_span=64, waypoint_cost=1024):
        p = _capi.ShortcutParams(float(clearance), int(max_span), int(waypoint_cost))
        check(self.ctx.lib.bl_shortcut_set_params(self.h, C.byref(p)))
        self.params = p

    def cells(self, distances, paths):
        """paths: a list of (m, 2) integer arrays of cells (x, y).  Returns (keeps, costs): per path the kept indices (int32) and
        costs as an (P, 2) int64 array: the shortened path's cost and the input path's."""
        n = len(paths)
        arrs = [np.asarray(q, dtype=np.int32).reshape(-1, 2) for q in paths]
        offs = np.zeros(n + 1, np.int32)
        offs[1:] = np.cumsum([len(q) for q in arrs], dtype=np.int64)
        xy = np.ascontiguousarray(np.concatenate(arrs) if n else np.zeros((0, 2), np.int32), dtype=np.int32)
        keep = np.zeros(max(len(xy), 1), np.int32)
        counts = np.zeros(max(n, 1), np.int32)
        cost = np.zeros((max(n, 1), 2), np.int64)
        check(self.ctx.lib.bl_shortcut_cells(self.h, distances.h, xy.ctypes.data, offs.ctypes.data, n, keep.ctypes.data, counts.ctypes.data,
                                             cost.ctypes.data))
        return [keep[offs[k]:offs[k] + counts[k]].copy() for k in range(n)], cost[:n]

    def shortcut(self, distances, path, return_cost=False):
        """One path of Pose: the kept poses, headings along the segments."""
        out, costs = self.poses(distances, [path])
        return (out[0], costs[0]) if return_cost else out[0]

    def poses(self, distances, paths):
        """paths: a list of lists of Pose.  Returns (shortened paths as lists of Pose, (P, 2) int64 costs)."""
        n = len(paths)
        cap = max([len(q) for q in paths] + [1])
        buf = np.zeros((max(n, 1), cap), dtype=POSE_DTYPE)
        for k, q in enumerate(paths):
            for i, p in enumerate(q):
                buf[k, i] = (p.utime, p.x, p.y, p.theta, 0)
        lens = np.array([len(q) for q in paths] + ([] if n else [0]), np.int32)
        out = np.zeros_like(buf)
        out_lens = np.zeros(max(n, 1), np.int32)
        cost = np.zeros((max(n, 1), 2), np.int64)
        check(self.ctx.lib.bl_shortcut_poses(self.h, distances.h, buf.ctypes.data, cap, lens.ctypes.data, n, out.ctypes.data, out_lens.ctypes.data,
                                             cost.ctypes.data))
        res = [[Pose(int(p["utime"]), float(p["x"]), float(p["y"]), float(p["theta"])) for p in out[k, :out_lens[k]]] for k in range(n)]
        return res, cost[:n]

    def visible(self, distances, cells):
        """uint8 [m, m] of one path of m <= 512 cells: [j, i] = 1 iff (i, j) is an edge."""
        xy = np.ascontiguousarray(np.asarray(cells, dtype=np.int32).reshape(-1, 2))
        m = len(xy)
        out = np.zeros((m, m), np.uint8)
        check(self.ctx.lib.bl_shortcut_debug_visible(self.h, distances.h, xy.ctypes.data, m, out.ctypes.data))
        return out

    def debugPath(self):
        """0: the last launch staged the window in LDS; 1: it read the grids directly; -1 before the first."""
        return self.ctx.lib.bl_shortcut_debug_path(self.h)

    def lastDeviceMs(self):
        """(all kernels, k_sc_visible alone) of the last cells / poses call, in ms."""
        ms, mv = C.c_float(), C.c_float()
        check(self.ctx.lib.bl_shortcut_last_device_ms(self.h, C.byref(ms), C.byref(mv)))
        return ms.value, mv.value

    def close(self):
        if self.h:
            self.ctx.lib.bl_shortcut_destroy(self.h)
            self.h = None


class LikelihoodField:
    """Likelihood field (bl_lfield_*, include/botlab_hip.h): an int8 grid whose cells hold peak * exp(-d^2 / (2 sigma^2)) of their
    distance d to the nearest cell with log-odds >= occ_min, cut off beyond max_cells cells.  compute(grid) returns an OccupancyGrid
    that ParticleFilter.updateFilter / updateBegin and ScanMatcher.match* take where the map went.  It is not a map: it has no free /
    unknown distinction, so seeding, recovery, mapping, frontiers and the distance grids keep taking the real grid."""

    MAX_CELLS = 64

    def __init__(self, sigma=0.1, max_cells=None, occ_min=1, peak=127, ctx=None):
        self.ctx = ctx or default_context()
        self.sigma, self.max_cells, self.occ_min, self.peak = float(sigma), max_cells, int(occ_min), int(peak)
        h = C.c_void_p()
        check(self.ctx.lib.bl_lfield_create(self.ctx.h, C.byref(h)))
        self.h = h
        self.grid_ = None
        if max_cells is not None:
            self._set_params()

    def _set_params(self):
        p = _capi.LFieldParams(self.sigma, int(self.max_cells), self.occ_min, self.peak)
        check(self.ctx.lib.bl_lfield_set_params(self.h, C.byref(p)))

    def compute(self, grid):
        """The field of `grid` as it stands (enqueued; nothing waits).  The returned OccupancyGrid does not own its handle: it is the
        same object from call to call while the shape stays the same, and it dies with this field."""
        if self.max_cells is None:       # ceil(3 sigma cells_per_meter) in 1 .. 64, fixed here (1e-6 of slack: 3 * 0.1 * 20 is 6, not 7)
            self.max_cells = int(min(max(math.ceil(3.0 * self.sigma * float(grid.cpm) - 1e-6), 1), self.MAX_CELLS))
            self._set_params()
        check(self.ctx.lib.bl_lfield_compute(self.h, grid.h))
        raw = self.ctx.lib.bl_lfield_grid(self.h)
        g = self.grid_
        if g is None or g.h is None or g.h.value != raw or (g.width, g.height) != (grid.width, grid.height):
            g = OccupancyGrid.__new__(OccupancyGrid)
            g.ctx, g.h, g.owns_handle = self.ctx, C.c_void_p(raw), False
            self.grid_ = g
        g.width, g.height, g.mpc, g.cpm, g.origin = grid.width, grid.height, grid.mpc, grid.cpm, grid.origin
        return g

    def grid(self):
        """The OccupancyGrid of the last compute (None before the first)."""
        return self.grid_

    def table(self):
        """int8 [max_cells^2 + 2] of the last compute: the field's value by squared distance in cells; the last entry (FAR) is 0."""
        n = C.c_int()
        out = np.zeros(self.MAX_CELLS * self.MAX_CELLS + 2, np.int8)
        check(self.ctx.lib.bl_lfield_table(self.h, out.ctypes.data, C.byref(n)))
        return out[:n.value].copy()

    def lastDeviceMs(self):
        """Device time of the last compute in ms (waits for it)."""
        ms = C.c_float()
        check(self.ctx.lib.bl_lfield_last_device_ms(self.h, C.byref(ms)))
        return ms.value

    def close(self):
        if self.h:
            self.ctx.lib.bl_lfield_destroy(self.h)
            self.h = None
            if self.grid_ is not None:
                self.grid_.h = None
                self.grid_ = None


class ObstacleLayer:
    """Obstacle layer (bl_obslayer_*, include/botlab_hip.h): what the scan sees and the map does not.  update(grid, scan, pose) casts
    the scan against the static map and keeps a per-cell hit / clear / expire state; compose(grid, out) writes the map with 127 where
    the layer is live into another OccupancyGrid, which the distance grids (and so every planner) take where the map went.  Rays at
    or beyond max_range neither hit nor clear; an obstacle that left with nothing behind it goes by expiry (ttl_scans)."""

    OFF, EXPLAINED, NOVEL, THROUGH, OUTSIDE = 0, 1, 2, 3, 4

    def __init__(self, width, height, max_range=5.0, occ_min=1, tol_cells=1, ttl_scans=50, min_hits=1, ctx=None):
        self.ctx = ctx or default_context()
        self.width, self.height = int(width), int(height)
        h = C.c_void_p()
        check(self.ctx.lib.bl_obslayer_create(self.ctx.h, self.width, self.height, C.byref(h)))
        self.h = h
        try:
            self.setParams(max_range, occ_min, tol_cells, ttl_scans, min_hits)
        except _capi.BotlabHipError:
            self.close()
            raise

    def setParams(self, max_range, occ_min, tol_cells, ttl_scans, min_hits):
        """Refused (BotlabHipError raised): the layer keeps the parameters it had."""
        p = _capi.ObsLayerParams(float(np.float32(max_range)), int(occ_min), int(tol_cells), int(ttl_scans), int(min_hits))
        check(self.ctx.lib.bl_obslayer_set_params(self.h, C.byref(p)))
        self.params = p

    def update(self, grid, scan, pose):
        """One update from `scan` taken at `pose` against the static map `grid` (enqueued; nothing waits for the kernels)."""
        ls = scan.as_c()
        check(self.ctx.lib.bl_obslayer_update(self.h, grid.h, C.byref(ls), C.byref(pose)))

    def compose(self, grid, out=None):
        """`grid` with 127 where the layer is live, written into `out` (another OccupancyGrid of the same shape; made when None)."""
        if out is None:
            out = OccupancyGrid(ctx=self.ctx, _raw=(grid.width, grid.height, grid.mpc, grid.cpm, grid.origin[0], grid.origin[1]))
        check(self.ctx.lib.bl_obslayer_compose(self.h, grid.h, out.h))
        out.mpc, out.cpm, out.origin = grid.mpc, grid.cpm, grid.origin
        return out

    def classes(self):
        """uint8 per ray of the last update's scan, in scan order (OFF, EXPLAINED, NOVEL, THROUGH, OUTSIDE)."""
        n = C.c_int()
        check(self.ctx.lib.bl_obslayer_classes(self.h, None, C.byref(n)))
        out = np.zeros(max(n.value, 1), np.uint8)
        check(self.ctx.lib.bl_obslayer_classes(self.h, out.ctypes.data, C.byref(n)))
        return out[:n.value]

    def stats(self):
        """dict: n, valid (rays), classes [5], hs (|Hs|), clr (|C \\ Hs|), live (cells)."""
        s = _capi.ObsLayerStats()
        check(self.ctx.lib.bl_obslayer_stats(self.h, C.byref(s)))
        return dict(n=int(s.n), valid=int(s.valid_rays), classes=[int(v) for v in s.rays_by_class], hs=int(s.hit_cells),
                    clr=int(s.cleared_cells), live=int(s.live_cells))

    def live_cells(self, cap=None):
        """int32 [m][2] of the live cells (x, y) in row-major order; at most cap of them."""
        n = C.c_int()
        if cap is None:
            check(self.ctx.lib.bl_obslayer_live_cells(self.h, None, 0, C.byref(n)))
            cap = n.value
        out = np.zeros((max(int(cap), 1), 2), np.int32)
        check(self.ctx.lib.bl_obslayer_live_cells(self.h, out.ctypes.data, int(cap), C.byref(n)))
        return out[:min(n.value, int(cap))]

    def download(self):
        """(count uint8 [H][W], last uint32 [H][W], n)."""
        count = np.empty((self.height, self.width), np.uint8)
        last = np.empty((self.height, self.width), np.uint32)
        n = C.c_uint32()
        check(self.ctx.lib.bl_obslayer_download(self.h, count.ctypes.data, last.ctypes.data, C.byref(n)))
        return count, last, int(n.value)

    def upload(self, count, last, n):
        """Replaces the state (tests, a restored layer): saturation, expiry and the counter's end are reached this way."""
        count = np.ascontiguousarray(count, dtype=np.uint8)
        last = np.ascontiguousarray(last, dtype=np.uint32)
        assert count.shape == (self.height, self.width) and last.shape == (self.height, self.width)
        check(self.ctx.lib.bl_obslayer_upload(self.h, count.ctypes.data, last.ctypes.data, C.c_uint32(int(n))))

    def reset(self):
        check(self.ctx.lib.bl_obslayer_reset(self.h))

    def lastDeviceMs(self):
        """(update_ms, compose_ms): device time of the last update and the last compose (waits for them)."""
        u, c = C.c_float(), C.c_float()
        check(self.ctx.lib.bl_obslayer_last_device_ms(self.h, C.byref(u), C.byref(c)))
        return u.value, c.value

    def close(self):
        if self.h:
            self.ctx.lib.bl_obslayer_destroy(self.h)
            self.h = None


BEAM_OFF_GRID = -2 ** 63


class BeamModel:
    """Ray-cast (beam) sensor model (bl_beam_*, include/botlab_hip.h): every used ray of a scan cast against the map as far as
    max_range and the measured range scored against the expected one, for many poses at once.  scores() for host poses; reweigh()
    replaces a ParticleFilter's weight units in place and returns the beam-weighted posterior pose.  Every parameter is an untuned knob;
    span (Q16 nats) is the score gap at which a particle reaches the floor."""

    def __init__(self, max_range=5.0, occ_min=1, sigma_cells=1.0, z_hit=0.7, z_short=0.1, z_max=0.05, z_rand=0.15, lam=0.1,
                 blocked_factor=0.1, hit_cut=64, span=1 << 22, ray_stride=1, ctx=None):
        self.ctx = ctx or default_context()
        h = C.c_void_p()
        check(self.ctx.lib.bl_beam_create(self.ctx.h, C.byref(h)))
        self.h = h
        try:
            self.setParams(max_range, occ_min, sigma_cells, z_hit, z_short, z_max, z_rand, lam, blocked_factor, hit_cut, span, ray_stride)
        except _capi.BotlabHipError:
            self.close()
            raise

    def setParams(self, max_range, occ_min, sigma_cells, z_hit, z_short, z_max, z_rand, lam, blocked_factor, hit_cut, span, ray_stride):
        """Refused (BotlabHipError raised): the model keeps the parameters it had."""
        p = _capi.BeamParams(max_range, sigma_cells, z_hit, z_short, z_max, z_rand, lam, blocked_factor, int(occ_min), int(hit_cut),
                             int(ray_stride), 0, int(span))
        check(self.ctx.lib.bl_beam_set_params(self.h, C.byref(p)))
        self.params = p

    def tables(self, cells_per_meter):
        """dict: hit [1024], short [1024], lt [256] (uint32) and rand, max_free, max_blocked, ln2, reach for a map of cells_per_meter."""
        hit, short, lt, sc = np.zeros(1024, np.uint32), np.zeros(1024, np.uint32), np.zeros(256, np.uint32), np.zeros(5, np.uint32)
        check(self.ctx.lib.bl_beam_tables(self.h, C.c_float(cells_per_meter), hit.ctypes.data, short.ctypes.data, lt.ctypes.data, sc.ctypes.data))
        return dict(hit=hit, short=short, lt=lt, rand=int(sc[0]), max_free=int(sc[1]), max_blocked=int(sc[2]), ln2=int(sc[3]), reach=int(sc[4]))

    @staticmethod
    def unitTable():
        """U[0 .. 256] (host arithmetic only; needs no GPU)."""
        out = np.zeros(257, np.uint32)
        _capi.load().bl_beam_unit_table(out.ctypes.data)
        return out

    def _scores(self, fn, source, scan, poses):
        """Poses in, scores out through bl_beam_scores, bl_rangetable_scores or bl_clearance_scores; source: the grid, the table or the
        clearance grid."""
        q = np.ascontiguousarray(poses, dtype=np.float32).reshape(-1, 3)
        hp = np.zeros(len(q), POSE_DTYPE)
        hp["x"], hp["y"], hp["theta"] = q[:, 0], q[:, 1], q[:, 2]
        out = np.zeros(max(len(q), 1), np.int64)
        ls = scan.as_c()
        check(fn(self.h, source.h, C.byref(ls), hp.ctypes.data, len(q), out.ctypes.data))
        return out[:len(q)]

    def _debug(self, fn, source, scan, pose, names):
        """The debug planes of one pose, int32 each but p (uint32), cut to the used rays."""
        ls = scan.as_c()
        m = max(scan.num_ranges, 1)
        a = [np.zeros(m, np.uint32 if k == "p" else np.int32) for k in names]
        po = make_pose(*pose)
        check(fn(self.h, source.h, C.byref(ls), C.byref(po), *[v.ctypes.data for v in a]))
        r = self.ctx.lib.bl_beam_last_rays(self.h)
        return {k: v[:r].astype(np.int64) for k, v in zip(names, a)}

    def _reweigh(self, fn, pf, source, scan):
        ls = scan.as_c()
        out = Pose()
        check(fn(self.h, pf.h, source.h, C.byref(ls), C.byref(out)))
        return out

    def scores(self, grid, scan, poses):
        """int64 [n]: S of n poses, an [n][3] array of x, y, theta (BEAM_OFF_GRID for a pose that takes no part)."""
        return self._scores(self.ctx.lib.bl_beam_scores, grid, scan, poses)

    def units(self, n):
        """uint32 [n]: the units of the last scores() or reweigh() (n: that call's count)."""
        out = np.zeros(max(int(n), 1), np.uint32)
        check(self.ctx.lib.bl_beam_units(self.h, out.ctypes.data, int(n)))
        return out[:int(n)]

    def debug_cast(self, grid, scan, pose):
        """dict of int64 arrays over the used rays of one pose (x, y, theta): first, K, z, zstar, p."""
        return self._debug(self.ctx.lib.bl_beam_debug_cast, grid, scan, pose, ("first", "K", "z", "zstar", "p"))

    def reweigh(self, pf, grid, scan):
        """bl_beam_reweigh_pf: the filter's weight units replaced in place; returns the beam-weighted posterior pose."""
        return self._reweigh(self.ctx.lib.bl_beam_reweigh_pf, pf, grid, scan)

    def scores_table(self, table, scan, poses):
        """bl_rangetable_scores: scores() with the expected ranges looked up in a built RangeTable instead of cast against the map.
        The table is not checked against the live map."""
        return self._scores(self.ctx.lib.bl_rangetable_scores, table, scan, poses)

    def debug_lookup(self, table, scan, pose):
        """dict of int64 arrays over the used rays of one pose (x, y, theta): h, z, zstar, p."""
        return self._debug(self.ctx.lib.bl_rangetable_debug_lookup, table, scan, pose, ("h", "z", "zstar", "p"))

    def reweigh_table(self, pf, table, scan):
        """bl_rangetable_reweigh_pf: reweigh() with the table behind it."""
        return self._reweigh(self.ctx.lib.bl_rangetable_reweigh_pf, pf, table, scan)

    def scores_leap(self, clearance, scan, poses):
        """bl_clearance_scores: scores() with the expected ranges found by leaps over a built ClearanceGrid; value for value the
        cast's on the map the grid was built on.  The grid is not checked against the live map."""
        return self._scores(self.ctx.lib.bl_clearance_scores, clearance, scan, poses)

    def debug_leap(self, clearance, scan, pose):
        """dict of int64 arrays over the used rays of one pose (x, y, theta): first, K, z, zstar, p as debug_cast, and rounds (the
        entries of the clearance grid the ray read; -1 for a dropped ray)."""
        return self._debug(self.ctx.lib.bl_clearance_debug_cast, clearance, scan, pose, ("first", "K", "z", "zstar", "p", "rounds"))

    def reweigh_leap(self, pf, clearance, scan):
        """bl_clearance_reweigh_pf: reweigh() with the leaps behind it."""
        return self._reweigh(self.ctx.lib.bl_clearance_reweigh_pf, pf, clearance, scan)

    def debugSet(self, stage_windows=False, window_bytes=0):
        """Stage the workgroups' windows in LDS when they fit window_bytes (0: 40960).  Off by default: the grid is read directly."""
        check(self.ctx.lib.bl_beam_debug_set(self.h, 1 if stage_windows else 0, int(window_bytes)))

    def debugPath(self):
        """0 every workgroup staged its window in LDS, 1 every one read the grid, 2 some of each; -1 before the first launch."""
        return self.ctx.lib.bl_beam_debug_path(self.h)

    def lastDeviceMs(self):
        ms = C.c_float()
        check(self.ctx.lib.bl_beam_last_device_ms(self.h, C.byref(ms)))
        return ms.value

    def close(self):
        if self.h:
            self.ctx.lib.bl_beam_destroy(self.h)
            self.h = None


class RangeTable:
    """Range table (bl_rangetable_*, include/botlab_hip.h): the beam model's expected range of every (cell, heading) of a map that does
    not change, built once on the device and read by BeamModel.scores_table / reweigh_table.  build(beam, grid) takes reach and occ_min
    from the beam model; update(grid, x0, y0, x1, y1) after the cells of that box (inclusive) changed.  The table is never checked
    against the live map: keeping it current is the caller's job."""

    NONE = 0xFFFF

    def __init__(self, ctx=None, headings=256):
        self.ctx = ctx or default_context()
        h = C.c_void_p()
        check(self.ctx.lib.bl_rangetable_create(self.ctx.h, int(headings), C.byref(h)))
        self.h = h

    def build(self, beam, grid):
        check(self.ctx.lib.bl_rangetable_build(self.h, beam.h, grid.h))

    def update(self, grid, x0, y0, x1, y1):
        check(self.ctx.lib.bl_rangetable_update(self.h, grid.h, int(x0), int(y0), int(x1), int(y1)))

    def info(self):
        """dict: width, height, headings, reach, occ_min, built, bytes."""
        i = _capi.RangeTableInfo()
        check(self.ctx.lib.bl_rangetable_info(self.h, C.byref(i)))
        return {k: int(getattr(i, k)) for k, _ in _capi.RangeTableInfo._fields_}

    def read(self, x0=0, y0=0, w=None, h=None):
        """uint16 [h][w][headings]: the entries of a rectangle of cells (default: from (x0, y0) to the far corner)."""
        i = self.info()
        w = i["width"] - x0 if w is None else w
        h = i["height"] - y0 if h is None else h
        out = np.zeros((max(h, 1), max(w, 1), i["headings"]), np.uint16)
        check(self.ctx.lib.bl_rangetable_read(self.h, int(x0), int(y0), int(w), int(h), out.ctypes.data))
        return out

    def directions(self):
        """int32 [headings][2]: D[h] of the built table."""
        out = np.zeros((self.info()["headings"], 2), np.int32)
        check(self.ctx.lib.bl_rangetable_directions(self.h, out.ctypes.data))
        return out

    def lastDeviceMs(self):
        ms = C.c_float()
        check(self.ctx.lib.bl_rangetable_last_device_ms(self.h, C.byref(ms)))
        return ms.value

    def close(self):
        if self.h:
            self.ctx.lib.bl_rangetable_destroy(self.h)
            self.h = None


class ClearanceGrid:
    """Clearance grid (bl_clearance_*, include/botlab_hip.h): per cell the Chebyshev distance to the nearest occupied cell, capped at
    cap, one uint8, read by BeamModel.scores_leap / reweigh_leap to leap over empty space.  build(grid, occ_min) fills it;
    update(grid, x0, y0, x1, y1) after the cells of that box (inclusive) changed redoes the box widened by cap.  The grid is never
    checked against the live map: keeping it current is the caller's job.  cap is an untuned knob."""

    def __init__(self, ctx=None, cap=64):
        self.ctx = ctx or default_context()
        h = C.c_void_p()
        check(self.ctx.lib.bl_clearance_create(self.ctx.h, int(cap), C.byref(h)))
        self.h = h

    def build(self, grid, occ_min=1):
        check(self.ctx.lib.bl_clearance_build(self.h, grid.h, int(occ_min)))

    def update(self, grid, x0, y0, x1, y1):
        check(self.ctx.lib.bl_clearance_update(self.h, grid.h, int(x0), int(y0), int(x1), int(y1)))

    def info(self):
        """dict: width, height, cap, occ_min, built, bytes."""
        i = _capi.ClearanceInfo()
        check(self.ctx.lib.bl_clearance_info(self.h, C.byref(i)))
        return {k: int(getattr(i, k)) for k, _ in _capi.ClearanceInfo._fields_ if k != "pad"}

    def read(self, x0=0, y0=0, w=None, h=None):
        """uint8 [h][w]: the entries of a rectangle of cells (default: from (x0, y0) to the far corner)."""
        i = self.info()
        w = i["width"] - x0 if w is None else w
        h = i["height"] - y0 if h is None else h
        out = np.zeros((max(h, 1), max(w, 1)), np.uint8)
        check(self.ctx.lib.bl_clearance_read(self.h, int(x0), int(y0), int(w), int(h), out.ctypes.data))
        return out

    def lastDeviceMs(self):
        ms = C.c_float()
        check(self.ctx.lib.bl_clearance_last_device_ms(self.h, C.byref(ms)))
        return ms.value

    def close(self):
        if self.h:
            self.ctx.lib.bl_clearance_destroy(self.h)
            self.h = None


class ObstacleTracker:
    """Obstacle tracks (bl_obstracks_*, include/botlab_hip.h): the layer's live cells grouped into blobs, the blobs followed from
    update to update, and a composed grid that also holds where the moving ones are heading.  update() once after each
    layer.update(...); compose(grid, out, horizon, robot_cell) where layer.compose went.  Every parameter is an untuned knob."""

    CONFIRMED, MOVING, MATCHED, BORN = 1, 2, 4, 8
    MAX_TRACKS, MAX_BLOBS, MAX_CELLS = 256, 1024, 65536
    PARAMS = ("min_cells", "max_cells", "gate_cells", "alpha", "beta", "confirm_hits", "max_missed", "min_speed")

    def __init__(self, layer, min_cells=1, max_cells=65536, gate_cells=4, alpha=128, beta=64, confirm_hits=3, max_missed=3, min_speed=16):
        self.layer = layer
        self.ctx = layer.ctx
        h = C.c_void_p()
        check(self.ctx.lib.bl_obstracks_create(self.ctx.h, layer.width, layer.height, C.byref(h)))
        self.h = h
        try:
            self.setParams(min_cells, max_cells, gate_cells, alpha, beta, confirm_hits, max_missed, min_speed)
        except _capi.BotlabHipError:
            self.close()
            raise

    def setParams(self, min_cells, max_cells, gate_cells, alpha, beta, confirm_hits, max_missed, min_speed):
        """Refused (BotlabHipError raised): the tracker keeps the parameters it had."""
        p = _capi.ObsTracksParams(int(min_cells), int(max_cells), int(gate_cells), int(alpha), int(beta), int(confirm_hits), int(max_missed),
                                  int(min_speed))
        check(self.ctx.lib.bl_obstracks_set_params(self.h, C.byref(p)))
        self.params = p

    def update(self):
        """One update from the layer's state as it stands (enqueued; nothing waits for the kernels).  Two refusals are found on the
        device only -- more than MAX_CELLS live cells, a birth that would need id 2^32 - 1 -- and do not raise: the slots stay as they
        were, there are no blobs, and stats()["refused"] is 1 or 2.  A caller that never reads stats() never learns of them."""
        check(self.ctx.lib.bl_obstracks_update(self.h, self.layer.h))

    def compose(self, grid, out=None, horizon=0, robot_cell=(0, 0), keep_clear=-1):
        """layer.compose(grid, out), and 127 also where the confirmed moving tracks' cells will be within `horizon` updates, except
        within keep_clear cells (Chebyshev) of robot_cell."""
        if out is None:
            out = OccupancyGrid(ctx=self.ctx, _raw=(grid.width, grid.height, grid.mpc, grid.cpm, grid.origin[0], grid.origin[1]))
        c = _capi.ObsTracksCompose(int(horizon), int(robot_cell[0]), int(robot_cell[1]), int(keep_clear))
        check(self.ctx.lib.bl_obstracks_compose(self.h, self.layer.h, grid.h, out.h, C.byref(c)))
        out.mpc, out.cpm, out.origin = grid.mpc, grid.cpm, grid.origin
        return out

    def composeStatic(self, grid, out=None):
        """layer.compose(grid, out) without the cells of the confirmed moving tracks' blobs, which keep the map's value: the grid for
        the field of LocalPlanner.commands_moving, which meets the moving obstacles where they will be."""
        if out is None:
            out = OccupancyGrid(ctx=self.ctx, _raw=(grid.width, grid.height, grid.mpc, grid.cpm, grid.origin[0], grid.origin[1]))
        check(self.ctx.lib.bl_obstracks_compose_static(self.h, self.layer.h, grid.h, out.h))
        out.mpc, out.cpm, out.origin = grid.mpc, grid.cpm, grid.origin
        return out

    def tracks(self):
        """The occupied slots in slot order: a structured array (id, px, py, vx, vy, hits, missed, area, x0, y0, x1, y1, flags, slot)."""
        out = np.zeros(self.MAX_TRACKS, _capi.OBSTRACK_DTYPE)
        n = C.c_int()
        check(self.ctx.lib.bl_obstracks_tracks(self.h, out.ctypes.data, self.MAX_TRACKS, C.byref(n)))
        return out[:n.value]

    def blobs(self):
        """The kept blobs of the last update in rank order: a structured array (sum_x, sum_y, area, x0, y0, x1, y1, cx, cy, eligible,
        track, rep)."""
        out = np.zeros(self.MAX_BLOBS, _capi.OBSBLOB_DTYPE)
        n = C.c_int()
        check(self.ctx.lib.bl_obstracks_blobs(self.h, out.ctypes.data, self.MAX_BLOBS, C.byref(n)))
        return out[:n.value]

    def labels(self):
        """int32 per live cell of the last update, in the order of layer.live_cells(): its blob's rank, -1 when dropped."""
        n = C.c_int()
        check(self.ctx.lib.bl_obstracks_labels(self.h, None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), np.int32)
        check(self.ctx.lib.bl_obstracks_labels(self.h, out.ctypes.data, n.value, C.byref(n)))
        return out[:n.value]

    def stats(self):
        s = _capi.ObsTracksStats()
        check(self.ctx.lib.bl_obstracks_stats(self.h, C.byref(s)))
        return {k: int(getattr(s, k)) for k, _ in _capi.ObsTracksStats._fields_}

    def download(self):
        """(slots: all 256 as a structured array, dict(n, next_id, fresh))."""
        out = np.zeros(self.MAX_TRACKS, _capi.OBSTRACK_DTYPE)
        st = _capi.ObsTracksState()
        check(self.ctx.lib.bl_obstracks_download(self.h, out.ctypes.data, C.byref(st)))
        return out, dict(n=int(st.n), next_id=int(st.next_id), fresh=int(st.fresh))

    def upload(self, slots, n, next_id, fresh):
        """Replaces the state (tests, a restored tracker); the blobs of the last update are forgotten."""
        slots = np.ascontiguousarray(slots, dtype=_capi.OBSTRACK_DTYPE)
        assert slots.shape == (self.MAX_TRACKS,)
        st = _capi.ObsTracksState(int(n), int(next_id), int(bool(fresh)), 0)
        check(self.ctx.lib.bl_obstracks_upload(self.h, slots.ctypes.data, C.byref(st)))

    def reset(self):
        check(self.ctx.lib.bl_obstracks_reset(self.h))

    def lastDeviceMs(self):
        """(update_ms, compose_ms): device time of the last update and the last compose (waits for them)."""
        u, c = C.c_float(), C.c_float()
        check(self.ctx.lib.bl_obstracks_last_device_ms(self.h, C.byref(u), C.byref(c)))
        return u.value, c.value

    def close(self):
        if self.h:
            self.ctx.lib.bl_obstracks_destroy(self.h)
            self.h = None


def track_to_metric(track, grid, scan_period):
    """(x, y, vx, vy) in metres and metres per second of one record of ObstacleTracker.tracks(), in the frame of `grid` (anything with
    origin and mpc), one update taking scan_period seconds.  Double arithmetic on the host."""
    mpc = float(grid.mpc)
    return (float(grid.origin[0]) + int(track["px"]) / 256.0 * mpc, float(grid.origin[1]) + int(track["py"]) / 256.0 * mpc,
            int(track["vx"]) / 256.0 * mpc / float(scan_period), int(track["vy"]) / 256.0 * mpc / float(scan_period))


def nav_min_traversable_cells(distances, searchParams):
    """n_min: the smallest L1 distance (in cells) that is traversable under searchParams -- f[n] > minDistanceToObstacle * 1.000001
    with the distance grid's own table f[n] = f[n - 1] + 0.1f; None if no distance of this grid is."""
    w, h = distances.shape()
    f = np.float32(0.0)
    for n in range(w + h + 1):
        if float(f) > searchParams.minDistanceToObstacle * 1.000001:
            return n
        f = np.float32(f + np.float32(0.1))
    return None


def plan_path_to_frontier_by_cost(frontiers, robotPose, grid, planner, reach_cells=None, obstacle_gain=NAV_OBSTACLE_GAIN, cap=1 << 16,
                                  field=None):
    """The frontier that is cheapest to reach, not the one closest in a straight line: ONE navigation field whose goals are every
    cell of every frontier, and one descent from the robot.  A frontier cell borders unknown space and is never traversable itself,
    so a goal counts as reached within reach_cells of it; the default is n_min, the smallest traversable L1 distance under the
    planner's parameters.  Returns (path, index of the chosen frontier or -1, cost); an empty frontier list gives the empty path, as
    plan_path_to_frontier does.  `grid` is unused, as there."""
    dist = planner.distances_
    ctx = dist.ctx
    fr = frontiers.cells() if isinstance(frontiers, Frontiers) else [np.asarray(f, dtype=np.float32).reshape(-1, 2) for f in frontiers]
    if len(fr) == 0:
        return [], -1, NAV_UNREACHED
    if reach_cells is None:
        reach_cells = nav_min_traversable_cells(dist, planner.searchParams_)
        if reach_cells is None:
            reach_cells = 0
    mpc, cpm, ox, oy = dist.frame()
    owner, cells = [], []
    for k, f in enumerate(fr):
        for x, y in f:                                   # global_position_to_grid_cell (grid_utils.hpp:33-38)
            cells.append((int((float(x) - float(ox)) * float(cpm)), int((float(y) - float(oy)) * float(cpm))))
            owner.append(k)
    nf = field or NavigationField(ctx)
    try:
        nf.compute(dist, nav_params(planner.searchParams_, obstacle_gain, reach_cells), np.array(cells, np.int32).reshape(-1, 2))
        paths, labels, costs = nf.paths([robotPose], cap_each=cap)
    finally:
        if field is None:
            nf.close()
    label = int(labels[0])
    return paths[0], (owner[label] if label >= 0 else -1), int(costs[0])


class ViewGain:
    """The view gain (bl_viewgain_*, include/botlab_hip.h): the number of distinct unknown cells a fan of n_rays rays of
    radius_cells cells, cast from a candidate cell through the log-odds grid, reaches before a blocking cell or the edge of the
    grid ends each ray."""

    def __init__(self, radius_cells=60, n_rays=360, occupied_above=0, unknown_lo=0, unknown_hi=0, ctx=None):
        self.ctx = ctx or default_context()
        h = C.c_void_p()
        check(self.ctx.lib.bl_viewgain_create(self.ctx.h, C.byref(h)))
        self.h = h
        try:
            self.setParams(radius_cells, n_rays, occupied_above, unknown_lo, unknown_hi)
        except _capi.BotlabHipError:
            self.close()
            raise

    def setParams(self, radius_cells, n_rays, occupied_above=0, unknown_lo=0, unknown_hi=0):
        p = _capi.ViewGainParams(int(radius_cells), int(n_rays), int(occupied_above), int(unknown_lo), int(unknown_hi))
        check(self.ctx.lib.bl_viewgain_set_params(self.h, C.byref(p)))
        self.radius_cells = int(radius_cells)

    def rayEnds(self):
        """(n_rays, 2) int32: the end offset (x, y) of every ray, as the kernel uses it."""
        n = C.c_int()
        check(self.ctx.lib.bl_viewgain_ray_ends(self.h, None, C.byref(n)))
        out = np.zeros((n.value, 2), np.int32)
        check(self.ctx.lib.bl_viewgain_ray_ends(self.h, out.ctypes.data, C.byref(n)))
        return out

    def compute(self, grid, cells):
        """uint32 gain of every candidate; cells: (n, 2) integer cells (x, y)."""
        q = np.ascontiguousarray(np.asarray(cells, dtype=np.int32).reshape(-1, 2))
        out = np.zeros(len(q), np.uint32)
        check(self.ctx.lib.bl_viewgain_compute(self.h, grid.h, q.ctypes.data if len(q) else None, len(q), out.ctypes.data if len(q) else None))
        return out

    def debugSeen(self, grid, x, y):
        """(2R + 1, 2R + 1) uint8, 0 / 1: the seen set of one candidate in the window around it."""
        side = 2 * self.radius_cells + 1
        out = np.zeros((side, side), np.uint8)
        check(self.ctx.lib.bl_viewgain_debug_seen(self.h, grid.h, int(x), int(y), out.ctypes.data))
        return out

    def close(self):
        if self.h:
            self.ctx.lib.bl_viewgain_destroy(self.h)
            self.h = None


class RBSlam:
    """Rao-Blackwellized grid SLAM (bl_rbslam_*, include/botlab_hip.h): numParticles particles, each with a pose, a parent pose, a
    cumulative score and its own map of `grid`'s shape and frame; weighed against its own map, resampled -- maps and all -- when
    num * P * sum u^2 >= den * (sum u)^2."""

    def __init__(self, numParticles, width, height, metersPerCell, cellsPerMeter, origin, maxLaserDistance, hitOdds, missOdds, ctx=None):
        self.ctx = ctx or default_context()
        self.P, self.width, self.height = int(numParticles), int(width), int(height)
        self.mpc, self.cpm = np.float32(metersPerCell), np.float32(cellsPerMeter)
        self.origin = (np.float32(origin[0]), np.float32(origin[1]))
        h = C.c_void_p()
        check(self.ctx.lib.bl_rbslam_create(self.ctx.h, self.P, self.width, self.height, self.mpc, self.cpm, self.origin[0], self.origin[1],
                                            np.float32(maxLaserDistance), int(hitOdds), int(missOdds), C.byref(h)))
        self.h = h

    @classmethod
    def like(cls, numParticles, grid, maxLaserDistance, hitOdds, missOdds):
        """Maps of the shape and frame of an OccupancyGrid."""
        return cls(numParticles, grid.width, grid.height, grid.mpc, grid.cpm, grid.origin, maxLaserDistance, hitOdds, missOdds, ctx=grid.ctx)

    def setResampling(self, num, den):
        check(self.ctx.lib.bl_rbslam_set_resampling(self.h, int(num), int(den)))

    def setNoiseSeed(self, seed):
        check(self.ctx.lib.bl_rbslam_set_noise_seed(self.h, C.c_uint64(seed)))

    def initializeAtPose(self, pose, seed=None):
        if seed is None:
            seed = int.from_bytes(np.random.bytes(8), "little")
        check(self.ctx.lib.bl_rbslam_init_at_pose(self.h, C.byref(pose), C.c_uint64(seed)))

    def setParticles(self, particles, cum_scores=None):
        p = np.ascontiguousarray(particles)
        assert p.dtype.itemsize == 56 and p.size == self.P
        c = None
        if cum_scores is not None:
            c = np.ascontiguousarray(cum_scores, dtype=np.int64)
            assert c.size == self.P
        check(self.ctx.lib.bl_rbslam_set_particles(self.h, p.ctypes.data, c.ctypes.data if c is not None else None))

    def particles(self):
        """(particles as PARTICLE_DTYPE, cumulative scores int64, weight units uint64)."""
        out = np.zeros(self.P, dtype=PARTICLE_DTYPE)
        cum = np.zeros(self.P, np.int64)
        units = np.zeros(self.P, np.uint64)
        check(self.ctx.lib.bl_rbslam_get_particles(self.h, out.ctypes.data, cum.ctypes.data, units.ctypes.data))
        return out, cum, units

    def update(self, odometry, laser, rand_value=None, noise=None):
        """One update; returns dict(moved, resampled, best, pose, S, Q).  noise (3 * P float32) replaces the Philox action noise."""
        if rand_value is None:
            rand_value = _libc.rand()
        ls = laser.as_c()
        nz = None
        if noise is not None:
            nz = np.ascontiguousarray(noise, dtype=np.float32)
            assert nz.size == 3 * self.P
        r = _capi.RBSlamResult()
        check(self.ctx.lib.bl_rbslam_update(self.h, C.byref(odometry), C.byref(ls), int(rand_value), nz.ctypes.data if nz is not None else None,
                                            C.byref(r)))
        bp = r.best_pose
        return dict(moved=bool(r.moved), resampled=bool(r.resampled), best=int(r.best), pose=Pose(bp.utime, bp.x, bp.y, bp.theta), S=int(r.S),
                    Q=(int(r.Q_hi) << 64) | int(r.Q_lo))

    def mapCells(self, p):
        out = np.empty((self.height, self.width), np.int8)
        check(self.ctx.lib.bl_rbslam_map_download(self.h, int(p), out.ctypes.data))
        return out

    def uploadMap(self, p, cells):
        c = np.ascontiguousarray(cells, dtype=np.int8)
        assert c.shape == (self.height, self.width)
        check(self.ctx.lib.bl_rbslam_map_upload(self.h, int(p), c.ctypes.data))

    def best_map(self, grid=None):
        """The best particle's map as an OccupancyGrid (device to device; `grid`: one of the same shape to fill)."""
        if grid is None:
            grid = OccupancyGrid(ctx=self.ctx, _raw=(self.width, self.height, self.mpc, self.cpm, self.origin[0], self.origin[1]))
        check(self.ctx.lib.bl_rbslam_best_map(self.h, grid.h))
        grid.mpc, grid.cpm, grid.origin = self.mpc, self.cpm, self.origin
        return grid

    bestMap = best_map

    def debugLast(self):
        idx = np.empty(self.P, np.int32)
        like = np.empty(self.P, np.int32)
        check(self.ctx.lib.bl_rbslam_debug_last(self.h, idx.ctypes.data, like.ctypes.data))
        return idx, like

    MATCH_FIELDS = ("di", "dj", "dk", "score", "score_centre", "ties", "accepted")

    def setScanMatching(self, nx=2, ny=2, ntheta=4, dtheta=math.radians(0.5), max_range=8.0, min_score=0):
        """Scan-matched proposals: after the action of a moved update every particle matches the scan against its own map in the
        window +-nx, +-ny cells, +-ntheta steps of dtheta around its pose and moves to the best pose there.  setScanMatching(None): off."""
        if nx is None:
            check(self.ctx.lib.bl_rbslam_set_scan_matching(self.h, None))
            return
        p = _capi.RBSlamMatchParams(int(nx), int(ny), int(ntheta), float(dtheta), float(max_range), int(min_score))
        check(self.ctx.lib.bl_rbslam_set_scan_matching(self.h, C.byref(p)))

    def debugMatch(self):
        """dict of int32 arrays (di, dj, dk, score, score_centre, ties, accepted) of the last moved update with matching on."""
        out = [np.empty(self.P, np.int32) for _ in self.MATCH_FIELDS]
        check(self.ctx.lib.bl_rbslam_debug_match(self.h, *[a.ctypes.data for a in out]))
        return dict(zip(self.MATCH_FIELDS, out))

    def debugMatchPath(self):
        return int(self.ctx.lib.bl_rbslam_debug_match_path(self.h))

    def close(self):
        if self.h:
            self.ctx.lib.bl_rbslam_destroy(self.h)
            self.h = None


def plan_path_to_frontier_by_gain(frontiers, robotPose, grid, planner, view=None, reach_cells=None, stride=1, min_gain=1, gain_weight=1,
                                  obstacle_gain=NAV_OBSTACLE_GAIN, cap=1 << 16):
    """The viewpoint near a frontier that weighs expected new map against travel cost.  Candidates are the cells within Chebyshev
    reach_cells (default n_min, as plan_path_to_frontier_by_cost) of a frontier cell that the robot can reach, in row-major order,
    thinned to x % stride == 0 and y % stride == 0; cost(c) is the navigation field rooted at the robot's cell, gain(c) the view
    gain (`view`: a ViewGain, default ViewGain() on the grid's context).  Of the candidates with gain >= min_gain the one that
    maximises gain_weight * gain - cost is chosen, ties by lower cost, then lower y, then lower x; the path is the cheapest one to
    that cell (a second field, rooted there).  gain_weight = 1 is UNTUNED -- one newly seen cell is worth a tenth of a straight
    step --: a knob for the caller, not a result.
    Returns (path, frontier index, chosen cell (x, y) or None, gain, cost): the candidate's frontier is the owner of the
    lowest-indexed frontier cell within reach of it.  An empty frontier list gives the empty path and -1; no surviving candidate
    gives the robot's 1-pose path and -1."""
    dist = planner.distances_
    ctx = dist.ctx
    fr = frontiers.cells() if isinstance(frontiers, Frontiers) else [np.asarray(f, dtype=np.float32).reshape(-1, 2) for f in frontiers]
    if len(fr) == 0:
        return [], -1, None, 0, NAV_UNREACHED
    none = ([Pose(robotPose.utime, robotPose.x, robotPose.y, robotPose.theta)], -1, None, 0, NAV_UNREACHED)
    if reach_cells is None:
        reach_cells = nav_min_traversable_cells(dist, planner.searchParams_)
        if reach_cells is None:
            reach_cells = 0
    reach_cells, stride = int(reach_cells), max(int(stride), 1)
    mpc, cpm, ox, oy = dist.frame()
    w, h = dist.shape()
    rvx = (float(np.float32(robotPose.x)) - float(ox)) * float(cpm)      # the cell of a pose as the navigation field finds it
    rvy = (float(np.float32(robotPose.y)) - float(oy)) * float(cpm)
    if not (rvx > -1.0 and rvx < w and rvy > -1.0 and rvy < h):
        return none
    fcell, owner = [], []
    for k, f in enumerate(fr):
        for x, y in f:                                   # global_position_to_grid_cell (grid_utils.hpp:33-38)
            fcell.append((int((float(x) - float(ox)) * float(cpm)), int((float(y) - float(oy)) * float(cpm))))
            owner.append(k)
    fcell = np.array(fcell, np.int64).reshape(-1, 2)
    on = (fcell[:, 0] >= 0) & (fcell[:, 0] < w) & (fcell[:, 1] >= 0) & (fcell[:, 1] < h)
    idx = np.flatnonzero(on)
    if len(idx) == 0:
        return none
    # every cell within reach of a frontier cell inside the grid, with the lowest index of such a frontier cell
    d = np.arange(-reach_cells, reach_cells + 1)         # arrays over (frontier cell, dy, dx); the 0 * terms only broadcast
    cx =(fcell[idx, 0][:, None, None] + d[None, None, :]) + 0 * d[None, :, None]
    cy = (fcell[idx, 1][:, None, None] + d[None, :, None]) + 0 * d[None, None, :]
    who = np.broadcast_to(idx[:, None, None], cx.shape)
    keep = (cx >= 0) & (cx < w) & (cy >= 0) & (cy < h) & (cx % stride == 0) & (cy % stride == 0)
    flat, who = (cy * w + cx)[keep], who[keep]
    if len(flat) == 0:
        return none
    order = np.lexsort((who, flat))                      # row-major, the lowest frontier cell first within a cell
    flat, who = flat[order], who[order]
    first = np.concatenate(([True], flat[1:] != flat[:-1]))
    flat, who = flat[first], who[first]
    cand = np.stack([flat % w, flat // w], axis=1).astype(np.int32)
    nf = NavigationField(ctx)
    vg = view or ViewGain(ctx=ctx)
    try:
        nf.compute(dist, nav_params(planner.searchParams_, obstacle_gain, 0), np.array([[int(rvx), int(rvy)]], np.int32))
        cost = nf.gather(cand)
        ok = cost != NAV_UNREACHED                       # UNREACHED also where the cell is not traversable
        cand, who, cost = cand[ok], who[ok], cost[ok].astype(np.int64)
        gain = vg.compute(grid, cand).astype(np.int64)
        ok = gain >= int(min_gain)
        cand, who, cost, gain = cand[ok], who[ok], cost[ok], gain[ok]
        if len(cand) == 0:
            return none
        u = int(gain_weight) * gain - cost
        best = np.lexsort((cand[:, 0], cand[:, 1], cost, -u))[0]
        nf.compute(dist, nav_params(planner.searchParams_, obstacle_gain, 0), cand[best:best + 1])
        paths, _, _ = nf.paths([robotPose], cap_each=cap)
    finally:
        nf.close()
        if view is None:
            vg.close()
    return paths[0], owner[int(who[best])], (int(cand[best, 0]), int(cand[best, 1])), int(gain[best]), int(cost[best])


# exploration_status_t (lcmtypes/exploration_status_t.lcm:3-11)
STATE_INITIALIZING, STATE_EXPLORING_MAP, STATE_RETURNING_HOME, STATE_COMPLETED_EXPLORATION, STATE_FAILED_EXPLORATION = 0, 1, 2, 3, 4
STATUS_IN_PROGRESS, STATUS_COMPLETE, STATUS_FAILED = 0, 1, 2


class ExploringMap:
    """Exploration::executeExploringMap (src/planning/exploration.cpp:277-369), the per-map step of the exploration loop,
    without its LCM calls: setMap (distance transform), find_map_frontiers, and -- when the robot is within 0.5 m of the
    current target or has none -- plan_path_to_frontier; then the status / next-state rule of :332-368.  The reference
    leaves status.status unset when frontiers remain but no path was found (:344-347 is commented out) and so falls into the
    default branch of :365-367: FAILED_EXPLORATION (definition D10; `status` then reports STATUS_FAILED)."""

    def __init__(self, planner):
        self.planner_ = planner
        self.currentTarget_ = make_pose(0.0, 0.0, 0.0)
        self.currentPath_ = []
        self.frontiers_ = None
        self.status = None

    def execute(self, currentMap, currentPose):
        self.planner_.setMap(currentMap)                                             # :299
        self.frontiers_ = find_map_frontiers(currentMap, currentPose)                # :300
        lists = self.frontiers_.cells()
        self.planner_.setNumFrontiers(len(lists))                                    # :302
        t = self.currentTarget_
        if t.x != 0 or t.y != 0:                                                      # :307-311: double pow/sqrt, stored to a float
            dx = float(np.float32(currentPose.x) - np.float32(t.x))
            dy = float(np.float32(currentPose.y) - np.float32(t.y))
            currDist = float(np.float32(np.sqrt(dx * dx + dy * dy)))
        else:
            currDist = 0.0
        if currDist <= float(np.float32(0.5)) and len(lists) > 0:                     # :316-321
            self.currentPath_ = plan_path_to_frontier(self.frontiers_, currentPose, currentMap, self.planner_)
            if len(self.currentPath_) > 1:
                p = self.currentPath_[-1]
                self.currentTarget_ = Pose(p.utime, p.x, p.y, p.theta)
        if len(lists) == 0:                                                           # :335-347
            self.status = STATUS_COMPLETE
        elif len(self.currentPath_) > 1:
            self.status = STATUS_IN_PROGRESS
        else:
            self.status = STATUS_FAILED                                               # D10
        return {STATUS_IN_PROGRESS: STATE_EXPLORING_MAP, STATUS_COMPLETE: STATE_RETURNING_HOME,
                STATUS_FAILED: STATE_FAILED_EXPLORATION}[self.status]                # :352-368


class AsyncExplorer:
    """bl_explorer: ExploringMap's step (exploration.cpp:277-369) on side streams -- submit(map, device pose) snapshots both on
    the SLAM stream; a lane runs setMap + find_map_frontiers against the snapshot; fetch() hands the steps back in order and
    applies the 0.5 m re-planning rule with the state they share, running plan_path_to_frontier on that lane when it is due."""

    def __init__(self, ctx=None, lanes=1, robotRadius=0.2):
        self.ctx = ctx or default_context()
        self.lanes = int(lanes)
        h = C.c_void_p()
        check(self.ctx.lib.bl_explorer_create(self.ctx.h, self.lanes, float(robotRadius), C.byref(h)))
        self.h = h
        self._buf = (Pose * 65536)()

    def submit(self, grid, pose_dev):
        check(self.ctx.lib.bl_explorer_submit(self.h, grid.h, pose_dev))

    def pending(self):
        return self.ctx.lib.bl_explorer_pending(self.h)

    def fetch(self, want_path=True):
        """-> (bl_explore_result_t as _capi.ExploreResult, currentPath_ as a list of poses or None)"""
        r = _capi.ExploreResult()
        check(self.ctx.lib.bl_explorer_fetch(self.h, C.byref(r), self._buf, 65536 if want_path else 0))
        path = [Pose(p.utime, p.x, p.y, p.theta) for p in self._buf[:min(r.path_length, 65536)]] if want_path else None
        return r, path

    def frontiers(self):
        h = C.c_void_p()
        check(self.ctx.lib.bl_explorer_frontiers(self.h, C.byref(h)))
        return Frontiers(self.ctx, h)

    def setState(self, target=None, prev_goal=None):
        check(self.ctx.lib.bl_explorer_set_state(self.h, C.byref(target) if target is not None else None,
                                                 C.byref(prev_goal) if prev_goal is not None else None))

    def close(self):
        if self.h:
            self.ctx.lib.bl_explorer_destroy(self.h)
            self.h = None


class AsyncPlanner:
    """bl_planner: MotionPlanner.setMap + planPath run on a second stream against a snapshot of the map and of the
    device-resident pose (the reference's planner process, src/planning/exploration.cpp:300-317)."""

    def __init__(self, ctx=None, params=None, lanes=1, batch=1):
        """lanes side streams; each collects `batch` submissions and searches them in one launch (bl_planner_create_batched)."""
        self.ctx = ctx or default_context()
        self.params_ = params or MotionPlannerParams()
        self.searchParams_ = SearchParams(self.params_.robotRadius, 10.0 * self.params_.robotRadius, 1.0)   # motion_planner.cpp:105-110
        self.lanes = int(lanes)
        h = C.c_void_p()
        self.batch = int(batch)
        check(self.ctx.lib.bl_planner_create_batched(self.ctx.h, self.lanes, self.batch, C.byref(h)))
        self.h = h
        self._buf = (Pose * 4097)()

    def submit(self, grid, start_dev, goal):
        check(self.ctx.lib.bl_planner_submit(self.h, grid.h, start_dev, C.byref(goal), C.byref(self.searchParams_)))

    def submit_with_map_update(self, mapping, scan, pose_dev, pose_utime, grid, goal):
        """mapping.updateMapDevicePose(scan, pose_dev, pose_utime, grid) then submit(grid, pose_dev, goal) as one library call
        (the map kernel leaves the snapshot behind on grids up to 256 K cells)."""
        c = scan.as_c()
        check(self.ctx.lib.bl_planner_submit_with_map_update(self.h, mapping.h, C.byref(c), pose_dev, int(pose_utime), grid.h,
                                                             C.byref(goal), C.byref(self.searchParams_)))

    def submit_with_map_update_finishing(self, mapping, scan, pf, pose_utime, grid, goal):
        """submit_with_map_update whose map kernel also ends the filter update begun with pf.updateBegin()."""
        c = scan.as_c()
        check(self.ctx.lib.bl_planner_submit_with_map_update_finishing_pf(self.h, mapping.h, C.byref(c), pf.h, int(pose_utime),
                                                                          grid.h, C.byref(goal), C.byref(self.searchParams_)))

    def fetch(self, return_stats=False):
        n = C.c_int()
        stats = (C.c_int64 * 2)()
        check(self.ctx.lib.bl_planner_fetch(self.h, self._buf, 4097, C.byref(n), stats))
        path = [Pose(p.utime, p.x, p.y, p.theta) for p in self._buf[:min(n.value, 4097)]]
        return (path, (stats[0], stats[1])) if return_stats else path

    def debugSnapshot(self, grid):
        """The cells of the snapshot the latest submission searched, shaped like `grid` (bl_planner_debug_snapshot)."""
        out = np.zeros((grid.height, grid.width), np.int8)
        check(self.ctx.lib.bl_planner_debug_snapshot(self.h, out.ctypes.data, out.size))
        return out

    def flush(self):
        """End of input: the batch every lane is still collecting goes out as it is (bl_planner_flush)."""
        check(self.ctx.lib.bl_planner_flush(self.h))

    def timing(self, on=-1):
        d, a, n = C.c_double(), C.c_double(), C.c_int64()
        check(self.ctx.lib.bl_planner_timing(self.h, on, C.byref(d), C.byref(a), C.byref(n)))
        return d.value, a.value, n.value

    def close(self):
        if self.h:
            self.ctx.lib.bl_planner_destroy(self.h)
            self.h = None


class MotionPlannerParams:
    def __init__(self, robotRadius=0.2):                                 # motion_planner.hpp:27-35
        self.robotRadius = float(robotRadius)


class MotionPlanner:
    """MotionPlanner (motion_planner.cpp:9-110): setMap, planPath, isValidGoal, setParams quirks included."""

    def __init__(self, params=None, ctx=None):
        self.params_ = params or MotionPlannerParams()
        self.distances_ = ObstacleDistanceGrid(ctx=ctx)
        self.searchParams_ = SearchParams()
        self.num_frontiers = 1           # uninitialised in the reference (motion_planner.hpp:164); callers set it
        self.prev_goal = make_pose(1e9, 1e9, 0.0)
        self.map_ = None
        self.metric_ = None              # setMetricClearance: a second, Euclidean grid for the field and the shortcut
        self.composed_ = None            # setMapWithObstacles: the planner's own grid of map and layer
        self.setParams(self.params_)

    def setParams(self, params):
        # motion_planner.cpp:105-110 reads params_ (the constructor's copy), not the argument
        self.searchParams_.minDistanceToObstacle = self.params_.robotRadius
        self.searchParams_.maxDistanceWithCost = 10.0 * self.searchParams_.minDistanceToObstacle
        self.searchParams_.distanceCostExponent = 1.0

    def setMap(self, grid):
        self.distances_.setDistances(grid)
        self.map_ = grid
        if self.metric_ is not None:
            self.metric_.setDistances(grid)

    def setMapWithObstacles(self, grid, layer):
        """setMap of `grid` with the cells an ObstacleLayer holds live written over it as occupied (127): composed into a grid the
        planner owns, then the ordinary setMap.  The caller's update comes first (layer.update(grid, scan, pose)); `grid` is untouched."""
        c = self.composed_
        if c is None or c.h is None or (c.width, c.height) != (grid.width, grid.height):
            if c is not None:
                c.close()
            c = None
        self.composed_ = layer.compose(grid, c)
        self.setMap(self.composed_)

    def setMapWithTracks(self, grid, layer, tracker, horizon, robot_pose, keep_clear=2):
        """setMapWithObstacles, with the cells that the tracker's confirmed moving tracks will cover within `horizon` updates occupied
        too (ObstacleTracker.compose), except within keep_clear cells of the robot's own cell.  The caller's layer.update and
        tracker.update come first."""
        c = self.composed_
        if c is None or c.h is None or (c.width, c.height) != (grid.width, grid.height):
            if c is not None:
                c.close()
            c = None
        assert tracker.layer is layer
        rx = int(math.floor((float(robot_pose.x) - float(grid.origin[0])) * float(grid.cpm)))
        ry = int(math.floor((float(robot_pose.y) - float(grid.origin[1])) * float(grid.cpm)))
        self.composed_ = tracker.compose(grid, c, horizon=horizon, robot_cell=(rx, ry), keep_clear=keep_clear)
        self.setMap(self.composed_)

    def setMapWithStaticObstacles(self, grid, layer, tracker):
        """setMapWithObstacles without the tracker's confirmed moving tracks (ObstacleTracker.composeStatic): the map for the field
        under LocalPlanner.commands_moving.  The caller's layer.update and tracker.update come first."""
        c = self.composed_
        if c is None or c.h is None or (c.width, c.height) != (grid.width, grid.height):
            if c is not None:
                c.close()
            c = None
        assert tracker.layer is layer
        self.composed_ = tracker.composeStatic(grid, c)
        self.setMap(self.composed_)

    def setMetricClearance(self, max_cells=64):
        """Metric clearance for planPathOptimal, shortcutPath and planPathShortcut: they read an exact Euclidean distance grid
        (capped at max_cells cells) beside the L1 grid, so that robotRadius means metres.  None turns it off (the default).  planPath,
        isValidGoal, isPathSafe and the frontier choosers stay on the L1 grid either way.  Takes effect with the next setMap (and at
        once for a map already set)."""
        if self.metric_ is not None:
            self.metric_.close()
            self.metric_ = None
        if max_cells is None:
            return
        self.metric_ = ObstacleDistanceGrid(ctx=self.distances_.ctx, metric="euclidean", max_cells=max_cells)
        if self.map_ is not None:
            self.metric_.setDistances(self.map_)

    def metricDistances(self):
        """The Euclidean grid of setMetricClearance (None while it is off)."""
        return self.metric_

    def _isValidGoalOn(self, distances, goal):
        # motion_planner.cpp:52-74
        dx = np.float32(goal.x) - np.float32(self.prev_goal.x)
        dy = np.float32(goal.y) - np.float32(self.prev_goal.y)
        dist_prev = np.sqrt(np.float32(dx * dx + dy * dy), dtype=np.float32)
        if self.num_frontiers != 1 and float(dist_prev) < 2 * self.searchParams_.minDistanceToObstacle:
            return False
        mpc, cpm, ox, oy = distances.frame()
        gx = int((float(np.float32(goal.x)) - float(ox)) * float(cpm))
        gy = int((float(np.float32(goal.y)) - float(oy)) * float(cpm))
        if distances.isCellInGrid(gx, gy):
            return float(distances(gx, gy)) > self.params_.robotRadius
        return False

    def setPrevGoal(self, goal): self.prev_goal = goal
    def setNumFrontiers(self, n): self.num_frontiers = int(n)

    def isValidGoal(self, goal):
        return self._isValidGoalOn(self.distances_, goal)

    def planPath(self, start, goal, searchParams=None, return_stats=False):
        if not self.isValidGoal(goal):
            failed = [Pose(start.utime, start.x, start.y, start.theta)]   # failedPath (motion_planner.cpp:28-40)
            return (failed, (0, 0)) if return_stats else failed
        return search_for_path(start, goal, self.distances_, searchParams or self.searchParams_, return_stats=return_stats)

    def planPathOptimal(self, start, goal, obstacle_gain=NAV_OBSTACLE_GAIN, return_cost=False, cap=1 << 16):
        """The cheapest 8-connected path to the goal's cell by the navigation field (bl_navfield_*): the failed path when isValidGoal
        fails, exactly as planPath; length 1 also when the goal cannot be reached."""
        dist = self.metric_ if self.metric_ is not None else self.distances_
        if not self._isValidGoalOn(dist, goal):
            failed = [Pose(start.utime, start.x, start.y, start.theta)]
            return (failed, NAV_UNREACHED) if return_cost else failed
        nf = NavigationField(dist.ctx)
        try:
            nf.computeToPose(dist, nav_params(self.searchParams_, obstacle_gain, 0), goal)
            paths, _, costs = nf.paths([start], cap_each=cap)
        finally:
            nf.close()
        return (paths[0], int(costs[0])) if return_cost else paths[0]

    def shortcutPath(self, path, clearance=None, max_span=64, waypoint_cost=1024):
        """Any-angle waypoints of a planPath / planPathOptimal result (PathShortcut); clearance None: minDistanceToObstacle."""
        sc = PathShortcut(self.distances_.ctx, clearance=self.searchParams_.minDistanceToObstacle if clearance is None else clearance,
                          max_span=max_span, waypoint_cost=waypoint_cost)
        try:
            return sc.shortcut(self.metric_ if self.metric_ is not None else self.distances_, path)
        finally:
            sc.close()

    def planPathShortcut(self, start, goal, clearance=None, max_span=64, waypoint_cost=1024):
        """planPathOptimal followed by shortcutPath."""
        return self.shortcutPath(self.planPathOptimal(start, goal), clearance, max_span, waypoint_cost)

    def isPathSafe(self, path):
        # motion_planner.cpp:77-96 (one gather for all poses); a pose outside the grid is unsafe
        mpc = np.float32(self.distances_.frame()[0])
        w, h = self.distances_.shape()
        q = np.zeros((len(path), 2), np.int32)
        for i, p in enumerate(path):
            q[i, 0] = int(np.float32(np.float32(p.x) / mpc) + np.float32(w // 2))
            q[i, 1] = int(np.float32(np.float32(p.y) / mpc) + np.float32(h // 2))
        out = np.zeros(len(path), np.float32)
        check(self.distances_.ctx.lib.bl_dist_gather(self.distances_.h, q.ctypes.data, len(path), out.ctypes.data))
        return bool(np.all(out > self.searchParams_.minDistanceToObstacle))


class ScanHistory:
    """Scan history and map rebuild (bl_scanlog_*, include/botlab_hip.h): the last `capacity` scans on the device -- kept rays,
    kept count, pose -- and rebuild(): the map that sequential Mapping.updateMap calls over a window of them would leave, at the
    recorded poses or at others, into any grid.  Index 0 is the oldest retained scan."""

    def __init__(self, capacity, max_rays=8192, ctx=None):
        self.ctx = ctx or default_context()
        h = C.c_void_p()
        check(self.ctx.lib.bl_scanlog_create(self.ctx.h, int(capacity), int(max_rays), C.byref(h)))
        self.h = h
        self.capacity, self.max_rays = int(capacity), int(max_rays)

    def __len__(self):
        return int(self.ctx.lib.bl_scanlog_size(self.h))

    def append(self, scan, pose):
        ls = scan.as_c()
        check(self.ctx.lib.bl_scanlog_append(self.h, C.byref(ls), C.byref(pose)))

    def append_device_pose(self, scan, d_pose_ptr, pose_utime):
        """x, y, theta read from a bl_pose_xyt_t in device memory (e.g. ParticleFilter.poseDevicePtr()), stream-ordered; utime given."""
        ls = scan.as_c()
        check(self.ctx.lib.bl_scanlog_append_dev_pose(self.h, C.byref(ls), d_pose_ptr, int(pose_utime)))

    def poses(self, first=0, count=None):
        """POSE_DTYPE [count]: the recorded poses of entries first .. first + count - 1 (count None: to the end)."""
        count = len(self) - first if count is None else int(count)
        out = np.zeros(max(count, 0), POSE_DTYPE)
        if count > 0:
            check(self.ctx.lib.bl_scanlog_get_poses(self.h, int(first), count, out.ctypes.data))
        return out

    def set_poses(self, first, poses):
        p = _pose_array(poses)
        check(self.ctx.lib.bl_scanlog_set_poses(self.h, int(first), len(p), p.ctypes.data))

    def scan(self, i):
        """(ranges, thetas, times) of entry i: its kept rays."""
        r, t, s = np.zeros(self.max_rays, np.float32), np.zeros(self.max_rays, np.float32), np.zeros(self.max_rays, np.int64)
        n = C.c_int()
        check(self.ctx.lib.bl_scanlog_get_scan(self.h, int(i), r.ctypes.data, t.ctypes.data, s.ctypes.data, C.byref(n)))
        return r[:n.value].copy(), t[:n.value].copy(), s[:n.value].copy()

    def rebuild(self, out, maxLaserDistance, hitOdds, missOdds, first=0, count=None, poses=None, prev_pose=None, base=None):
        """`out` becomes base (None: zeros) after Mapping(maxLaserDistance, hitOdds, missOdds).updateMap of entries first ..
        first + count - 1 in order, at `poses` (None: the recorded ones); prev_pose None: the first of them only latches its pose."""
        count = len(self) - first if count is None else int(count)
        p = None if poses is None else _pose_array(poses)
        assert p is None or len(p) == count
        check(self.ctx.lib.bl_scanlog_rebuild(self.h, int(first), count, None if p is None else p.ctypes.data,
                                              None if prev_pose is None else C.byref(prev_pose), C.c_float(maxLaserDistance), int(hitOdds),
                                              int(missOdds), None if base is None else base.h, out.h))

    def stats(self):
        s = _capi.ScanLogStats()
        check(self.ctx.lib.bl_scanlog_last_stats(self.h, C.byref(s)))
        return s

    def close(self):
        if self.h:
            self.ctx.lib.bl_scanlog_destroy(self.h)
            self.h = None


POSEGRAPH_EDGE_DTYPE = np.dtype([("i", "<i4"), ("j", "<i4"), ("z", "<f8", (3,)), ("info", "<f8", (6,))])
POSEGRAPH_RESULT_DTYPE = np.dtype([("cost_before", "<f8"), ("cost_after", "<f8"), ("final_lambda", "<f8"), ("tries", "<i4"), ("accepted", "<i4"),
                                   ("cg_iterations", "<i4"), ("status", "<i4")])
POSEGRAPH_CONVERGED_STEP, POSEGRAPH_CONVERGED_DECREASE, POSEGRAPH_OUT_OF_TRIES, POSEGRAPH_CG_CAP = 1, 2, 3, 16


def posegraph_params(fixed=0, max_tries=20, max_cg=500, lambda0=1e-6, lambda_up=10.0, lambda_down=0.1, step_tol=1e-6, rel_tol=1e-6, cg_tol=1e-8):
    """bl_posegraph_params_t.  The defaults are untuned: they end the loop graphs of the tests in 3 - 4 accepted steps."""
    return _capi.PoseGraphParams(int(fixed), int(max_tries), int(max_cg), 0, lambda0, lambda_up, lambda_down, step_tol, rel_tol, cg_tol)


def posegraph_edges(i, j, z, info):
    """POSEGRAPH_EDGE_DTYPE array of index arrays i, j, z (n, 3) and info (n, 6) or (6,): xx, xy, yy, xt, yt, tt."""
    i = np.asarray(i, np.int32).reshape(-1)
    e = np.zeros(len(i), POSEGRAPH_EDGE_DTYPE)
    e["i"], e["j"] = i, np.asarray(j, np.int32).reshape(-1)
    if len(i):
        e["z"] = np.asarray(z, np.float64).reshape(-1, 3)
        e["info"] = np.broadcast_to(np.asarray(info, np.float64), (len(i), 6))
    return e


class PoseGraph:
    """Pose-graph back end (bl_posegraph_*, include/botlab_hip.h, "pose graph"): nodes, a chain of odometry edges, loop edges, and
    solve(): one workgroup per subset of the loop edges, every subset in one launch.  The rules are the header's."""

    def __init__(self, max_nodes, max_loop_edges=0, max_subsets=1, ctx=None):
        self.ctx = ctx or default_context()
        h = C.c_void_p()
        check(self.ctx.lib.bl_posegraph_create(self.ctx.h, int(max_nodes), int(max_loop_edges), int(max_subsets), C.byref(h)))
        self.h = h
        self.n, self.n_loops, self.n_subsets = 0, 0, 0

    def set_nodes(self, poses):
        p = _pose_array(poses)
        check(self.ctx.lib.bl_posegraph_set_nodes(self.h, len(p), p.ctypes.data))
        self.n, self.n_loops = len(p), 0

    def set_nodes_from_log(self, history, first=0, count=None):
        count = len(history) - first if count is None else int(count)
        check(self.ctx.lib.bl_posegraph_set_nodes_from_log(self.h, history.h, int(first), count))
        self.n, self.n_loops = count, 0

    def set_chain(self, edges):
        e = np.ascontiguousarray(edges, POSEGRAPH_EDGE_DTYPE)
        assert len(e) == self.n - 1
        check(self.ctx.lib.bl_posegraph_set_chain(self.h, e.ctypes.data))

    def set_chain_from_nodes(self, info6):
        v = np.ascontiguousarray(info6, np.float64)
        assert v.shape == (6,)
        check(self.ctx.lib.bl_posegraph_set_chain_from_nodes(self.h, v.ctypes.data))

    def set_loops(self, edges):
        e = np.ascontiguousarray(edges, POSEGRAPH_EDGE_DTYPE)
        check(self.ctx.lib.bl_posegraph_set_loops(self.h, len(e), e.ctypes.data if len(e) else None))
        self.n_loops = len(e)

    def solve(self, params=None, masks=None):
        """masks: None (one subset, every loop edge on) or uint32 [n_subsets][(L + 31) // 32].  Enqueued; the readers wait."""
        prm = params if params is not None else posegraph_params()
        if masks is None:
            check(self.ctx.lib.bl_posegraph_solve(self.h, C.byref(prm), 1, None))
            self.n_subsets = 1
            return
        m = np.ascontiguousarray(masks, np.uint32)
        words = (self.n_loops + 31) // 32
        m = m.reshape(len(m), -1)[:, :words] if words else m.reshape(len(m), -1)[:, :0]
        m = np.ascontiguousarray(m)
        keep = m if m.size else np.zeros(1, np.uint32)
        check(self.ctx.lib.bl_posegraph_solve(self.h, C.byref(prm), len(m), keep.ctypes.data))
        self.n_subsets = len(m)

    def results(self):
        out = np.zeros(self.n_subsets, POSEGRAPH_RESULT_DTYPE)
        check(self.ctx.lib.bl_posegraph_results(self.h, out.ctypes.data))
        return out

    def poses(self, subset=0, want_double=False):
        """POSE_DTYPE [n] of a subset's result, narrowed once; with want_double also float64 [n][3]."""
        out = np.zeros(self.n, POSE_DTYPE)
        d = np.zeros((self.n, 3), np.float64) if want_double else None
        check(self.ctx.lib.bl_posegraph_poses(self.h, int(subset), out.ctypes.data, None if d is None else d.ctypes.data))
        return (out, d) if want_double else out

    def edge_chi2(self, subset=0):
        """(before, after): e' Omega e of every edge, chain first, at the nodes and at the subset's result."""
        b, a = np.zeros(self.n - 1 + self.n_loops), np.zeros(self.n - 1 + self.n_loops)
        check(self.ctx.lib.bl_posegraph_edge_chi2(self.h, int(subset), b.ctypes.data, a.ctypes.data))
        return b, a

    def poses_to_log(self, history, subset=0, first=0):
        check(self.ctx.lib.bl_posegraph_poses_to_log(self.h, int(subset), history.h, int(first)))

    def lastDeviceMs(self):
        ms = C.c_float()
        check(self.ctx.lib.bl_posegraph_last_device_ms(self.h, C.byref(ms)))
        return ms.value

    def close(self):
        if self.h:
            self.ctx.lib.bl_posegraph_destroy(self.h)
            self.h = None


def find_loop_closures(history, matcher, like_grid, stride=4, min_gap=40, radius=1.0, w=5, submap_cells=200, nx=8, ny=8, ntheta=12,
                       dtheta=math.radians(0.5), max_range=8.0, half_life=64, min_score=0, maxLaserDistance=5.0, hitOdds=3, missOdds=1):
    """Loop-edge candidates from what is already here, for PoseGraph.set_loops / close_loops.  For every stride-th scan q of the
    history: the older scans j < q - min_gap within `radius` metres of its recorded position, the nearest of them; the window
    [j - w, j + w] rebuilt into a local grid of submap_cells x submap_cells cells of like_grid's resolution centred on pose j;
    matcher.match_prior of scan q in it around its recorded pose, with moments.  A match is kept when it is accepted, has one best
    candidate (ties == 1) and that candidate is off the window's edge.  Its edge (i = j, j = q): z is the sub-cell matched pose seen
    from the recorded pose j; info is the inverse of the match's covariance (bl_scanmatch_covariance, turned into pose j's frame) plus
    diag(mpc^2 / 12, mpc^2 / 12, dtheta^2 / 12), the variance of the matcher's own quantisation, which keeps the matrix invertible
    when one candidate holds all the weight.  Returns a POSEGRAPH_EDGE_DTYPE array.

    min_gap, radius, w, submap_cells, the match window (nx, ny, ntheta, dtheta), half_life and min_score are untuned knobs."""
    n = len(history)
    poses = history.poses()
    mpc = float(like_grid.mpc)
    px, py = poses["x"].astype(np.float64), poses["y"].astype(np.float64)
    out = []
    for q in range(0, n, max(int(stride), 1)):
        last = q - int(min_gap) - 1                     # j < q - min_gap
        if last < 0:
            continue
        d2 = (px[:last + 1] - px[q]) ** 2 + (py[:last + 1] - py[q]) ** 2
        j = int(np.argmin(d2))
        if d2[j] > radius * radius:
            continue
        first, end = max(j - int(w), 0), min(j + int(w), n - 1)
        half = np.float32(submap_cells * mpc / 2.0)
        sub = OccupancyGrid(ctx=history.ctx, _raw=(int(submap_cells), int(submap_cells), like_grid.mpc, like_grid.cpm,
                                                   np.float32(poses["x"][j]) - half, np.float32(poses["y"][j]) - half))
        try:
            history.rebuild(sub, maxLaserDistance, hitOdds, missOdds, first=first, count=end - first + 1)
            r, t, s = history.scan(q)
            scan = LidarScan(r, t, s, utime=int(poses["utime"][q]))
            centre = make_pose(poses["x"][q], poses["y"][q], poses["theta"][q], utime=int(poses["utime"][q]))
            res, mom = matcher.match_prior(scan, centre, sub, half_life=half_life, nx=nx, ny=ny, ntheta=ntheta, dtheta=dtheta,
                                           max_range=max_range, min_score=min_score)
        finally:
            sub.close()
        if not (res.accepted and res.ties == 1 and abs(res.di) < nx and abs(res.dj) < ny and abs(res.dk) < ntheta):
            continue
        m = mom.refined_pose(res, centre, mpc, float(np.float32(dtheta)))
        _, cov = mom.covariance(mpc, float(np.float32(dtheta)))
        tj = float(poses["theta"][j])
        c, sn = math.cos(tj), math.sin(tj)
        dx, dy = float(m.x) - float(poses["x"][j]), float(m.y) - float(poses["y"][j])
        dth = float(m.theta) - tj
        z = (c * dx + sn * dy, -sn * dx + c * dy, math.atan2(math.sin(dth), math.cos(dth)))
        S = np.array([[cov[0], cov[1], cov[3]], [cov[1], cov[2], cov[4]], [cov[3], cov[4], cov[5]]])
        Rt = np.array([[c, sn, 0.0], [-sn, c, 0.0], [0.0, 0.0, 1.0]])
        S = Rt @ S @ Rt.T + np.diag([mpc * mpc / 12.0, mpc * mpc / 12.0, float(np.float32(dtheta)) ** 2 / 12.0])
        I = np.linalg.inv(S)
        I = 0.5 * (I + I.T)
        out.append((j, q, z, (I[0, 0], I[0, 1], I[1, 1], I[0, 2], I[1, 2], I[2, 2])))
    return posegraph_edges([e[0] for e in out], [e[1] for e in out], [e[2] for e in out] or np.zeros((0, 3)),
                           [e[3] for e in out] or np.zeros((0, 6)))


SCAN_MATCH_RESULT_DTYPE = np.dtype([("pose", POSE_DTYPE), ("di", "<i4"), ("dj", "<i4"), ("dk", "<i4"), ("score", "<i4"), ("score_centre", "<i4"),
                                    ("ties", "<i4"), ("rays_used", "<i4"), ("accepted", "<i4")])
SCAN_MATCH_MOMENTS_DTYPE = np.dtype([(n, "<i8") for n in ("s0", "sx", "sy", "st", "sxx", "sxy", "syy", "sxt", "syt", "stt")] +
                                    [("best_obj", "<i4"), ("pen_best", "<i4"), ("sub_num", "<i4", (3,)), ("sub_den", "<i4", (3,))])
LOOPCLOSE_CANDIDATE_DTYPE = np.dtype([("q", "<i4"), ("j", "<i4"), ("first", "<i4"), ("count", "<i4"), ("flags", "<u4"), ("pad", "<i4"),
                                      ("result", SCAN_MATCH_RESULT_DTYPE), ("moments", SCAN_MATCH_MOMENTS_DTYPE), ("edge", POSEGRAPH_EDGE_DTYPE)])
assert SCAN_MATCH_RESULT_DTYPE.itemsize == 56 and SCAN_MATCH_MOMENTS_DTYPE.itemsize == 112 and LOOPCLOSE_CANDIDATE_DTYPE.itemsize == 272
LOOPCLOSE_PLACE_DTYPE = np.dtype([(n, "<i4") for n in ("q", "j", "shift", "key", "overlap", "bits_q", "bits_j", "partner")])
assert LOOPCLOSE_PLACE_DTYPE.itemsize == 32
LC_NOT_ACCEPTED, LC_TIED, LC_ON_EDGE, LC_TOO_MANY_RAYS = _capi.LC_NOT_ACCEPTED, _capi.LC_TIED, _capi.LC_ON_EDGE, _capi.LC_TOO_MANY_RAYS


class LoopCloser:
    """Loop-closure front end on the device (bl_loopclose_*, include/botlab_hip.h, "loop closure"): find_loop_closures' pairs, submaps,
    matches and gate for every candidate in one sequence of launches, and the edges by the header's stated arithmetic.  find() returns
    the POSEGRAPH_EDGE_DTYPE array close_loops takes."""

    def __init__(self, max_candidates, ctx=None):
        self.ctx = ctx or default_context()
        h = C.c_void_p()
        check(self.ctx.lib.bl_loopclose_create(self.ctx.h, int(max_candidates), C.byref(h)))
        self.h = h
        self.n_candidates, self.submap_cells = 0, 0

    def find(self, history, like_grid, stride=4, min_gap=40, radius=1.0, w=5, submap_cells=200, nx=8, ny=8, ntheta=12,
             dtheta=math.radians(0.5), max_range=8.0, half_life=64, min_score=0, maxLaserDistance=5.0, hitOdds=3, missOdds=1,
             prior=(0, 0, 0, 0)):
        """The keyword names are find_loop_closures'; prior: the match's motion prior (a_xx, a_xy, a_yy, a_tt)."""
        match = _capi.ScanMatchParams(int(nx), int(ny), int(ntheta), float(np.float32(dtheta)), float(np.float32(max_range)), int(min_score), 0)
        pr = _capi.ScanMatchPrior(int(prior[0]), int(prior[1]), int(prior[2]), int(prior[3]), int(half_life), 1)
        prm = _capi.LoopCloseParams(int(stride), int(min_gap), float(np.float32(radius)), int(w), int(submap_cells),
                                    float(np.float32(maxLaserDistance)), int(hitOdds), int(missOdds), match, pr)
        m = C.c_int()
        check(self.ctx.lib.bl_loopclose_find(self.h, history.h, like_grid.h, C.byref(prm), C.byref(m)))
        self.n_candidates, self.submap_cells = m.value, int(submap_cells)
        return self.edges()

    def find_places(self, history, like_grid, bins_per_meter=4.0, place_max_range=8.0, dilate=1, min_key=16384, min_bits=8, stride=4,
                    min_gap=40, w=5, submap_cells=200, nx=8, ny=8, ntheta=12, dtheta=math.radians(0.5), max_range=8.0, half_life=64,
                    min_score=0, maxLaserDistance=5.0, hitOdds=3, missOdds=1, prior=(0, 0, 0, 0)):
        """find with the partner chosen by what the scans look like, not by where odometry says they were taken
        (bl_loopclose_find_places, include/botlab_hip.h, "loop closure by place recognition"): every scan's 64 x 32 bit descriptor,
        per query the older scan and circular shift of greatest overlap, the match centred on that scan's pose turned by the shift.
        The other keywords are find's; there is no radius.

        bins_per_meter, dilate, min_key and min_bits are untuned knobs."""
        match = _capi.ScanMatchParams(int(nx), int(ny), int(ntheta), float(np.float32(dtheta)), float(np.float32(max_range)), int(min_score), 0)
        pr = _capi.ScanMatchPrior(int(prior[0]), int(prior[1]), int(prior[2]), int(prior[3]), int(half_life), 1)
        prm = _capi.LoopCloseParams(int(stride), int(min_gap), 0.0, int(w), int(submap_cells), float(np.float32(maxLaserDistance)),
                                    int(hitOdds), int(missOdds), match, pr)
        pl = _capi.PlaceParams(float(np.float32(bins_per_meter)), float(np.float32(place_max_range)), int(dilate), int(min_key), int(min_bits))
        m = C.c_int()
        check(self.ctx.lib.bl_loopclose_find_places(self.h, history.h, like_grid.h, C.byref(prm), C.byref(pl), C.byref(m)))
        self.n_candidates, self.submap_cells = m.value, int(submap_cells)
        return self.edges()

    def places(self):
        """LOOPCLOSE_PLACE_DTYPE [queries]: q, j, shift, key, overlap, bits_q, bits_j, partner of the last find_places that launched."""
        n = C.c_int()
        check(self.ctx.lib.bl_loopclose_places(self.h, C.byref(n), None))
        out = np.zeros(n.value, LOOPCLOSE_PLACE_DTYPE)
        if n.value:
            check(self.ctx.lib.bl_loopclose_places(self.h, C.byref(n), out.ctypes.data))
        return out

    def descriptors(self):
        """(words uint32 [n][64], bits int32 [n]) of the n log entries of the last find_places that launched."""
        n = C.c_int()
        check(self.ctx.lib.bl_loopclose_descriptors(self.h, C.byref(n), None, None))
        words, bits = np.zeros((n.value, _capi.PLACE_SECTORS), np.uint32), np.zeros(n.value, np.int32)
        if n.value:
            check(self.ctx.lib.bl_loopclose_descriptors(self.h, C.byref(n), words.ctypes.data, bits.ctypes.data))
        return words, bits

    def edges(self):
        n = C.c_int()
        out = np.zeros(max(self.n_candidates, 1), POSEGRAPH_EDGE_DTYPE)
        check(self.ctx.lib.bl_loopclose_edges(self.h, C.byref(n), out.ctypes.data))
        return out[:n.value].copy()

    def candidates(self):
        """LOOPCLOSE_CANDIDATE_DTYPE [M]: q, j, first, count, flags, result, moments, edge of every candidate of the last find."""
        out = np.zeros(self.n_candidates, LOOPCLOSE_CANDIDATE_DTYPE)
        check(self.ctx.lib.bl_loopclose_candidates(self.h, out.ctypes.data if len(out) else None))
        return out

    def submap(self, m):
        """(cells int8 [S][S], origin float32 [2]) of candidate m's submap."""
        cells = np.zeros((self.submap_cells, self.submap_cells), np.int8)
        origin = np.zeros(2, np.float32)
        check(self.ctx.lib.bl_loopclose_submap(self.h, int(m), cells.ctypes.data, origin.ctypes.data))
        return cells, origin

    def lastDeviceMs(self, split=False):
        """Device time of the last find; with split also (pairs, rays + fold, match, records)."""
        ms, ms4 = C.c_float(), (C.c_float * 4)()
        check(self.ctx.lib.bl_loopclose_last_device_ms(self.h, C.byref(ms), ms4))
        return (ms.value, tuple(ms4)) if split else ms.value

    def close(self):
        if self.h:
            self.ctx.lib.bl_loopclose_destroy(self.h)
            self.h = None


def close_loops(history, graph, candidates, chain_info, gate=11.345, params=None):
    """Gate loop-edge candidates and correct the history's poses.  The nodes are the history's recorded poses, the chain is made from
    them with the information chain_info (xx, xy, yy, xt, yt, tt) on every edge.  One solve with L + 1 subsets: each candidate alone,
    and all together (the graph needs max_subsets >= L + 1).  A candidate whose alone-cost -- its Mahalanobis distance under the
    accumulated odometry -- exceeds `gate` is dropped (11.345: the 99 % point of chi2 with 3 degrees of freedom).  The survivors are
    solved once more, those whose own chi2 in the joint solution exceeds the gate are dropped, and if any fell the rest is solved
    again.  The poses are written to the history.  Returns (kept edges, results of the last solve, poses of it, alone costs).

    chain_info and the gate are untuned knobs."""
    cand = np.ascontiguousarray(candidates, POSEGRAPH_EDGE_DTYPE)
    L, n = len(cand), len(history)
    prm = params if params is not None else posegraph_params()
    graph.set_nodes_from_log(history, 0, n)
    graph.set_chain_from_nodes(chain_info)
    alone = np.zeros(0)
    kept = cand
    if L:
        graph.set_loops(cand)
        words = (L + 31) // 32
        masks = np.zeros((L + 1, words), np.uint32)
        for l in range(L):
            masks[l, l >> 5] = np.uint32(1) << np.uint32(l & 31)
            masks[L, l >> 5] |= np.uint32(1) << np.uint32(l & 31)
        graph.solve(prm, masks)
        alone = graph.results()["cost_after"][:L].copy()
        kept = cand[alone <= gate]
    graph.set_loops(kept)
    graph.solve(prm)
    if len(kept):
        own = graph.edge_chi2(0)[1][n - 1:]
        if np.any(own > gate):
            kept = kept[own <= gate]
            graph.set_loops(kept)
            graph.solve(prm)
    graph.poses_to_log(history, 0, 0)
    return kept, graph.results(), graph.poses(0), alone


def _pose_array(poses):
    """POSE_DTYPE array of a POSE_DTYPE array or of a sequence of Pose."""
    if isinstance(poses, np.ndarray) and poses.dtype == POSE_DTYPE:
        return np.ascontiguousarray(poses)
    out = np.zeros(len(poses), POSE_DTYPE)
    for i, q in enumerate(poses):
        out[i] = (int(q.utime), q.x, q.y, q.theta, 0.0)
    return out
