"""ctypes binding of libbotlab_hip.so (include/botlab_hip.h).  Loading fails loudly when the HIP library has not
been built: there is no CPU fallback anywhere in this package."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BOTLAB_HIP_LIB") or os.path.join(_HERE, "libbotlab_hip.so")   # BOTLAB_HIP_LIB: a diagnostic build (probes)


class Pose(C.Structure):
    """lcmtypes/pose_xyt_t.lcm (24 bytes)."""
    _fields_ = [("utime", C.c_int64), ("x", C.c_float), ("y", C.c_float), ("theta", C.c_float)]

    def __repr__(self):
        return f"Pose(utime={self.utime}, x={self.x!r}, y={self.y!r}, theta={self.theta!r})"


class Particle(C.Structure):
    """lcmtypes/particle_t.lcm (56 bytes)."""
    _fields_ = [("pose", Pose), ("parent_pose", Pose), ("weight", C.c_double)]


class Lidar(C.Structure):
    """lcmtypes/lidar_t.lcm, arrays as host pointers."""
    _fields_ = [("utime", C.c_int64), ("num_ranges", C.c_int32), ("ranges", C.POINTER(C.c_float)),
                ("thetas", C.POINTER(C.c_float)), ("times", C.POINTER(C.c_int64)),
                ("intensities", C.POINTER(C.c_float))]


class SearchParams(C.Structure):
    """src/planning/astar.hpp:15-27."""
    _fields_ = [("minDistanceToObstacle", C.c_double), ("maxDistanceWithCost", C.c_double),
                ("distanceCostExponent", C.c_double)]


class PfSpread(C.Structure):
    """bl_pf_spread_t: spread of the posterior (80 bytes)."""
    _fields_ = [("n_eff", C.c_double), ("mean_x", C.c_double), ("mean_y", C.c_double), ("var_x", C.c_double), ("var_y", C.c_double),
                ("cov_xy", C.c_double), ("theta_resultant", C.c_double), ("units_sum", C.c_uint64), ("units_sq_lo", C.c_uint64),
                ("units_sq_hi", C.c_uint64)]


class PfRecoveryParams(C.Structure):
    """bl_pf_recovery_params_t: kidnapped-robot recovery (48 bytes)."""
    _fields_ = [("alpha_slow", C.c_double), ("alpha_fast", C.c_double), ("ratio", C.c_double), ("max_fraction", C.c_double),
                ("min_dist", C.c_float), ("seed", C.c_uint64)]


class PfRecoveryState(C.Structure):
    """bl_pf_recovery_state_t: the recovery tracker (56 bytes)."""
    _fields_ = [("w_slow", C.c_double), ("w_fast", C.c_double), ("w_avg", C.c_double), ("p_inject", C.c_double),
                ("updates", C.c_uint32), ("primed", C.c_uint32), ("injected_last", C.c_uint32), ("pad", C.c_uint32),
                ("injected_total", C.c_uint64)]


class PfAdaptiveParams(C.Structure):
    """bl_pf_adaptive_params_t: adaptive particle count, KLD-sampling (40 bytes)."""
    _fields_ = [("min_particles", C.c_int32), ("pad", C.c_int32), ("epsilon", C.c_double), ("z", C.c_double),
                ("bin_xy", C.c_double), ("bin_theta", C.c_double)]


class PfAdaptiveState(C.Structure):
    """bl_pf_adaptive_state_t: active / next particle counts and the last count of bins (24 bytes)."""
    _fields_ = [("active", C.c_int32), ("next", C.c_int32), ("bins", C.c_uint32), ("k_sat", C.c_uint32), ("counts", C.c_uint64)]


class PfClusterParams(C.Structure):
    """bl_pf_cluster_params_t: bins and result size of bl_pf_clusters (16 bytes)."""
    _fields_ = [("bin_xy", C.c_double), ("theta_bins", C.c_int32), ("max_clusters", C.c_int32)]


class I128(C.Structure):
    """bl_i128_t: a signed 128-bit integer, hi * 2^64 + lo."""
    _fields_ = [("lo", C.c_uint64), ("hi", C.c_int64)]

    def value(self):
        return (int(self.hi) << 64) + int(self.lo)


PF_MAX_CLUSTERS = 64
PF_CLUSTER_SUMS = ("sx", "sy", "sxx", "syy", "sxy", "sc", "ss")


class PfCluster(C.Structure):
    """bl_pf_cluster_t: one cluster of the cloud, exact integer sums (144 bytes)."""
    _fields_ = ([("count", C.c_uint64), ("units", C.c_uint64)] + [(n, I128) for n in PF_CLUSTER_SUMS] +
                [("anchor_ix", C.c_int32), ("anchor_iy", C.c_int32), ("anchor_it", C.c_int32), ("pad", C.c_int32)])


class PfClusters(C.Structure):
    """bl_pf_clusters_t: what bl_pf_clusters reports (9240 bytes)."""
    _fields_ = [("num_clusters", C.c_uint64), ("units_sum", C.c_uint64), ("active", C.c_int32), ("pad", C.c_int32),
                ("clusters", PfCluster * PF_MAX_CLUSTERS)]


class PfClusterPose(C.Structure):
    """bl_pf_cluster_pose_t: a cluster's share, mean, covariance and heading in plain double (64 bytes)."""
    _fields_ = [("share", C.c_double), ("mean_x", C.c_double), ("mean_y", C.c_double), ("var_x", C.c_double), ("var_y", C.c_double),
                ("cov_xy", C.c_double), ("theta", C.c_double), ("theta_resultant", C.c_double)]


class ScanMatchParams(C.Structure):
    """bl_scan_match_params_t: the window of a correlative scan match (28 bytes)."""
    _fields_ = [("nx", C.c_int32), ("ny", C.c_int32), ("ntheta", C.c_int32), ("dtheta", C.c_float), ("max_range", C.c_float),
                ("min_score", C.c_int32), ("keep_volume", C.c_int32)]


class ScanMatchResult(C.Structure):
    """bl_scan_match_result_t: the best candidate of a correlative scan match (56 bytes)."""
    _fields_ = [("pose", Pose), ("di", C.c_int32), ("dj", C.c_int32), ("dk", C.c_int32), ("score", C.c_int32),
                ("score_centre", C.c_int32), ("ties", C.c_int32), ("rays_used", C.c_int32), ("accepted", C.c_int32)]

    def __repr__(self):
        return (f"ScanMatchResult(pose={self.pose!r}, di={self.di}, dj={self.dj}, dk={self.dk}, score={self.score}, "
                f"score_centre={self.score_centre}, ties={self.ties}, rays_used={self.rays_used}, accepted={self.accepted})")


class ScanMatchWideParams(C.Structure):
    """bl_scan_match_wide_params_t: the window of a wide (pruned) correlative scan match (32 bytes)."""
    _fields_ = [("nx", C.c_int32), ("ny", C.c_int32), ("ntheta", C.c_int32), ("dtheta", C.c_float), ("max_range", C.c_float),
                ("min_score", C.c_int32), ("block_log2", C.c_int32), ("exhaustive", C.c_int32)]


class ScanMatchWideStats(C.Structure):
    """bl_scan_match_wide_stats_t: what the last wide match pruned (40 bytes)."""
    _fields_ = [("candidates", C.c_int64), ("blocks", C.c_int64), ("blocks_kept", C.c_int64), ("candidates_scored", C.c_int64),
                ("block_log2", C.c_int32), ("path", C.c_int32)]

    def __repr__(self):
        return (f"ScanMatchWideStats(candidates={self.candidates}, blocks={self.blocks}, blocks_kept={self.blocks_kept}, "
                f"candidates_scored={self.candidates_scored}, block_log2={self.block_log2}, path={self.path})")


class ScanMatchPrior(C.Structure):
    """bl_scan_match_prior_t: the motion prior of a scan match and whether its moments are wanted (24 bytes)."""
    _fields_ = [("a_xx", C.c_int32), ("a_xy", C.c_int32), ("a_yy", C.c_int32), ("a_tt", C.c_int32), ("half_life", C.c_int32),
                ("want_moments", C.c_int32)]


class ScanMatchMoments(C.Structure):
    """bl_scan_match_moments_t: the weighted sums over a scan match's window, the best objective, the sub-cell fractions (112 bytes)."""
    _fields_ = [(n, C.c_int64) for n in ("s0", "sx", "sy", "st", "sxx", "sxy", "syy", "sxt", "syt", "stt")] + \
               [("best_obj", C.c_int32), ("pen_best", C.c_int32), ("sub_num", C.c_int32 * 3), ("sub_den", C.c_int32 * 3)]

    def sums(self):
        return tuple(int(getattr(self, n)) for n in ("s0", "sx", "sy", "st", "sxx", "sxy", "syy", "sxt", "syt", "stt"))

    def fractions(self):
        return tuple((int(self.sub_num[a]), int(self.sub_den[a])) for a in range(3))

    def covariance(self, meters_per_cell, dtheta):
        """(mean[3], cov[6] = xx, xy, yy, xt, yt, tt) in metres and radians: bl_scanmatch_covariance itself."""
        mean, cov = (C.c_double * 3)(), (C.c_double * 6)()
        load().bl_scanmatch_covariance(C.byref(self), float(meters_per_cell), float(dtheta), mean, cov)
        return tuple(mean), tuple(cov)

    def refined_pose(self, result, centre, meters_per_cell, dtheta):
        """The matched pose moved by the sub-cell fractions (the centre when the match was not accepted): bl_scanmatch_refined_pose."""
        out = Pose()
        load().bl_scanmatch_refined_pose(C.byref(result), C.byref(self), C.byref(centre), float(meters_per_cell), float(dtheta),
                                         C.byref(out))
        return out

    def __repr__(self):
        return f"ScanMatchMoments(sums={self.sums()}, best_obj={self.best_obj}, pen_best={self.pen_best}, fractions={self.fractions()})"


class NavFieldParams(C.Structure):
    """bl_navfield_params_t: the metric and the goal reach of a navigation field (32 bytes)."""
    _fields_ = [("minDistanceToObstacle", C.c_double), ("maxDistanceWithCost", C.c_double), ("distanceCostExponent", C.c_double),
                ("obstacle_gain", C.c_int32), ("reach_cells", C.c_int32)]


assert C.sizeof(Pose) == 24 and C.sizeof(Particle) == 56 and C.sizeof(PfSpread) == 80
assert C.sizeof(NavFieldParams) == 32


class ViewGainParams(C.Structure):
    """bl_viewgain_params_t: the ray fan and the cell classes of a view gain (20 bytes)."""
    _fields_ = [("radius_cells", C.c_int32), ("n_rays", C.c_int32), ("occupied_above", C.c_int32), ("unknown_lo", C.c_int32),
                ("unknown_hi", C.c_int32)]


assert C.sizeof(ViewGainParams) == 20


class LocalPlanState(C.Structure):
    """bl_localplan_state_t: a pose and the velocities the robot has now (32 bytes)."""
    _fields_ = [("pose", Pose), ("v", C.c_float), ("w", C.c_float)]


class LocalPlanParams(C.Structure):
    """bl_localplan_params_t: limits, candidate counts, horizon and the four weights of the local planner (56 bytes)."""
    _fields_ = [("v_min", C.c_float), ("v_max", C.c_float), ("w_max", C.c_float), ("acc_v", C.c_float), ("acc_w", C.c_float),
                ("dt_control", C.c_float), ("dt_sim", C.c_float), ("n_v", C.c_int32), ("n_w", C.c_int32), ("n_steps", C.c_int32),
                ("w_field", C.c_int32), ("w_heading", C.c_int32), ("w_clear", C.c_int32), ("w_speed", C.c_int32)]


class LocalPlanResult(C.Structure):
    """bl_localplan_result_t: the command of one state (32 bytes)."""
    _fields_ = [("trans_v", C.c_float), ("angular_v", C.c_float), ("index", C.c_int32), ("n_admissible", C.c_int32), ("cost", C.c_int64),
                ("flags", C.c_int32), ("pad", C.c_int32)]

    def __repr__(self):
        return (f"LocalPlanResult(trans_v={self.trans_v!r}, angular_v={self.angular_v!r}, index={self.index}, n_admissible={self.n_admissible}, "
                f"cost={self.cost}, flags={self.flags})")


class LocalPlanMoving(C.Structure):
    """bl_localplan_moving_t: how the rollout's steps relate to the tracker's updates, and the margin around a moving box (16 bytes)."""
    _fields_ = [("steps_per_update", C.c_int32), ("margin_cells", C.c_int32), ("lead_steps", C.c_int32), ("reserved", C.c_int32)]


assert C.sizeof(LocalPlanState) == 32 and C.sizeof(LocalPlanParams) == 56 and C.sizeof(LocalPlanResult) == 32
assert C.sizeof(LocalPlanMoving) == 16


class MppiParams(C.Structure):
    """bl_mppi_params_t: limits, noise, sample count, horizon, temperature, weights and seed of the sampling local planner (72 bytes)."""
    _fields_ = [("v_min", C.c_float), ("v_max", C.c_float), ("w_max", C.c_float), ("acc_v", C.c_float), ("acc_w", C.c_float),
                ("dt_sim", C.c_float), ("noise_v", C.c_float), ("noise_w", C.c_float), ("n_samples", C.c_int32), ("horizon", C.c_int32),
                ("n_sub", C.c_int32), ("lam", C.c_int32), ("w_field", C.c_int32), ("w_heading", C.c_int32), ("w_clear", C.c_int32),
                ("pad", C.c_int32), ("seed", C.c_uint64)]


class MppiState(C.Structure):
    """bl_mppi_state_t: a local planner state and the two Philox counter words of its draw (40 bytes)."""
    _fields_ = [("s", LocalPlanState), ("tick", C.c_uint32), ("stream", C.c_uint32)]


class MppiResult(C.Structure):
    """bl_mppi_result_t: the command of one state, the best sample, the costs and the weight sums (56 bytes)."""
    _fields_ = [("trans_v", C.c_float), ("angular_v", C.c_float), ("index_best", C.c_int32), ("n_admissible", C.c_int32),
                ("cost_best", C.c_int64), ("cost_out", C.c_int64), ("weight_sum", C.c_uint64), ("weight_sq_sum", C.c_uint64),
                ("flags", C.c_int32), ("pad", C.c_int32)]


assert C.sizeof(MppiParams) == 72 and C.sizeof(MppiState) == 40 and C.sizeof(MppiResult) == 56


class ShortcutParams(C.Structure):
    """bl_shortcut_params_t: clearance, longest span and the price of a waypoint of the path shortcutting (16 bytes)."""
    _fields_ = [("clearance", C.c_double), ("max_span", C.c_int32), ("waypoint_cost", C.c_int32)]


assert C.sizeof(ShortcutParams) == 16


class LFieldParams(C.Structure):
    """bl_lfield_params_t: sigma (metres), the cap in cells, the source threshold and the peak of the likelihood field (16 bytes)."""
    _fields_ = [("sigma", C.c_float), ("max_cells", C.c_int32), ("occ_min", C.c_int32), ("peak", C.c_int32)]


assert C.sizeof(LFieldParams) == 16


class ObsLayerParams(C.Structure):
    """bl_obslayer_params_t: the range cut, the occupancy threshold, the tolerance box, the time to live and the hits needed (20 bytes)."""
    _fields_ = [("max_range", C.c_float), ("occ_min", C.c_int32), ("tol_cells", C.c_int32), ("ttl_scans", C.c_int32), ("min_hits", C.c_int32)]


class ObsLayerStats(C.Structure):
    """bl_obslayer_stats_t: the counter, the last update's rays by class and its two sets, the live cells (40 bytes)."""
    _fields_ = [("n", C.c_uint32), ("valid_rays", C.c_int32), ("rays_by_class", C.c_int32 * 5), ("hit_cells", C.c_int32),
                ("cleared_cells", C.c_int32), ("live_cells", C.c_int32)]


assert C.sizeof(ObsLayerParams) == 20 and C.sizeof(ObsLayerStats) == 40


class BeamParams(C.Structure):
    """bl_beam_params_t: the beam model's range cut, mixture, tables' shapes, tempering span and ray stride (56 bytes)."""
    _fields_ = [("max_range", C.c_float), ("sigma_cells", C.c_float), ("z_hit", C.c_float), ("z_short", C.c_float), ("z_max", C.c_float),
                ("z_rand", C.c_float), ("lam", C.c_float), ("blocked_factor", C.c_float), ("occ_min", C.c_int32), ("hit_cut", C.c_int32),
                ("ray_stride", C.c_int32), ("pad", C.c_int32), ("span", C.c_int64)]


assert C.sizeof(BeamParams) == 56 and BeamParams.span.offset == 48


class RangeTableInfo(C.Structure):
    """bl_rangetable_info_t: the shape, headings, reach, occ_min and device bytes of a range table (32 bytes)."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("headings", C.c_int32), ("reach", C.c_int32), ("occ_min", C.c_int32),
                ("built", C.c_int32), ("bytes", C.c_int64)]


assert C.sizeof(RangeTableInfo) == 32 and RangeTableInfo.bytes.offset == 24


class ClearanceInfo(C.Structure):
    """bl_clearance_info_t: the shape, cap, occ_min and device bytes of a clearance grid (32 bytes)."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("cap", C.c_int32), ("occ_min", C.c_int32), ("built", C.c_int32),
                ("pad", C.c_int32), ("bytes", C.c_int64)]


assert C.sizeof(ClearanceInfo) == 32 and ClearanceInfo.bytes.offset == 24


class ScanLogStats(C.Structure):
    """bl_scanlog_stats_t: the launch shape and the device time of the last map rebuild (64 bytes)."""
    _fields_ = [("tiles", C.c_int64), ("chunks", C.c_int64), ("pairs", C.c_int64), ("scratch_bytes", C.c_int64), ("chunk_scans", C.c_int32),
                ("tile_cells", C.c_int32), ("scans", C.c_int32), ("pad", C.c_int32), ("ms_total", C.c_float), ("ms_geometry", C.c_float),
                ("ms_fold", C.c_float), ("ms_apply", C.c_float)]

    def __repr__(self):
        return (f"ScanLogStats(tiles={self.tiles}, chunks={self.chunks}, pairs={self.pairs}, scratch_bytes={self.scratch_bytes}, "
                f"chunk_scans={self.chunk_scans}, tile_cells={self.tile_cells}, scans={self.scans}, ms_total={self.ms_total:.4f}, "
                f"ms_geometry={self.ms_geometry:.4f}, ms_fold={self.ms_fold:.4f}, ms_apply={self.ms_apply:.4f})")


assert C.sizeof(ScanLogStats) == 64


class PoseGraphEdge(C.Structure):
    """bl_posegraph_edge_t: pose j seen from pose i is z, with information xx, xy, yy, xt, yt, tt (80 bytes)."""
    _fields_ = [("i", C.c_int32), ("j", C.c_int32), ("z", C.c_double * 3), ("info", C.c_double * 6)]


class PoseGraphParams(C.Structure):
    """bl_posegraph_params_t: the held node, the caps on tries and on conjugate-gradient iterations, lambda and the tolerances (64 bytes)."""
    _fields_ = [("fixed", C.c_int32), ("max_tries", C.c_int32), ("max_cg", C.c_int32), ("pad", C.c_int32), ("lambda0", C.c_double),
                ("lambda_up", C.c_double), ("lambda_down", C.c_double), ("step_tol", C.c_double), ("rel_tol", C.c_double), ("cg_tol", C.c_double)]


class PoseGraphResult(C.Structure):
    """bl_posegraph_result_t: costs, lambda, counters and status of one subset's solve (40 bytes)."""
    _fields_ = [("cost_before", C.c_double), ("cost_after", C.c_double), ("final_lambda", C.c_double), ("tries", C.c_int32),
                ("accepted", C.c_int32), ("cg_iterations", C.c_int32), ("status", C.c_int32)]

    def __repr__(self):
        return (f"PoseGraphResult(cost_before={self.cost_before!r}, cost_after={self.cost_after!r}, final_lambda={self.final_lambda!r}, "
                f"tries={self.tries}, accepted={self.accepted}, cg_iterations={self.cg_iterations}, status={self.status})")


assert C.sizeof(PoseGraphEdge) == 80 and C.sizeof(PoseGraphParams) == 64 and C.sizeof(PoseGraphResult) == 40


class LoopCloseParams(C.Structure):
    """bl_loopclose_params_t: the pair rule, the submap, the mapper's constants, the match window and its prior (84 bytes)."""
    _fields_ = [("stride", C.c_int32), ("min_gap", C.c_int32), ("radius", C.c_float), ("w", C.c_int32), ("submap_cells", C.c_int32),
                ("max_laser", C.c_float), ("hit", C.c_int32), ("miss", C.c_int32), ("match", ScanMatchParams), ("prior", ScanMatchPrior)]


class LoopCloseCandidate(C.Structure):
    """bl_loopclose_candidate_t: a candidate pair, its window, the gate's flags, the match and the edge (272 bytes)."""
    _fields_ = [("q", C.c_int32), ("j", C.c_int32), ("first", C.c_int32), ("count", C.c_int32), ("flags", C.c_uint32), ("pad", C.c_int32),
                ("result", ScanMatchResult), ("moments", ScanMatchMoments), ("edge", PoseGraphEdge)]


class PlaceParams(C.Structure):
    """bl_place_params_t: the descriptor's range bins and limit, the query's dilation, and the two thresholds (20 bytes)."""
    _fields_ = [("bins_per_meter", C.c_float), ("max_range", C.c_float), ("dilate", C.c_int32), ("min_key", C.c_int32),
                ("min_bits", C.c_int32)]


class Place(C.Structure):
    """bl_place_t: a query's best pair by the descriptors (32 bytes)."""
    _fields_ = [(n, C.c_int32) for n in ("q", "j", "shift", "key", "overlap", "bits_q", "bits_j", "partner")]


assert C.sizeof(PlaceParams) == 20 and C.sizeof(Place) == 32
PLACE_SECTORS, PLACE_BINS = 64, 32
assert C.sizeof(LoopCloseParams) == 84 and LoopCloseParams.match.offset == 32 and LoopCloseParams.prior.offset == 60
assert C.sizeof(LoopCloseCandidate) == 272 and LoopCloseCandidate.result.offset == 24 and LoopCloseCandidate.moments.offset == 80
assert LoopCloseCandidate.edge.offset == 192
LC_NOT_ACCEPTED, LC_TIED, LC_ON_EDGE, LC_TOO_MANY_RAYS = 1, 2, 4, 8


class ObsTracksParams(C.Structure):
    """bl_obstracks_params_t: blob area limits, the gate, the two filter gains, confirmation, coasting and the speed of "moving" (32 bytes)."""
    _fields_ = [("min_cells", C.c_int32), ("max_cells", C.c_int32), ("gate_cells", C.c_int32), ("alpha", C.c_int32), ("beta", C.c_int32),
                ("confirm_hits", C.c_int32), ("max_missed", C.c_int32), ("min_speed", C.c_int32)]


class ObsTracksCompose(C.Structure):
    """bl_obstracks_compose_t: how far ahead to stamp, and the box around the robot's cell that stays clear (16 bytes)."""
    _fields_ = [("horizon", C.c_int32), ("robot_x", C.c_int32), ("robot_y", C.c_int32), ("keep_clear", C.c_int32)]


class ObsTrack(C.Structure):
    """bl_obstrack_t: one slot (56 bytes)."""
    _fields_ = [("id", C.c_uint32), ("px", C.c_int32), ("py", C.c_int32), ("vx", C.c_int32), ("vy", C.c_int32), ("hits", C.c_int32),
                ("missed", C.c_int32), ("area", C.c_int32), ("x0", C.c_int32), ("y0", C.c_int32), ("x1", C.c_int32), ("y1", C.c_int32),
                ("flags", C.c_int32), ("slot", C.c_int32)]


class ObsBlob(C.Structure):
    """bl_obsblob_t: one blob of the last update (56 bytes)."""
    _fields_ = [("sum_x", C.c_int64), ("sum_y", C.c_int64), ("area", C.c_int32), ("x0", C.c_int32), ("y0", C.c_int32), ("x1", C.c_int32),
                ("y1", C.c_int32), ("cx", C.c_int32), ("cy", C.c_int32), ("eligible", C.c_int32), ("track", C.c_int32), ("rep", C.c_int32)]


class ObsTracksStats(C.Structure):
    """bl_obstracks_stats_t (56 bytes)."""
    _fields_ = [("n", C.c_uint32), ("next_id", C.c_uint32), ("live_cells", C.c_int32), ("blobs", C.c_int32), ("eligible", C.c_int32),
                ("dropped", C.c_int32), ("matched", C.c_int32), ("born", C.c_int32), ("deleted", C.c_int32), ("unborn", C.c_int32),
                ("tracks", C.c_int32), ("confirmed", C.c_int32), ("refused", C.c_int32), ("rounds", C.c_int32)]


class ObsTracksState(C.Structure):
    """bl_obstracks_state_t: the counters that go with the slots (16 bytes)."""
    _fields_ = [("n", C.c_uint32), ("next_id", C.c_uint32), ("fresh", C.c_int32), ("reserved", C.c_int32)]


assert C.sizeof(ObsTracksParams) == 32 and C.sizeof(ObsTracksCompose) == 16 and C.sizeof(ObsTrack) == 56 and C.sizeof(ObsBlob) == 56
assert C.sizeof(ObsTracksStats) == 56 and C.sizeof(ObsTracksState) == 16
OBSTRACK_DTYPE = [("id", "<u4"), ("px", "<i4"), ("py", "<i4"), ("vx", "<i4"), ("vy", "<i4"), ("hits", "<i4"), ("missed", "<i4"), ("area", "<i4"),
                  ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("flags", "<i4"), ("slot", "<i4")]
OBSBLOB_DTYPE = [("sum_x", "<i8"), ("sum_y", "<i8"), ("area", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("cx", "<i4"),
                 ("cy", "<i4"), ("eligible", "<i4"), ("track", "<i4"), ("rep", "<i4")]


class RBSlamResult(C.Structure):
    """bl_rbslam_result_t: what one update of the Rao-Blackwellized SLAM hands back (64 bytes)."""
    _fields_ = [("moved", C.c_int32), ("resampled", C.c_int32), ("best", C.c_int32), ("pad", C.c_int32), ("best_pose", Pose),
                ("S", C.c_uint64), ("Q_lo", C.c_uint64), ("Q_hi", C.c_uint64)]


class RBSlamMatchParams(C.Structure):
    """bl_rbslam_match_params_t: the window of the per-particle scan match of the Rao-Blackwellized SLAM (24 bytes)."""
    _fields_ = [("nx", C.c_int32), ("ny", C.c_int32), ("ntheta", C.c_int32), ("dtheta", C.c_float), ("max_range", C.c_float),
                ("min_score", C.c_int32)]


assert C.sizeof(RBSlamResult) == 64 and C.sizeof(RBSlamMatchParams) == 24
assert C.sizeof(ScanMatchParams) == 28 and C.sizeof(ScanMatchResult) == 56
assert C.sizeof(ScanMatchWideParams) == 32 and C.sizeof(ScanMatchWideStats) == 40
assert C.sizeof(ScanMatchPrior) == 24 and C.sizeof(ScanMatchMoments) == 112
assert C.sizeof(PfRecoveryParams) == 48 and C.sizeof(PfRecoveryState) == 56
assert C.sizeof(PfAdaptiveParams) == 40 and C.sizeof(PfAdaptiveState) == 24
assert C.sizeof(PfClusterParams) == 16 and C.sizeof(PfCluster) == 144 and C.sizeof(PfClusters) == 9240 and C.sizeof(PfClusterPose) == 64

class MotionPlannerState(C.Structure):
    """bl_motion_planner_t: the MotionPlanner members plan_path_to_frontier reads (motion_planner.hpp:153-165)."""
    _fields_ = [("robot_radius", C.c_double), ("search", SearchParams), ("num_frontiers", C.c_int32), ("prev_goal", Pose)]


class ExploreResult(C.Structure):
    """bl_explore_result_t: one Exploration::executeExploringMap step (exploration.cpp:277-369)."""
    _fields_ = [("next_state", C.c_int32), ("status", C.c_int32), ("num_frontiers", C.c_int32), ("frontier_cells", C.c_int32),
                ("planned", C.c_int32), ("path_length", C.c_int32), ("pops", C.c_int64), ("pushes", C.c_int64), ("searches", C.c_int64),
                ("bfs_cells", C.c_int32), ("bfs_levels", C.c_int32), ("pose", Pose), ("target", Pose), ("frontiers_ms", C.c_float),
                ("plan_ms", C.c_float)]


BL_K_MCL_MAIN, BL_K_MCL_SCAN, BL_K_MAP, BL_K_DIST, BL_K_ASTAR, BL_K_FRONTIERS = range(6)
BL_K_DIST_ROWS, BL_K_DIST_COLS_SUMMARY, BL_K_DIST_COLS_APPLY, BL_K_SNAPSHOT, BL_K_DIST_FUSED = range(6, 11)
BL_OK, BL_ERR_HIP, BL_ERR_ARG, BL_ERR_CAPACITY, BL_ERR_STATE = range(5)
BL_DIST_L1, BL_DIST_EUCLIDEAN = 0, 1
BL_EDT_MAX_CELLS = 254

_vp = C.c_void_p
_P = C.POINTER

# name -> (restype, argtypes); every symbol include/botlab_hip.h declares
SIGNATURES = {
    "bl_last_error": (C.c_char_p, []),
    "bl_version": (C.c_char_p, []),
    "bl_ctx_create": (C.c_int, [C.c_int, _vp, _P(_vp)]),
    "bl_ctx_destroy": (None, [_vp]),
    "bl_ctx_sync": (C.c_int, [_vp]),
    "bl_ctx_timing_enable": (C.c_int, [_vp, C.c_int]),
    "bl_ctx_timing_stride": (C.c_int, [_vp, C.c_int]),
    "bl_ctx_timing_get": (C.c_int, [_vp, C.c_int, _P(C.c_double), _P(C.c_int64)]),
    "bl_ctx_timing_reset": (C.c_int, [_vp]),
    "bl_grid_create": (C.c_int, [_vp, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, _P(_vp)]),
    "bl_grid_destroy": (None, [_vp]),
    "bl_grid_upload": (C.c_int, [_vp, _vp]),
    "bl_grid_download": (C.c_int, [_vp, _vp]),
    "bl_grid_reset": (C.c_int, [_vp]),
    "bl_grid_set_frame": (C.c_int, [_vp, C.c_float, C.c_float, C.c_float, C.c_float]),
    "bl_grid_copy": (C.c_int, [_vp, _vp]),
    "bl_grid_device_ptr": (_vp, [_vp]),
    "bl_grid_shape": (C.c_int, [_vp, _P(C.c_int), _P(C.c_int)]),
    "bl_mapping_create": (C.c_int, [_vp, C.c_float, C.c_int8, C.c_int8, _P(_vp)]),
    "bl_mapping_destroy": (None, [_vp]),
    "bl_mapping_update": (C.c_int, [_vp, _P(Lidar), _P(Pose), _vp]),
    "bl_mapping_update_dev_pose": (C.c_int, [_vp, _P(Lidar), _vp, C.c_int64, _vp]),
    "bl_pf_create": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _P(_vp)]),
    "bl_pf_destroy": (None, [_vp]),
    "bl_pf_set_exchange_buffers": (C.c_int, [_vp, _vp, _vp]),
    "bl_pf_exchange_rec_ptr": (_vp, [_vp]),
    "bl_pf_init_at_pose": (C.c_int, [_vp, _P(Pose), C.c_uint64]),
    "bl_pf_init_uniform": (C.c_int, [_vp, _vp, _vp, C.c_float, C.c_int64, C.c_uint64]),
    "bl_pf_spread": (C.c_int, [_vp, _P(PfSpread)]),
    "bl_pf_set_recovery": (C.c_int, [_vp, _vp, _vp, _P(PfRecoveryParams)]),
    "bl_pf_recovery_state": (C.c_int, [_vp, _P(PfRecoveryState)]),
    "bl_pf_set_adaptive": (C.c_int, [_vp, _P(PfAdaptiveParams)]),
    "bl_pf_adaptive_state": (C.c_int, [_vp, _P(PfAdaptiveState)]),
    "bl_pf_clusters": (C.c_int, [_vp, _P(PfClusterParams), _P(PfClusters), _vp]),
    "bl_pf_cluster_pose": (C.c_int, [_P(PfCluster), C.c_uint64, _P(PfClusterParams), _P(PfClusterPose)]),
    "bl_pf_set_particles": (C.c_int, [_vp, _vp, _vp]),
    "bl_pf_get_particles": (C.c_int, [_vp, _vp]),
    "bl_pf_set_noise_seed": (C.c_int, [_vp, C.c_uint64]),
    "bl_pf_update": (C.c_int, [_vp, _P(Pose), _P(Lidar), _vp, C.c_int, _vp, _P(Pose)]),
    "bl_pf_update_begin": (C.c_int, [_vp, _P(Pose), _P(Lidar), _vp, C.c_int, _vp, _P(C.c_int)]),
    "bl_pf_update_end": (C.c_int, [_vp, _P(Pose)]),
    "bl_pf_update_action_only": (C.c_int, [_vp, _P(Pose), _vp, _P(Pose)]),
    "bl_pf_pose_estimate": (C.c_int, [_vp, _P(Pose)]),
    "bl_pf_pose_device_ptr": (_vp, [_vp]),
    "bl_pf_estimate_posterior_pose": (C.c_int, [_vp, _vp]),
    "bl_pf_debug_estimate_stats": (C.c_int, [_vp, _vp]),
    "bl_pf_debug_lookahead": (C.c_int, [_vp, _vp]),
    "bl_pf_debug_set_finish_generation": (C.c_int, [_vp, C.c_uint32]),
    "bl_pf_set_strict_resampling": (C.c_int, [_vp, C.c_int]),
    "bl_pf_debug_resample": (C.c_int, [_vp, C.c_int, _vp]),
    "bl_pf_debug_enable": (C.c_int, [_vp, C.c_int]),
    "bl_pf_debug_last": (C.c_int, [_vp, _vp, _vp]),
    "bl_pf_debug_uniform_runs": (C.c_int, [_vp, _P(C.c_int)]),
    "bl_debug_trig_addition_probe": (C.c_int, [_vp, C.c_uint64, C.c_uint32, _P(C.c_float), _P(C.c_float), _P(C.c_float), _P(C.c_uint64)]),
    "bl_dist_create": (C.c_int, [_vp, _P(_vp)]),
    "bl_dist_destroy": (None, [_vp]),
    "bl_dist_set_distances": (C.c_int, [_vp, _vp]),
    "bl_dist_download": (C.c_int, [_vp, _vp]),
    "bl_dist_debug_stats": (C.c_int, [_vp, _vp]),
    "bl_dist_forget": (C.c_int, [_vp]),
    "bl_dist_debug_bound": (C.c_int, [_vp, _vp, _vp]),
    "bl_dist_debug_fused": (C.c_int, [_vp, _vp]),
    "bl_dist_shape": (C.c_int, [_vp, _P(C.c_int), _P(C.c_int)]),
    "bl_dist_frame": (C.c_int, [_vp, _P(C.c_float), _P(C.c_float), _P(C.c_float), _P(C.c_float)]),
    "bl_dist_device_ptr": (_vp, [_vp]),
    "bl_dist_create_euclidean": (C.c_int, [_vp, C.c_int, _P(_vp)]),
    "bl_dist_metric": (C.c_int, [_vp, _P(C.c_int), _P(C.c_int)]),
    "bl_dist_download_codes": (C.c_int, [_vp, _vp]),
    "bl_dist_table": (C.c_int, [_vp, _vp, _P(C.c_int)]),
    "bl_astar_search": (C.c_int, [_vp, _vp, _P(Pose), _P(Pose), _P(SearchParams), _vp, C.c_int, _P(C.c_int),
                                  _P(C.c_int64)]),
    "bl_astar_set_open_capacity": (C.c_int, [_vp, C.c_int64]),
    "bl_astar_debug_last_kernel": (C.c_int, [_vp]),
    "bl_debug_heap2_replay": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int64, _vp, _vp, _P(C.c_int), _vp]),
    "bl_astar_search_async": (C.c_int, [_vp, _vp, _P(Pose), _P(Pose), _P(SearchParams)]),
    "bl_astar_search_async_dev_start": (C.c_int, [_vp, _vp, _vp, _P(Pose), _P(SearchParams)]),
    "bl_astar_search_result": (C.c_int, [_vp, _vp, C.c_int, _P(C.c_int), _P(C.c_int64)]),
    "bl_planner_create": (C.c_int, [_vp, C.c_int, _P(_vp)]),
    "bl_planner_create_batched": (C.c_int, [_vp, C.c_int, C.c_int, _P(_vp)]),
    "bl_planner_destroy": (None, [_vp]),
    "bl_planner_submit": (C.c_int, [_vp, _vp, _vp, _P(Pose), _P(SearchParams)]),
    "bl_planner_debug_snapshot": (C.c_int, [_vp, _vp, C.c_int64]),
    "bl_planner_fetch": (C.c_int, [_vp, _vp, C.c_int, _P(C.c_int), _P(C.c_int64)]),
    "bl_planner_flush": (C.c_int, [_vp]),
    "bl_planner_timing": (C.c_int, [_vp, C.c_int, _P(C.c_double), _P(C.c_double), _P(C.c_int64)]),
    "bl_planner_submit_with_map_update": (C.c_int, [_vp, _vp, _P(Lidar), _vp, C.c_int64, _vp, _P(Pose), _P(SearchParams)]),
    "bl_mapping_update_finishing_pf": (C.c_int, [_vp, _P(Lidar), _vp, C.c_int64, _vp]),
    "bl_scan_prefetch": (C.c_int, [_vp, _P(Lidar)]),
    "bl_comm_load": (C.c_int, [C.c_char_p]),
    "bl_comm_unique_id": (C.c_int, [C.c_char_p, C.c_char_p]),
    "bl_comm_create": (C.c_int, [_vp, C.c_char_p, C.c_char_p, C.c_int, C.c_int, _P(_vp)]),
    "bl_comm_destroy": (None, [_vp]),
    "bl_comm_all_gather_inplace": (C.c_int, [_vp, _vp, C.c_size_t]),
    "bl_dev_enable_peer_access": (C.c_int, [C.c_int, C.c_int]),
    "bl_dev_alloc": (C.c_int, [_vp, C.c_size_t, _P(_vp)]),
    "bl_dev_word": (C.c_int, [_vp, _vp, C.c_int, _P(C.c_uint32)]),
    "bl_dev_free": (C.c_int, [_vp]),
    "bl_ipc_export": (C.c_int, [_vp, C.c_char_p]),
    "bl_ipc_open": (C.c_int, [C.c_char_p, _P(_vp)]),
    "bl_ipc_close": (C.c_int, [_vp]),
    "bl_pf_shard_setup": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int]),
    "bl_pf_shard_local_ptrs": (C.c_int, [_vp, _P(_vp), _P(_vp), _P(_vp)]),
    "bl_pf_shard_set_peer": (C.c_int, [_vp, C.c_int, _vp, _vp, _vp]),
    "bl_pf_shard_commit": (C.c_int, [_vp]),
    "bl_pf_shard_buffers": (C.c_int, [_vp, _P(_vp), _P(C.c_size_t), _P(_vp), _P(C.c_size_t)]),
    "bl_pf_shard_stage": (C.c_int, [_vp, C.c_int]),
    "bl_pf_shard_exchange": (C.c_int, [_vp, _vp]),
    "bl_pf_shard_traffic": (C.c_int, [_vp, _vp]),
    "bl_pf_shard_local_ptrs_peer": (C.c_int, [_vp, _P(_vp), _P(_vp), _P(_vp)]),
    "bl_pf_shard_set_peer_buffers": (C.c_int, [_vp, C.c_int, _vp, _vp, _vp]),
    "bl_pf_shard_peer_commit": (C.c_int, [_vp]),
    "bl_pf_shard_peer_active": (C.c_int, [_vp]),
    "bl_pf_shard_peer_selftest": (C.c_int, [_vp, _P(C.c_int)]),
    "bl_pf_shard_peer_reset": (C.c_int, [_vp, C.c_int]),
    "bl_pf_shard_exchange_peer": (C.c_int, [_vp]),
    "bl_pf_shard_exchange_peer_phase": (C.c_int, [_vp, C.c_int]),
    "bl_planner_submit_with_map_update_finishing_pf": (C.c_int, [_vp, _vp, _P(Lidar), _vp, C.c_int64, _vp, _P(Pose), _P(SearchParams)]),
    "bl_astar_search_batch": (C.c_int, [_vp, _vp, _P(Pose), _vp, C.c_int, _P(SearchParams), _vp, C.c_int, _vp, _vp]),
    "bl_dist_gather": (C.c_int, [_vp, _vp, C.c_int, _vp]),
    "bl_frontiers_find": (C.c_int, [_vp, _vp, _P(Pose), C.c_double, _P(_vp)]),
    "bl_frontiers_from_host": (C.c_int, [_vp, C.c_int, _vp, _P(_vp)]),
    "bl_frontiers_count": (C.c_int, [_vp]),
    "bl_frontiers_total_cells": (C.c_int, [_vp]),
    "bl_frontiers_get": (C.c_int, [_vp, _vp, _vp]),
    "bl_frontiers_stats": (C.c_int, [_vp, _P(C.c_int), _P(C.c_int)]),
    "bl_frontiers_debug_sweep_kernel": (C.c_int, [_vp]),
    "bl_frontiers_destroy": (None, [_vp]),
    "bl_scanmatch_create": (C.c_int, [_vp, _P(_vp)]),
    "bl_scanmatch_destroy": (None, [_vp]),
    "bl_scanmatch_match": (C.c_int, [_vp, _vp, _P(Lidar), _P(Pose), _P(ScanMatchParams), _P(ScanMatchResult)]),
    "bl_scanmatch_volume": (C.c_int, [_vp, _vp]),
    "bl_scanmatch_debug_path": (C.c_int, [_vp]),
    "bl_scanmatch_match_wide": (C.c_int, [_vp, _vp, _P(Lidar), _P(Pose), _P(ScanMatchWideParams), _P(ScanMatchResult)]),
    "bl_scanmatch_wide_stats": (C.c_int, [_vp, _P(ScanMatchWideStats)]),
    "bl_scanmatch_match_prior": (C.c_int, [_vp, _vp, _P(Lidar), _P(Pose), _P(ScanMatchParams), _P(ScanMatchPrior),
                                           _P(ScanMatchResult), _P(ScanMatchMoments)]),
    "bl_scanmatch_covariance": (None, [_P(ScanMatchMoments), C.c_double, C.c_double, _P(C.c_double), _P(C.c_double)]),
    "bl_scanmatch_refined_pose": (None, [_P(ScanMatchResult), _P(ScanMatchMoments), _P(Pose), C.c_double, C.c_double, _P(Pose)]),
    "bl_navfield_create": (C.c_int, [_vp, _P(_vp)]),
    "bl_navfield_destroy": (None, [_vp]),
    "bl_navfield_compute": (C.c_int, [_vp, _vp, _P(NavFieldParams), _vp, C.c_int]),
    "bl_navfield_compute_to_pose": (C.c_int, [_vp, _vp, _P(NavFieldParams), _P(Pose)]),
    "bl_navfield_paths": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, _vp, _vp, _vp]),
    "bl_navfield_gather": (C.c_int, [_vp, _vp, C.c_int, _vp]),
    "bl_navfield_download": (C.c_int, [_vp, _vp]),
    "bl_navfield_shape": (C.c_int, [_vp, _P(C.c_int), _P(C.c_int)]),
    "bl_navfield_device_ptr": (_vp, [_vp]),
    "bl_navfield_tables": (C.c_int, [_vp, _vp, _vp, _P(C.c_int)]),
    "bl_navfield_stats": (C.c_int, [_vp, _vp]),
    "bl_localplan_create": (C.c_int, [_vp, _P(_vp)]),
    "bl_localplan_destroy": (None, [_vp]),
    "bl_localplan_set_params": (C.c_int, [_vp, _P(LocalPlanParams)]),
    "bl_localplan_commands": (C.c_int, [_vp, _vp, _vp, C.c_int, _vp]),
    "bl_localplan_debug_costs": (C.c_int, [_vp, _vp, _P(LocalPlanState), _vp]),
    "bl_localplan_debug_rollout": (C.c_int, [_vp, _vp, _P(LocalPlanState), C.c_int, _vp]),
    "bl_localplan_tables": (C.c_int, [_vp, _P(LocalPlanState), _vp, _vp]),
    "bl_localplan_debug_path": (C.c_int, [_vp]),
    "bl_localplan_last_device_ms": (C.c_int, [_vp, _P(C.c_float)]),
    "bl_localplan_commands_moving": (C.c_int, [_vp, _vp, _vp, _P(LocalPlanMoving), _vp, C.c_int, _vp]),
    "bl_localplan_debug_costs_moving": (C.c_int, [_vp, _vp, _vp, _P(LocalPlanMoving), _P(LocalPlanState), _vp, _vp]),
    "bl_localplan_debug_moving_path": (C.c_int, [_vp]),
    "bl_mppi_create": (C.c_int, [_vp, _P(_vp)]),
    "bl_mppi_destroy": (None, [_vp]),
    "bl_mppi_set_params": (C.c_int, [_vp, _P(MppiParams)]),
    "bl_mppi_plan": (C.c_int, [_vp, _vp, _vp, _P(LocalPlanMoving), _vp, C.c_int, _vp, _vp, _vp]),
    "bl_mppi_debug_samples": (C.c_int, [_vp, _vp, _vp, _P(LocalPlanMoving), _P(MppiState), _vp, _vp, _vp, _vp]),
    "bl_mppi_debug_rollout": (C.c_int, [_vp, _vp, _P(MppiState), _vp, _vp]),
    "bl_mppi_weight_table": (None, [_vp]),
    "bl_mppi_debug_path": (C.c_int, [_vp]),
    "bl_mppi_last_device_ms": (C.c_int, [_vp, _P(C.c_float)]),
    "bl_beam_create": (C.c_int, [_vp, _P(_vp)]),
    "bl_beam_destroy": (None, [_vp]),
    "bl_beam_set_params": (C.c_int, [_vp, _P(BeamParams)]),
    "bl_beam_tables": (C.c_int, [_vp, C.c_float, _vp, _vp, _vp, _vp]),
    "bl_beam_unit_table": (None, [_vp]),
    "bl_beam_scores": (C.c_int, [_vp, _vp, _P(Lidar), _vp, C.c_int, _vp]),
    "bl_beam_debug_cast": (C.c_int, [_vp, _vp, _P(Lidar), _P(Pose), _vp, _vp, _vp, _vp, _vp]),
    "bl_beam_reweigh_pf": (C.c_int, [_vp, _vp, _vp, _P(Lidar), _P(Pose)]),
    "bl_beam_units": (C.c_int, [_vp, _vp, C.c_int]),
    "bl_beam_last_rays": (C.c_int, [_vp]),
    "bl_beam_debug_set": (C.c_int, [_vp, C.c_int, C.c_int]),
    "bl_beam_debug_path": (C.c_int, [_vp]),
    "bl_beam_last_device_ms": (C.c_int, [_vp, _P(C.c_float)]),
    "bl_rangetable_create": (C.c_int, [_vp, C.c_int, _P(_vp)]),
    "bl_rangetable_destroy": (None, [_vp]),
    "bl_rangetable_build": (C.c_int, [_vp, _vp, _vp]),
    "bl_rangetable_update": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int]),
    "bl_rangetable_read": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp]),
    "bl_rangetable_directions": (C.c_int, [_vp, _vp]),
    "bl_rangetable_info": (C.c_int, [_vp, _P(RangeTableInfo)]),
    "bl_rangetable_last_device_ms": (C.c_int, [_vp, _P(C.c_float)]),
    "bl_rangetable_scores": (C.c_int, [_vp, _vp, _P(Lidar), _vp, C.c_int, _vp]),
    "bl_rangetable_reweigh_pf": (C.c_int, [_vp, _vp, _vp, _P(Lidar), _P(Pose)]),
    "bl_rangetable_debug_lookup": (C.c_int, [_vp, _vp, _P(Lidar), _P(Pose), _vp, _vp, _vp, _vp]),
    "bl_clearance_create": (C.c_int, [_vp, C.c_int, _P(_vp)]),
    "bl_clearance_destroy": (None, [_vp]),
    "bl_clearance_build": (C.c_int, [_vp, _vp, C.c_int]),
    "bl_clearance_update": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int]),
    "bl_clearance_read": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp]),
    "bl_clearance_info": (C.c_int, [_vp, _P(ClearanceInfo)]),
    "bl_clearance_last_device_ms": (C.c_int, [_vp, _P(C.c_float)]),
    "bl_clearance_scores": (C.c_int, [_vp, _vp, _P(Lidar), _vp, C.c_int, _vp]),
    "bl_clearance_reweigh_pf": (C.c_int, [_vp, _vp, _vp, _P(Lidar), _P(Pose)]),
    "bl_clearance_debug_cast": (C.c_int, [_vp, _vp, _P(Lidar), _P(Pose), _vp, _vp, _vp, _vp, _vp, _vp]),
    "bl_scanlog_create": (C.c_int, [_vp, C.c_int, C.c_int, _P(_vp)]),
    "bl_scanlog_destroy": (None, [_vp]),
    "bl_scanlog_append": (C.c_int, [_vp, _P(Lidar), _P(Pose)]),
    "bl_scanlog_append_dev_pose": (C.c_int, [_vp, _P(Lidar), _vp, C.c_int64]),
    "bl_scanlog_size": (C.c_int, [_vp]),
    "bl_scanlog_get_poses": (C.c_int, [_vp, C.c_int, C.c_int, _vp]),
    "bl_scanlog_set_poses": (C.c_int, [_vp, C.c_int, C.c_int, _vp]),
    "bl_scanlog_get_scan": (C.c_int, [_vp, C.c_int, _vp, _vp, _vp, _P(C.c_int)]),
    "bl_scanlog_rebuild": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _P(Pose), C.c_float, C.c_int8, C.c_int8, _vp, _vp]),
    "bl_scanlog_last_stats": (C.c_int, [_vp, _P(ScanLogStats)]),
    "bl_posegraph_create": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _P(_vp)]),
    "bl_posegraph_destroy": (None, [_vp]),
    "bl_posegraph_set_nodes": (C.c_int, [_vp, C.c_int, _vp]),
    "bl_posegraph_set_nodes_from_log": (C.c_int, [_vp, _vp, C.c_int, C.c_int]),
    "bl_posegraph_set_chain": (C.c_int, [_vp, _vp]),
    "bl_posegraph_set_chain_from_nodes": (C.c_int, [_vp, _vp]),
    "bl_posegraph_set_loops": (C.c_int, [_vp, C.c_int, _vp]),
    "bl_posegraph_solve": (C.c_int, [_vp, _P(PoseGraphParams), C.c_int, _vp]),
    "bl_posegraph_results": (C.c_int, [_vp, _vp]),
    "bl_posegraph_poses": (C.c_int, [_vp, C.c_int, _vp, _vp]),
    "bl_posegraph_edge_chi2": (C.c_int, [_vp, C.c_int, _vp, _vp]),
    "bl_posegraph_poses_to_log": (C.c_int, [_vp, C.c_int, _vp, C.c_int]),
    "bl_posegraph_last_device_ms": (C.c_int, [_vp, _P(C.c_float)]),
    "bl_loopclose_create": (C.c_int, [_vp, C.c_int, _P(_vp)]),
    "bl_loopclose_destroy": (None, [_vp]),
    "bl_loopclose_find": (C.c_int, [_vp, _vp, _vp, _P(LoopCloseParams), _P(C.c_int)]),
    "bl_loopclose_candidates": (C.c_int, [_vp, _vp]),
    "bl_loopclose_edges": (C.c_int, [_vp, _P(C.c_int), _vp]),
    "bl_loopclose_submap": (C.c_int, [_vp, C.c_int, _vp, _vp]),
    "bl_loopclose_last_device_ms": (C.c_int, [_vp, _P(C.c_float), _vp]),
    "bl_loopclose_find_places": (C.c_int, [_vp, _vp, _vp, _P(LoopCloseParams), _P(PlaceParams), _P(C.c_int)]),
    "bl_loopclose_places": (C.c_int, [_vp, _P(C.c_int), _vp]),
    "bl_loopclose_descriptors": (C.c_int, [_vp, _P(C.c_int), _vp, _vp]),
    "bl_shortcut_create": (C.c_int, [_vp, _P(_vp)]),
    "bl_shortcut_destroy": (None, [_vp]),
    "bl_shortcut_set_params": (C.c_int, [_vp, _P(ShortcutParams)]),
    "bl_shortcut_cells": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, _vp, _vp, _vp]),
    "bl_shortcut_poses": (C.c_int, [_vp, _vp, _vp, C.c_int, _vp, C.c_int, _vp, _vp, _vp]),
    "bl_shortcut_debug_visible": (C.c_int, [_vp, _vp, _vp, C.c_int, _vp]),
    "bl_shortcut_debug_path": (C.c_int, [_vp]),
    "bl_shortcut_last_device_ms": (C.c_int, [_vp, _P(C.c_float), _P(C.c_float)]),
    "bl_lfield_create": (C.c_int, [_vp, _P(_vp)]),
    "bl_lfield_destroy": (None, [_vp]),
    "bl_lfield_set_params": (C.c_int, [_vp, _P(LFieldParams)]),
    "bl_lfield_compute": (C.c_int, [_vp, _vp]),
    "bl_lfield_grid": (_vp, [_vp]),
    "bl_lfield_table": (C.c_int, [_vp, _vp, _P(C.c_int)]),
    "bl_lfield_last_device_ms": (C.c_int, [_vp, _P(C.c_float)]),
    "bl_obslayer_create": (C.c_int, [_vp, C.c_int, C.c_int, _P(_vp)]),
    "bl_obslayer_destroy": (None, [_vp]),
    "bl_obslayer_set_params": (C.c_int, [_vp, _P(ObsLayerParams)]),
    "bl_obslayer_reset": (C.c_int, [_vp]),
    "bl_obslayer_update": (C.c_int, [_vp, _vp, _P(Lidar), _P(Pose)]),
    "bl_obslayer_compose": (C.c_int, [_vp, _vp, _vp]),
    "bl_obslayer_classes": (C.c_int, [_vp, _vp, _P(C.c_int)]),
    "bl_obslayer_stats": (C.c_int, [_vp, _P(ObsLayerStats)]),
    "bl_obslayer_live_cells": (C.c_int, [_vp, _vp, C.c_int, _P(C.c_int)]),
    "bl_obslayer_download": (C.c_int, [_vp, _vp, _vp, _P(C.c_uint32)]),
    "bl_obslayer_upload": (C.c_int, [_vp, _vp, _vp, C.c_uint32]),
    "bl_obslayer_last_device_ms": (C.c_int, [_vp, _P(C.c_float), _P(C.c_float)]),
    "bl_obstracks_create": (C.c_int, [_vp, C.c_int, C.c_int, _P(_vp)]),
    "bl_obstracks_destroy": (None, [_vp]),
    "bl_obstracks_set_params": (C.c_int, [_vp, _P(ObsTracksParams)]),
    "bl_obstracks_reset": (C.c_int, [_vp]),
    "bl_obstracks_update": (C.c_int, [_vp, _vp]),
    "bl_obstracks_compose": (C.c_int, [_vp, _vp, _vp, _vp, _P(ObsTracksCompose)]),
    "bl_obstracks_compose_static": (C.c_int, [_vp, _vp, _vp, _vp]),
    "bl_obstracks_tracks": (C.c_int, [_vp, _vp, C.c_int, _P(C.c_int)]),
    "bl_obstracks_blobs": (C.c_int, [_vp, _vp, C.c_int, _P(C.c_int)]),
    "bl_obstracks_labels": (C.c_int, [_vp, _vp, C.c_int, _P(C.c_int)]),
    "bl_obstracks_stats": (C.c_int, [_vp, _P(ObsTracksStats)]),
    "bl_obstracks_download": (C.c_int, [_vp, _vp, _P(ObsTracksState)]),
    "bl_obstracks_upload": (C.c_int, [_vp, _vp, _P(ObsTracksState)]),
    "bl_obstracks_last_device_ms": (C.c_int, [_vp, _P(C.c_float), _P(C.c_float)]),
    "bl_viewgain_create": (C.c_int, [_vp, _P(_vp)]),
    "bl_viewgain_destroy": (None, [_vp]),
    "bl_viewgain_set_params": (C.c_int, [_vp, _P(ViewGainParams)]),
    "bl_viewgain_ray_ends": (C.c_int, [_vp, _vp, _P(C.c_int)]),
    "bl_viewgain_compute": (C.c_int, [_vp, _vp, _vp, C.c_int, _vp]),
    "bl_viewgain_debug_seen": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp]),
    "bl_rbslam_create": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int8, C.c_int8,
                                   _P(_vp)]),
    "bl_rbslam_destroy": (None, [_vp]),
    "bl_rbslam_set_resampling": (C.c_int, [_vp, C.c_uint32, C.c_uint32]),
    "bl_rbslam_set_noise_seed": (C.c_int, [_vp, C.c_uint64]),
    "bl_rbslam_init_at_pose": (C.c_int, [_vp, _P(Pose), C.c_uint64]),
    "bl_rbslam_set_particles": (C.c_int, [_vp, _vp, _vp]),
    "bl_rbslam_get_particles": (C.c_int, [_vp, _vp, _vp, _vp]),
    "bl_rbslam_update": (C.c_int, [_vp, _P(Pose), _P(Lidar), C.c_int, _vp, _P(RBSlamResult)]),
    "bl_rbslam_map_download": (C.c_int, [_vp, C.c_int, _vp]),
    "bl_rbslam_map_upload": (C.c_int, [_vp, C.c_int, _vp]),
    "bl_rbslam_best_map": (C.c_int, [_vp, _vp]),
    "bl_rbslam_debug_last": (C.c_int, [_vp, _vp, _vp]),
    "bl_rbslam_set_scan_matching": (C.c_int, [_vp, _P(RBSlamMatchParams)]),
    "bl_rbslam_debug_match": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "bl_rbslam_debug_match_path": (C.c_int, [_vp]),
    "bl_lcm_fingerprint": (C.c_uint64, [C.c_int]),
    "bl_lcm_encode_pose": (C.c_int64, [C.c_int, _P(Pose), _vp, C.c_int64]),
    "bl_lcm_encode_lidar": (C.c_int64, [_P(Lidar), _vp, _vp, C.c_int64]),
    "bl_lcm_encode_particles": (C.c_int64, [C.c_int64, _vp, C.c_int32, _vp, C.c_int64]),
    "bl_lcm_encode_grid": (C.c_int64, [C.c_int64, C.c_float, C.c_float, C.c_float, C.c_int32, C.c_int32, _vp, _vp, C.c_int64]),
    "bl_lcm_encode_path": (C.c_int64, [C.c_int64, _vp, C.c_int32, _vp, C.c_int64]),
    "bl_lcm_decode_pose": (C.c_int, [C.c_int, _vp, C.c_int64, _P(Pose)]),
    "bl_lcm_decode_lidar": (C.c_int, [_vp, C.c_int64, _P(C.c_int64), _P(C.c_int32), _vp, _vp, _vp, _vp, C.c_int32]),
    "bl_lcm_decode_particles": (C.c_int, [_vp, C.c_int64, _P(C.c_int64), _P(C.c_int32), _vp, C.c_int32]),
    "bl_lcm_decode_grid": (C.c_int, [_vp, C.c_int64, _P(C.c_int64), _vp, _vp, _vp, C.c_int64]),
    "bl_lcm_decode_path": (C.c_int, [_vp, C.c_int64, _P(C.c_int64), _P(C.c_int32), _vp, C.c_int32]),
    "bl_lcm_log_event_size": (C.c_int64, [C.c_int32, C.c_int32]),
    "bl_lcm_log_write_event": (C.c_int64, [C.c_int64, C.c_int64, C.c_char_p, _vp, C.c_int32, _vp, C.c_int64]),
    "bl_lcm_log_read_event": (C.c_int64, [_vp, C.c_int64, _P(C.c_int64), _P(C.c_int64), _P(C.c_int64), _P(C.c_int32), _P(C.c_int64),
                                          _P(C.c_int32)]),
    "bl_pf_encode_particles_lcm": (C.c_int64, [_vp, C.c_int64, _vp, C.c_int64]),
    "bl_grid_encode_lcm": (C.c_int64, [_vp, C.c_int64, _vp, C.c_int64]),
    "bl_sim_cast_beams": (C.c_int, [_vp, _vp, C.c_double, C.c_double, C.c_double, _vp, _vp, _vp, C.c_int, C.c_double, _vp]),
    "bl_explorer_create": (C.c_int, [_vp, C.c_int, C.c_double, _P(_vp)]),
    "bl_explorer_destroy": (None, [_vp]),
    "bl_explorer_set_state": (C.c_int, [_vp, _P(Pose), _P(Pose)]),
    "bl_explorer_submit": (C.c_int, [_vp, _vp, _vp]),
    "bl_explorer_pending": (C.c_int, [_vp]),
    "bl_explorer_fetch": (C.c_int, [_vp, _P(ExploreResult), _vp, C.c_int]),
    "bl_explorer_frontiers": (C.c_int, [_vp, _P(_vp)]),
    "bl_plan_path_to_frontier": (C.c_int, [_vp, _vp, _P(Pose), _vp, _P(MotionPlannerState), _vp, C.c_int, _P(C.c_int), _P(Pose),
                                           _vp]),
}

_lib = None


class BotlabHipError(RuntimeError):
    pass


def load():
    """Returns the loaded library with argtypes set; raises if the extension is missing (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise BotlabHipError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). botlab_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError here = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        msg = load().bl_last_error()
        raise BotlabHipError(f"botlab_hip call failed (status {rc}): {msg.decode() if msg else ''}")
