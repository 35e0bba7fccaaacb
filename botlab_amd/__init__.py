"""botlab_amd -- MI355X (gfx950) implementation of botLab's occupancy-grid SLAM / MCL / A* hot path.

The product is libbotlab_hip.so (hand-written HIP kernels behind the C ABI in include/botlab_hip.h).  This package is
the Python host mirror of the reference's class surfaces used by tests and bench.py.  There is no CPU fallback: every
call raises if the HIP library is missing or no GPU is visible.
"""
from ._capi import BotlabHipError, Lidar, Particle, Pose, SearchParams, load  # noqa: F401
from .host import (AsyncExplorer, AsyncPlanner, Context, LidarScan, Mapping, MotionPlanner, MotionPlannerParams, ObstacleDistanceGrid,  # noqa: F401
                   OccupancyGrid, ParticleFilter, PARTICLE_DTYPE, POSE_DTYPE, default_context, make_pose,
                   search_for_path, search_for_path_begin, search_for_path_end, search_for_path_batch, Frontiers,
                   find_map_frontiers, plan_path_to_frontier, ExploringMap, ScanMatcher, NavigationField, nav_params,
                   plan_path_to_frontier_by_cost, NAV_UNREACHED, ViewGain, plan_path_to_frontier_by_gain, RBSlam, LocalPlanner, LOCALPLAN_RESULT_DTYPE, MppiPlanner, MPPI_RESULT_DTYPE, MPPI_FELL_BACK,
                   LOCALPLAN_REACHED, LOCALPLAN_OFF_FIELD, LOCALPLAN_BLOCKED, PathShortcut, LikelihoodField, ObstacleLayer, ObstacleTracker, track_to_metric, BeamModel, BEAM_OFF_GRID, RangeTable, ClearanceGrid,
                   prior_from_sigmas, ScanHistory, PoseGraph, posegraph_params, posegraph_edges, find_loop_closures, close_loops, POSEGRAPH_EDGE_DTYPE,
                   LoopCloser, LOOPCLOSE_CANDIDATE_DTYPE, LOOPCLOSE_PLACE_DTYPE, LC_NOT_ACCEPTED, LC_TIED, LC_ON_EDGE, LC_TOO_MANY_RAYS,
                   POSEGRAPH_RESULT_DTYPE, POSEGRAPH_CONVERGED_STEP, POSEGRAPH_CONVERGED_DECREASE, POSEGRAPH_OUT_OF_TRIES, POSEGRAPH_CG_CAP)

__all__ = ["AsyncExplorer", "AsyncPlanner", "BotlabHipError", "Lidar", "Particle", "Pose", "SearchParams", "load", "Context", "LidarScan", "Mapping",
           "MotionPlanner", "MotionPlannerParams", "ObstacleDistanceGrid", "OccupancyGrid", "ParticleFilter",
           "PARTICLE_DTYPE", "POSE_DTYPE", "default_context", "make_pose", "search_for_path", "search_for_path_begin",
           "search_for_path_end", "search_for_path_batch", "Frontiers", "find_map_frontiers", "plan_path_to_frontier", "ExploringMap", "ScanMatcher",
           "NavigationField", "nav_params", "plan_path_to_frontier_by_cost", "NAV_UNREACHED", "ViewGain",
           "plan_path_to_frontier_by_gain", "RBSlam", "LocalPlanner", "LOCALPLAN_RESULT_DTYPE", "MppiPlanner", "MPPI_RESULT_DTYPE", "MPPI_FELL_BACK", "LOCALPLAN_REACHED", "LOCALPLAN_OFF_FIELD",
           "LOCALPLAN_BLOCKED", "PathShortcut", "LikelihoodField", "ObstacleLayer", "ObstacleTracker", "track_to_metric", "prior_from_sigmas", "BeamModel", "BEAM_OFF_GRID", "RangeTable", "ClearanceGrid", "ScanHistory", "PoseGraph", "posegraph_params", "find_loop_closures", "close_loops",
           "posegraph_edges", "POSEGRAPH_EDGE_DTYPE", "POSEGRAPH_RESULT_DTYPE", "POSEGRAPH_CONVERGED_STEP", "POSEGRAPH_CONVERGED_DECREASE",
           "POSEGRAPH_OUT_OF_TRIES", "POSEGRAPH_CG_CAP", "LoopCloser", "LOOPCLOSE_CANDIDATE_DTYPE", "LOOPCLOSE_PLACE_DTYPE", "LC_NOT_ACCEPTED", "LC_TIED", "LC_ON_EDGE",
           "LC_TOO_MANY_RAYS"]
