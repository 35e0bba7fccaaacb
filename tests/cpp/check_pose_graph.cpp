// Compile check of include/botlab/pose_graph.hpp and OccupancyGridSLAMT::optimizeHistory (g++ -std=c++11 -fsyntax-only), a translation
// unit of its own beside check_headers.cpp.  See tests/cpp/pose_graph_test.cpp for the run-time check.
#include "dropin_test_types.hpp"
#include <botlab/pose_graph.hpp>
#include <botlab/slam_driver.hpp>

#include <cstddef>

typedef botlab_hip::PoseGraphT<pose_xyt_t> CheckGraph;
struct check_odometry_t { int64_t utime; float x, y, theta; };
typedef botlab_hip::OccupancyGridSLAMT<pose_xyt_t, lidar_t, check_odometry_t, particle_t, particles_t, occupancy_grid_t> CheckGraphSLAM;

static_assert(sizeof(bl_posegraph_edge_t) == 80 && offsetof(bl_posegraph_edge_t, z) == 8 && offsetof(bl_posegraph_edge_t, info) == 32, "bl_posegraph_edge_t is 80 bytes");
static_assert(sizeof(bl_posegraph_params_t) == 64 && offsetof(bl_posegraph_params_t, lambda0) == 16 && offsetof(bl_posegraph_params_t, cg_tol) == 56, "bl_posegraph_params_t is 64 bytes");
static_assert(sizeof(bl_posegraph_result_t) == 40 && offsetof(bl_posegraph_result_t, tries) == 24 && offsetof(bl_posegraph_result_t, status) == 36, "bl_posegraph_result_t is 40 bytes");

void touch_pose_graph(const std::vector<pose_xyt_t>& poses, bl_scanlog* log, CheckGraphSLAM& slam)
{
    const double info[6] = {1e4, 0, 1e4, 0, 0, 1e5};
    CheckGraph g(64, 8, 9);
    g.setNodes(poses);
    g.setNodesFromLog(log, 0, 5);
    g.setChainFromNodes(info);
    std::vector<bl_posegraph_edge_t> chain(4, botlab_hip::poseGraphEdge(0, 1, 0.1, 0.0, 0.0, info)), loops(1, botlab_hip::poseGraphEdge(0, 4, 0.0, 0.0, 0.0, info));
    g.setChain(chain);
    g.setLoops(loops);
    g.solve(botlab_hip::poseGraphParams(2));
    g.solve(botlab_hip::poseGraphParams(), 2, std::vector<uint32_t>(2, 1u));
    (void)g.results().size();
    std::vector<double> xyt, before, after;
    (void)g.poses(1, &xyt).size(); (void)g.poses().size();
    g.edgeChi2(0, before, after);
    g.posesToLog(0, log, 0);
    (void)g.lastDeviceMs(); (void)g.nodes(); (void)g.device();
    (void)slam.optimizeHistory(loops, info);
    (void)slam.optimizeHistory(loops, info, botlab_hip::poseGraphParams(1));
    (void)slam.lastPoseGraphResult().cost_after;
}
