// Compile check of include/botlab/obstacle_layer.hpp and MotionPlannerT::setMapWithObstacles (g++ -std=c++11 -fsyntax-only), a
// translation unit of its own beside check_headers.cpp.  See tests/cpp/obstacle_layer_test.cpp for the run-time check on a GPU.
#include "dropin_test_types.hpp"
#include <botlab/obstacle_layer.hpp>
#include <botlab/planning_dropin.hpp>

typedef botlab_hip::ObstacleLayerT<pose_xyt_t, lidar_t> CheckLayer;
typedef botlab_hip::MotionPlannerT<pose_xyt_t, robot_path_t> CheckPlanner;

static_assert(sizeof(bl_obslayer_params_t) == 20, "bl_obslayer_params_t is 20 bytes");
static_assert(sizeof(bl_obslayer_stats_t) == 40, "bl_obslayer_stats_t is 40 bytes");

void touch_obstacle_layer(const botlab_hip::OccupancyGrid& map, const lidar_t& scan, const pose_xyt_t& pose, CheckPlanner& planner)
{
    CheckLayer layer(map.widthInCells(), map.heightInCells()), layer2(10, 10, botlab_hip::default_obslayer_params());
    bl_obslayer_params_t p = botlab_hip::default_obslayer_params();
    p.max_range = 8.0f; p.occ_min = 10; p.tol_cells = 2; p.ttl_scans = 20; p.min_hits = 2;
    (void)layer.setParams(p);
    layer.update(map, scan, pose);
    botlab_hip::OccupancyGrid out;
    layer.compose(map, out);
    (void)out.logOdds(0, 0);
    (void)layer.classes(); (void)layer.stats().live_cells; (void)layer.liveCells(); (void)layer.lastUpdateMs(); (void)layer.lastComposeMs();
    std::vector<uint8_t> count; std::vector<uint32_t> last; uint32_t n = 0;
    layer.download(count, last, n);
    layer.upload(count, last, n);
    layer.reset();
    (void)layer.device(); (void)layer.widthInCells(); (void)layer.heightInCells();
    planner.setMapWithObstacles(map, layer);
    (void)planner.composedMap().widthInCells();
}
