// Compile check of LocalPlannerT::commandMoving (include/botlab/local_planner.hpp), ObstacleTrackerT::composeStatic and
// MotionPlannerT::setMapWithStaticObstacles (g++ -std=c++11 -fsyntax-only), a translation unit of its own beside check_headers.cpp.
// See tests/cpp/local_plan_moving_test.cpp for the run-time check on a GPU.
#include <cstddef>
#include "dropin_test_types.hpp"
#include <botlab/obstacle_tracks.hpp>
#include <botlab/planning_dropin.hpp>
#include <botlab/local_planner.hpp>

typedef botlab_hip::ObstacleLayerT<pose_xyt_t, lidar_t> CheckLayer;
typedef botlab_hip::ObstacleTrackerT<CheckLayer> CheckTracker;
typedef botlab_hip::MotionPlannerT<pose_xyt_t, robot_path_t> CheckPlanner;
typedef botlab_hip::LocalPlannerT<pose_xyt_t, robot_path_t> CheckLocalPlanner;

static_assert(sizeof(bl_localplan_moving_t) == 16 && offsetof(bl_localplan_moving_t, steps_per_update) == 0 && offsetof(bl_localplan_moving_t, margin_cells) == 4 &&
              offsetof(bl_localplan_moving_t, lead_steps) == 8 && offsetof(bl_localplan_moving_t, reserved) == 12, "bl_localplan_moving_t is 16 bytes");
static_assert(BL_LOCALPLAN_MOVING_BYTES % 8 == 0 && BL_LOCALPLAN_MAX_MARGIN == 64, "the moving rule's constants");

void touch_local_plan_moving(const botlab_hip::OccupancyGrid& map, const pose_xyt_t& pose, CheckPlanner& planner, CheckLocalPlanner& lp,
                             const CheckLocalPlanner::NavigationField& field)
{
    CheckLayer layer(map.widthInCells(), map.heightInCells());
    CheckTracker tracker(layer);
    botlab_hip::OccupancyGrid out;
    tracker.composeStatic(map, out);
    planner.setMapWithStaticObstacles(map, layer, tracker);
    const bl_localplan_moving_t m = botlab_hip::local_plan_moving(2, 1, 0);
    bl_localplan_result_t r;
    (void)lp.commandMoving(pose, 0.1f, 0.0f, field, tracker, m, &r).trans_v;
    (void)lp.commandMoving(pose, 0.1f, 0.0f, field, tracker, botlab_hip::local_plan_moving(2)).angular_v;
    std::vector<bl_localplan_state_t> states(2);
    (void)lp.commandsMoving(states, field, tracker, m).size();
    (void)bl_localplan_debug_moving_path(lp.device());
}
