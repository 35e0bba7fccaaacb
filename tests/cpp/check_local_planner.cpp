// Compile check of include/botlab/local_planner.hpp (g++ -std=c++11 -fsyntax-only), a translation unit of its own beside
// check_headers.cpp: instantiates LocalPlannerT with plain message structs.  See tests/cpp/local_planner_test.cpp for the run-time
// check on a GPU.
#include "dropin_test_types.hpp"
#include <botlab/local_planner.hpp>

struct mbot_motor_command_t { int64_t utime = 0; float trans_v = 0, angular_v = 0; };
typedef botlab_hip::LocalPlannerT<pose_xyt_t, robot_path_t, mbot_motor_command_t> CheckLocalPlanner;
typedef botlab_hip::LocalPlannerT<pose_xyt_t, robot_path_t> CheckLocalPlannerDefaultCommand;

void touch_local_planner(const botlab_hip::ObstacleDistanceGrid& d, const pose_xyt_t& pose)
{
    CheckLocalPlanner::NavigationField field;
    field.computeToPose(d, botlab_hip::nav_params(botlab_hip::SearchParams()), pose);
    CheckLocalPlanner lp;
    lp.setParams(botlab_hip::local_plan_params(0.4f));
    bl_localplan_result_t r;
    mbot_motor_command_t c = lp.command(pose, 0.1f, 0.0f, field, &r);
    (void)c.utime; (void)lp.params(); (void)lp.device();
    std::vector<pose_xyt_t> arc = lp.rollout(pose, 0.1f, 0.0f, field, 0);
    std::vector<bl_localplan_state_t> states(2);
    (void)lp.commands(states, field); (void)arc;
    CheckLocalPlannerDefaultCommand lp2;
    botlab_hip::motor_command_t c2 = lp2.command(pose, 0.0f, 0.0f, field);
    (void)c2;
}
