// Compile check of include/botlab/path_shortcut.hpp and the MotionPlannerT methods built on it (g++ -std=c++11 -fsyntax-only), a
// translation unit of its own beside check_headers.cpp.  See tests/cpp/path_shortcut_test.cpp for the run-time check on a GPU.
#include "dropin_test_types.hpp"
#include <botlab/planning_dropin.hpp>
#include <botlab/path_shortcut.hpp>

typedef botlab_hip::PathShortcutT<robot_path_t, pose_xyt_t> CheckPathShortcut;
typedef botlab_hip::MotionPlannerT<pose_xyt_t, robot_path_t> CheckShortcutPlanner;

void touch_path_shortcut(const CheckShortcutPlanner& planner, const robot_path_t& path, const pose_xyt_t& a, const pose_xyt_t& b)
{
    CheckPathShortcut sc;
    sc.setParams(botlab_hip::shortcut_params(0.25, 32, 0));
    int64_t cost[2];
    robot_path_t s = sc.shortcut(path, planner.distances(), cost);
    (void)s.path_length; (void)sc.params(); (void)sc.device();
    std::vector<int32_t> xy(4), offsets(2);
    std::vector<int64_t> costs;
    (void)sc.cells(xy, offsets, planner.distances(), &costs);
    robot_path_t p1 = planner.shortcutPath(path, 0.2, 64, 1024, cost), p2 = planner.shortcutPath(path);
    robot_path_t p3 = planner.planPathShortcut(a, b, 0.2, 16, 0), p4 = planner.planPathShortcut(a, b);
    (void)p1; (void)p2; (void)p3; (void)p4;
}
