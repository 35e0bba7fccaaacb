// local_planner_test.cpp -- LocalPlannerT (include/botlab/local_planner.hpp) on a map file, for tests/test_gpu_local_plan_cpp.py,
// which compares what this writes with the model.
//   local_planner_test <map file> <run file> <out file> <goal cell x> <goal cell y> <reach cells>
// Run file: bl_localplan_params_t, then records of (int64 utime, float x, y, theta, v, w) to the end of the file.
// Output, per record: utime, trans_v, angular_v, flags, index, cost; then the x, y, theta of the first record's winning rollout.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "dropin_test_types.hpp"
#include <botlab/planning_dropin.hpp>
#include <botlab/local_planner.hpp>

struct mbot_motor_command_t { int64_t utime = 0; float trans_v = 0, angular_v = 0; };
typedef botlab_hip::MotionPlannerT<pose_xyt_t, robot_path_t> MotionPlanner;
typedef botlab_hip::LocalPlannerT<pose_xyt_t, robot_path_t, mbot_motor_command_t> LocalPlanner;

int main(int argc, char** argv)
{
    if (argc < 7) return 2;
    botlab_hip::OccupancyGrid map;
    if (!map.loadFromFile(argv[1])) { std::fprintf(stderr, "cannot load %s\n", argv[1]); return 2; }
    FILE* in = std::fopen(argv[2], "rb");
    FILE* out = std::fopen(argv[3], "wb");
    if (!in || !out) return 2;
    bl_localplan_params_t params;
    if (std::fread(&params, sizeof(params), 1, in) != 1) return 2;

    MotionPlanner planner;                                         // robotRadius 0.2: the search parameters the field is built from
    planner.setMap(map);
    LocalPlanner::NavigationField field;
    std::vector<int32_t> goal(2);
    goal[0] = std::atoi(argv[4]); goal[1] = std::atoi(argv[5]);
    field.compute(planner.distances(), botlab_hip::nav_params(planner.searchParams(), botlab_hip::NAV_OBSTACLE_GAIN, std::atoi(argv[6])), goal);

    LocalPlanner lp;                                               // the defaults first, then the run's own
    lp.setParams(params);
    int n = 0;
    std::vector<pose_xyt_t> first_rollout;
    for (;;) {
        pose_xyt_t pose; float v, w;
        if (std::fread(&pose.utime, 8, 1, in) != 1) break;
        if (std::fread(&pose.x, 4, 1, in) != 1 || std::fread(&pose.y, 4, 1, in) != 1 || std::fread(&pose.theta, 4, 1, in) != 1) return 3;
        if (std::fread(&v, 4, 1, in) != 1 || std::fread(&w, 4, 1, in) != 1) return 3;
        bl_localplan_result_t r;
        mbot_motor_command_t c = lp.command(pose, v, w, field, &r);
        if (c.trans_v != r.trans_v || c.angular_v != r.angular_v) return 3;
        std::fwrite(&c.utime, 8, 1, out); std::fwrite(&c.trans_v, 4, 1, out); std::fwrite(&c.angular_v, 4, 1, out);
        std::fwrite(&r.flags, 4, 1, out); std::fwrite(&r.index, 4, 1, out); std::fwrite(&r.cost, 8, 1, out);
        if (n == 0 && r.index >= 0) first_rollout = lp.rollout(pose, v, w, field, r.index);
        ++n;
    }
    for (const pose_xyt_t& q : first_rollout) { std::fwrite(&q.x, 4, 1, out); std::fwrite(&q.y, 4, 1, out); std::fwrite(&q.theta, 4, 1, out); }
    std::fclose(in);
    std::fclose(out);
    std::printf("local_planner_test ok: %d commands, %d rollout poses\n", n, static_cast<int>(first_rollout.size()));
    return 0;
}
