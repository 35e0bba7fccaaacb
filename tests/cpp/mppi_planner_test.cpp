// mppi_planner_test.cpp -- MppiPlannerT (include/botlab/mppi_planner.hpp) on a map file, for tests/test_gpu_mppi_cpp.py, which
// compares what this writes with the model.
//   mppi_planner_test <map file> <run file> <out file> <goal cell x> <goal cell y> <reach cells>
// Run file: bl_mppi_params_t, then records of (int64 utime, float x, y, theta, v, w) to the end of the file: consecutive ticks of one
// robot.  Each record is one command() -- the last one commandMoving() against a tracker without tracks -- followed by advance().
// Output, per record: utime, trans_v, angular_v, flags, index_best, cost_out; then the sequence held after the last command.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "dropin_test_types.hpp"
#include <botlab/obstacle_tracks.hpp>
#include <botlab/planning_dropin.hpp>
#include <botlab/mppi_planner.hpp>

struct mbot_motor_command_t { int64_t utime = 0; float trans_v = 0, angular_v = 0; };
typedef botlab_hip::ObstacleLayerT<pose_xyt_t, lidar_t> Layer;
typedef botlab_hip::ObstacleTrackerT<Layer> Tracker;
typedef botlab_hip::MotionPlannerT<pose_xyt_t, robot_path_t> MotionPlanner;
typedef botlab_hip::MppiPlannerT<pose_xyt_t, robot_path_t, mbot_motor_command_t> MppiPlanner;

int main(int argc, char** argv)
{
    if (argc < 7) return 2;
    botlab_hip::OccupancyGrid map;
    if (!map.loadFromFile(argv[1])) { std::fprintf(stderr, "cannot load %s\n", argv[1]); return 2; }
    FILE* in = std::fopen(argv[2], "rb");
    FILE* out = std::fopen(argv[3], "wb");
    if (!in || !out) return 2;
    bl_mppi_params_t params;
    if (std::fread(&params, sizeof(params), 1, in) != 1) return 2;
    std::vector<pose_xyt_t> poses;
    std::vector<float> vs, ws;
    for (;;) {
        pose_xyt_t pose; float v, w;
        if (std::fread(&pose.utime, 8, 1, in) != 1) break;
        if (std::fread(&pose.x, 4, 1, in) != 1 || std::fread(&pose.y, 4, 1, in) != 1 || std::fread(&pose.theta, 4, 1, in) != 1) return 3;
        if (std::fread(&v, 4, 1, in) != 1 || std::fread(&w, 4, 1, in) != 1) return 3;
        poses.push_back(pose); vs.push_back(v); ws.push_back(w);
    }

    MotionPlanner planner;                                         // robotRadius 0.2: the search parameters the field is built from
    planner.setMap(map);
    MppiPlanner::NavigationField field;
    std::vector<int32_t> goal(2);
    goal[0] = std::atoi(argv[4]); goal[1] = std::atoi(argv[5]);
    field.compute(planner.distances(), botlab_hip::nav_params(planner.searchParams(), botlab_hip::NAV_OBSTACLE_GAIN, std::atoi(argv[6])), goal);
    Layer layer(map.widthInCells(), map.heightInCells());
    Tracker tracker(layer);                                        // no update yet: no tracks

    MppiPlanner mp;                                                // the defaults first, then the run's own
    mp.setParams(params);
    for (size_t k = 0; k < poses.size(); ++k) {
        if (k) mp.advance();
        bl_mppi_result_t r;
        mbot_motor_command_t c = k + 1 < poses.size() ? mp.command(poses[k], vs[k], ws[k], field, &r)
                                                      : mp.commandMoving(poses[k], vs[k], ws[k], field, tracker, botlab_hip::local_plan_moving(2, 1, 0), &r);
        if (c.trans_v != r.trans_v || c.angular_v != r.angular_v || c.utime != poses[k].utime || mp.tick() != k) return 3;
        std::fwrite(&c.utime, 8, 1, out); std::fwrite(&c.trans_v, 4, 1, out); std::fwrite(&c.angular_v, 4, 1, out);
        std::fwrite(&r.flags, 4, 1, out); std::fwrite(&r.index_best, 4, 1, out); std::fwrite(&r.cost_out, 8, 1, out);
    }
    const std::vector<int32_t>& seq = mp.sequence();
    std::fwrite(seq.data(), 4, seq.size(), out);
    const size_t drawn = mp.rollout(poses.back(), vs.back(), ws.back(), field).size();
    std::fclose(in);
    std::fclose(out);
    std::printf("mppi_planner_test ok: %d commands, %d controls, %d rollout poses\n", static_cast<int>(poses.size()), static_cast<int>(seq.size() / 2),
                static_cast<int>(drawn));
    return 0;
}
