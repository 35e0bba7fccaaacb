// local_plan_moving_test.cpp -- LocalPlannerT::commandMoving / commandsMoving (include/botlab/local_planner.hpp),
// ObstacleTrackerT::composeStatic (obstacle_tracks.hpp) and MotionPlannerT::setMapWithStaticObstacles (planning_dropin.hpp) on a map
// file, for tests/test_gpu_local_plan_moving_cpp.py, which compares what this writes with numbers the Python model wrote.
//   local_plan_moving_test <map file> <run file> <out file> <goal cell x> <goal cell y> <reach cells>
// Run file: bl_localplan_params_t, bl_localplan_moving_t, bl_obslayer_params_t, bl_obstracks_params_t, int32 updates, per update the
// layer's state (count uint8 per cell, last uint32 per cell, n uint32), int32 states, then records of (int64 utime, float x, y, theta, v, w).
// Output: the grid of composeStatic, the planner's composed grid, then per record utime, trans_v, angular_v, flags, index, cost.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "dropin_test_types.hpp"
#include <botlab/obstacle_tracks.hpp>
#include <botlab/planning_dropin.hpp>
#include <botlab/local_planner.hpp>

struct mbot_motor_command_t { int64_t utime = 0; float trans_v = 0, angular_v = 0; };
typedef botlab_hip::ObstacleLayerT<pose_xyt_t, lidar_t> Layer;
typedef botlab_hip::ObstacleTrackerT<Layer> Tracker;
typedef botlab_hip::MotionPlannerT<pose_xyt_t, robot_path_t> MotionPlanner;
typedef botlab_hip::LocalPlannerT<pose_xyt_t, robot_path_t, mbot_motor_command_t> LocalPlanner;

static void rd(FILE* f, void* p, size_t n) { if (n && std::fread(p, n, 1, f) != 1) { std::fprintf(stderr, "short run file\n"); std::exit(2); } }

static void put_grid(FILE* out, const botlab_hip::OccupancyGrid& g)
{
    for (int y = 0; y < g.heightInCells(); ++y)
        for (int x = 0; x < g.widthInCells(); ++x) { const int8_t v = g.logOdds(x, y); std::fwrite(&v, 1, 1, out); }
}

int main(int argc, char** argv)
{
    if (argc < 7) return 2;
    botlab_hip::OccupancyGrid map;
    if (!map.loadFromFile(argv[1])) { std::fprintf(stderr, "cannot load %s\n", argv[1]); return 2; }
    FILE* in = std::fopen(argv[2], "rb");
    FILE* out = std::fopen(argv[3], "wb");
    if (!in || !out) return 2;
    bl_localplan_params_t params; bl_localplan_moving_t moving; bl_obslayer_params_t lparams; bl_obstracks_params_t tparams;
    rd(in, &params, sizeof(params)); rd(in, &moving, sizeof(moving)); rd(in, &lparams, sizeof(lparams)); rd(in, &tparams, sizeof(tparams));
    const size_t cells = static_cast<size_t>(map.widthInCells()) * map.heightInCells();
    Layer layer(map.widthInCells(), map.heightInCells(), lparams);
    Tracker tracker(layer, tparams);
    int32_t updates = 0;
    rd(in, &updates, 4);
    std::vector<uint8_t> count(cells);
    std::vector<uint32_t> last(cells);
    for (int u = 0; u < updates; ++u) {
        uint32_t n = 0;
        rd(in, count.data(), cells); rd(in, last.data(), 4 * cells); rd(in, &n, 4);
        layer.upload(count, last, n);
        tracker.update();
    }
    botlab_hip::OccupancyGrid composed;
    tracker.composeStatic(map, composed);
    put_grid(out, composed);
    MotionPlanner planner;
    planner.setMapWithStaticObstacles(map, layer, tracker);
    put_grid(out, planner.composedMap());
    LocalPlanner::NavigationField field;
    std::vector<int32_t> goal(2);
    goal[0] = std::atoi(argv[4]); goal[1] = std::atoi(argv[5]);
    field.compute(planner.distances(), botlab_hip::nav_params(planner.searchParams(), botlab_hip::NAV_OBSTACLE_GAIN, std::atoi(argv[6])), goal);

    LocalPlanner lp;
    lp.setParams(params);
    int32_t n_states = 0;
    rd(in, &n_states, 4);
    std::vector<bl_localplan_state_t> states;
    std::vector<bl_localplan_result_t> single;
    for (int k = 0; k < n_states; ++k) {
        pose_xyt_t pose; float v, w;
        rd(in, &pose.utime, 8); rd(in, &pose.x, 4); rd(in, &pose.y, 4); rd(in, &pose.theta, 4); rd(in, &v, 4); rd(in, &w, 4);
        bl_localplan_result_t r;
        mbot_motor_command_t c = lp.commandMoving(pose, v, w, field, tracker, moving, &r);
        if (c.trans_v != r.trans_v || c.angular_v != r.angular_v || c.utime != pose.utime) return 3;
        std::fwrite(&c.utime, 8, 1, out); std::fwrite(&c.trans_v, 4, 1, out); std::fwrite(&c.angular_v, 4, 1, out);
        std::fwrite(&r.flags, 4, 1, out); std::fwrite(&r.index, 4, 1, out); std::fwrite(&r.cost, 8, 1, out);
        bl_localplan_state_t s;
        s.pose = botlab_hip::pose_in(pose); s.v = v; s.w = w;
        states.push_back(s);
        single.push_back(r);
    }
    const std::vector<bl_localplan_result_t> many = lp.commandsMoving(states, field, tracker, moving);     // the many-state form agrees
    if (many.size() != single.size() || (!many.empty() && std::memcmp(many.data(), single.data(), many.size() * sizeof(many[0])) != 0)) return 3;
    std::fclose(in);
    std::fclose(out);
    std::printf("local_plan_moving_test ok: %d updates, %d commands, moving path %d\n", updates, n_states, bl_localplan_debug_moving_path(lp.device()));
    return 0;
}
