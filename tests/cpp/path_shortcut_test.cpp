// path_shortcut_test.cpp -- PathShortcutT (include/botlab/path_shortcut.hpp) and MotionPlannerT::shortcutPath / planPathShortcut
// (planning_dropin.hpp) on a map file, for tests/test_gpu_path_shortcut_cpp.py and tests/test_gpu_path_shortcut_driver.py, which
// compare what this writes with the model.
//   path_shortcut_test <map file> <path file> <out file> <clearance> <max span> <waypoint cost>
//                      [<start utime> <start x> <start y> <start theta> <goal x> <goal y>]
// Path file: records of (int64 utime, float x, y, theta) to the end of the file.
// Output records: 'S' PathShortcutT::shortcut (length, the two costs, poses), 'M' MotionPlannerT::shortcutPath (length, poses), 'C'
// PathShortcutT::cells on the path's cells (count, kept indices); with a start and a goal 'D' planPathShortcut (length, poses); 'E'.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "dropin_test_types.hpp"
#include <botlab/planning_dropin.hpp>
#include <botlab/path_shortcut.hpp>

typedef botlab_hip::MotionPlannerT<pose_xyt_t, robot_path_t> MotionPlanner;
typedef botlab_hip::PathShortcutT<robot_path_t, pose_xyt_t> PathShortcut;

static void put_path(FILE* out, const robot_path_t& p)
{
    int32_t n = static_cast<int32_t>(p.path.size());
    std::fwrite(&n, 4, 1, out);
    for (const pose_xyt_t& q : p.path) { std::fwrite(&q.utime, 8, 1, out); std::fwrite(&q.x, 4, 1, out); std::fwrite(&q.y, 4, 1, out); std::fwrite(&q.theta, 4, 1, out); }
}

int main(int argc, char** argv)
{
    if (argc < 7) return 2;
    botlab_hip::OccupancyGrid map;
    if (!map.loadFromFile(argv[1])) { std::fprintf(stderr, "cannot load %s\n", argv[1]); return 2; }
    FILE* in = std::fopen(argv[2], "rb");
    FILE* out = std::fopen(argv[3], "wb");
    if (!in || !out) return 2;
    const double clearance = std::atof(argv[4]);
    const int max_span = std::atoi(argv[5]), waypoint_cost = std::atoi(argv[6]);
    robot_path_t path;
    path.utime = 31;
    for (;;) {
        pose_xyt_t q;
        if (std::fread(&q.utime, 8, 1, in) != 1) break;
        if (std::fread(&q.x, 4, 1, in) != 1 || std::fread(&q.y, 4, 1, in) != 1 || std::fread(&q.theta, 4, 1, in) != 1) return 3;
        path.path.push_back(q);
    }
    path.path_length = static_cast<int32_t>(path.path.size());
    std::fclose(in);

    MotionPlanner planner;                                         // robotRadius 0.2
    planner.setMap(map);
    PathShortcut sc;                                               // the defaults first, then the run's own
    sc.setParams(botlab_hip::shortcut_params(clearance, max_span, waypoint_cost));
    int64_t cost[2] = {-1, -1};
    robot_path_t s = sc.shortcut(path, planner.distances(), cost);
    if (s.path_length != static_cast<int32_t>(s.path.size()) || s.utime != path.utime) return 3;
    std::fwrite("S", 1, 1, out); put_path(out, s); std::fwrite(cost, 8, 2, out);
    robot_path_t m = planner.shortcutPath(path, clearance, max_span, waypoint_cost);
    std::fwrite("M", 1, 1, out); put_path(out, m);

    const botlab_hip::PointT<float> o = planner.distances().originInGlobalFrame();
    std::vector<int32_t> xy, offsets(2, 0);
    for (const pose_xyt_t& q : path.path) {
        xy.push_back(static_cast<int>((static_cast<double>(q.x) - o.x) * planner.distances().cellsPerMeter()));
        xy.push_back(static_cast<int>((static_cast<double>(q.y) - o.y) * planner.distances().cellsPerMeter()));
    }
    offsets[1] = static_cast<int32_t>(path.path.size());
    std::vector<int64_t> costs;
    std::vector<std::vector<int32_t> > keep = sc.cells(xy, offsets, planner.distances(), &costs);
    if (keep.size() != 1 || costs.size() != 2 || costs[0] != cost[0] || costs[1] != cost[1]) return 3;
    int32_t nk = static_cast<int32_t>(keep[0].size());
    std::fwrite("C", 1, 1, out); std::fwrite(&nk, 4, 1, out); std::fwrite(keep[0].data(), 4, keep[0].size(), out);

    int nd = -1;
    if (argc >= 13) {
        pose_xyt_t start, goal;
        start.utime = std::atoll(argv[7]);
        start.x = static_cast<float>(std::atof(argv[8])); start.y = static_cast<float>(std::atof(argv[9])); start.theta = static_cast<float>(std::atof(argv[10]));
        goal.utime = 0; goal.x = static_cast<float>(std::atof(argv[11])); goal.y = static_cast<float>(std::atof(argv[12])); goal.theta = 0;
        robot_path_t d = planner.planPathShortcut(start, goal, clearance, max_span, waypoint_cost);
        nd = static_cast<int>(d.path.size());
        std::fwrite("D", 1, 1, out); put_path(out, d);
    }
    std::fwrite("E", 1, 1, out);
    std::fclose(out);
    std::printf("path_shortcut_test ok: %d poses -> %d, planned %d\n", path.path_length, s.path_length, nd);
    return 0;
}
