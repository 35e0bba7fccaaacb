// nav_field_test.cpp -- MotionPlannerT::planPathOptimal and plan_path_to_frontier_by_cost_t (include/botlab/planning_dropin.hpp,
// nav_field.hpp) on a map file, for tests/test_gpu_nav_field_driver.py, which compares what this writes with the model.
//   nav_field_test <map file> <out file> <start x> <start y> <start theta> <goal x> <goal y> [robot radius]
// Output records: 'P' planPathOptimal (length, cost, poses), 'F' the frontiers found from the start pose (count; per frontier its
// cell count and x, y floats), 'C' plan_path_to_frontier_by_cost_t (length, frontier index, cost, reach used, poses), 'T' the
// field's stats of a compute of its own (5 x int64), 'E'.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "dropin_test_types.hpp"
#include <botlab/planning_dropin.hpp>

typedef botlab_hip::MotionPlannerT<pose_xyt_t, robot_path_t> MotionPlanner;

static void put_path(FILE* out, const robot_path_t& p)
{
    for (const pose_xyt_t& q : p.path) { std::fwrite(&q.utime, 8, 1, out); std::fwrite(&q.x, 4, 1, out); std::fwrite(&q.y, 4, 1, out); std::fwrite(&q.theta, 4, 1, out); }
}

int main(int argc, char** argv)
{
    if (argc < 8) return 2;
    botlab_hip::OccupancyGrid map;
    if (!map.loadFromFile(argv[1])) { std::fprintf(stderr, "cannot load %s\n", argv[1]); return 2; }
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 2;
    pose_xyt_t start, goal;
    start.utime = 4242; start.x = static_cast<float>(std::atof(argv[3])); start.y = static_cast<float>(std::atof(argv[4])); start.theta = static_cast<float>(std::atof(argv[5]));
    goal.x = static_cast<float>(std::atof(argv[6])); goal.y = static_cast<float>(std::atof(argv[7]));

    botlab_hip::MotionPlannerParams mp;
    if (argc > 8) mp.robotRadius = std::atof(argv[8]);
    MotionPlanner planner(mp);
    planner.setMap(map);
    uint32_t cost = 0;
    robot_path_t p = planner.planPathOptimal(start, goal, botlab_hip::NAV_OBSTACLE_GAIN, &cost);
    if (p.path_length != static_cast<int32_t>(p.path.size())) return 3;
    std::fwrite("P", 1, 1, out); std::fwrite(&p.path_length, 4, 1, out); std::fwrite(&cost, 4, 1, out); put_path(out, p);

    std::vector<botlab_hip::frontier_t> fr = botlab_hip::find_map_frontiers_t(map, start);
    planner.setNumFrontiers(fr.size());
    int32_t nf = static_cast<int32_t>(fr.size());
    std::fwrite("F", 1, 1, out); std::fwrite(&nf, 4, 1, out);
    for (const botlab_hip::frontier_t& f : fr) {
        int32_t n = static_cast<int32_t>(f.cells.size());
        std::fwrite(&n, 4, 1, out);
        for (const botlab_hip::PointT<float>& c : f.cells) { std::fwrite(&c.x, 4, 1, out); std::fwrite(&c.y, 4, 1, out); }
    }
    int frontier = -2;
    robot_path_t c = botlab_hip::plan_path_to_frontier_by_cost_t<robot_path_t>(fr, start, map, planner, -1, &frontier, &cost);
    int32_t len = static_cast<int32_t>(c.path.size()), fi = frontier, reach = botlab_hip::nav_min_traversable_cells(planner.distances(), planner.searchParams());
    std::fwrite("C", 1, 1, out); std::fwrite(&len, 4, 1, out); std::fwrite(&fi, 4, 1, out); std::fwrite(&cost, 4, 1, out); std::fwrite(&reach, 4, 1, out);
    put_path(out, c);

    botlab_hip::NavigationFieldT<pose_xyt_t, robot_path_t> field;
    field.computeToPose(planner.distances(), botlab_hip::nav_params(planner.searchParams()), goal);
    std::vector<int64_t> st = field.stats();
    std::fwrite("T", 1, 1, out); std::fwrite(st.data(), 8, 5, out);
    if (field.cells().size() != static_cast<size_t>(field.widthInCells()) * field.heightInCells()) return 3;
    // an empty frontier list gives the empty path
    robot_path_t e = botlab_hip::plan_path_to_frontier_by_cost_t<robot_path_t>(std::vector<botlab_hip::frontier_t>(), start, map, planner);
    if (!e.path.empty()) return 3;
    std::fwrite("E", 1, 1, out);
    std::fclose(out);
    std::printf("nav_field_test ok: %d poses to the goal, %d frontiers, %d poses to frontier %d\n", p.path_length, nf, len, fi);
    return 0;
}
