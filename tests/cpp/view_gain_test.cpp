// view_gain_test.cpp -- ViewGainT and plan_path_to_frontier_by_gain_t (include/botlab/view_gain.hpp) on a map file, for
// tests/test_gpu_view_gain_driver.py, which compares what this writes with the model and with the Python planner.
//   view_gain_test <map file> <out file> <start x> <start y> <start theta> <robot radius> <radius cells> <rays>
// Output records: 'F' the frontiers found from the start pose (count; per frontier its cell count and x, y floats), 'R' the ray table
// (count, x, y int32 pairs), 'G' plan_path_to_frontier_by_gain_t (length, frontier, x, y, gain, cost, poses), 'Z' the same with
// gain_weight 0 and stride 2 (frontier, x, y, gain, cost), 'N' the lengths of the empty-frontier and the no-candidate results and the
// frontier the latter reports, 'E'.
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

static void put_choice(FILE* out, const botlab_hip::FrontierGainChoice& c)
{
    int32_t fi = c.frontier;
    std::fwrite(&fi, 4, 1, out); std::fwrite(&c.x, 4, 1, out); std::fwrite(&c.y, 4, 1, out); std::fwrite(&c.gain, 4, 1, out); std::fwrite(&c.cost, 4, 1, out);
}

int main(int argc, char** argv)
{
    if (argc < 9) return 2;
    botlab_hip::OccupancyGrid map;
    if (!map.loadFromFile(argv[1])) { std::fprintf(stderr, "cannot load %s\n", argv[1]); return 2; }
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 2;
    pose_xyt_t start;
    start.utime = 4242; start.x = static_cast<float>(std::atof(argv[3])); start.y = static_cast<float>(std::atof(argv[4])); start.theta = static_cast<float>(std::atof(argv[5]));
    botlab_hip::MotionPlannerParams mp;
    mp.robotRadius = std::atof(argv[6]);
    MotionPlanner planner(mp);
    planner.setMap(map);

    std::vector<botlab_hip::frontier_t> fr = botlab_hip::find_map_frontiers_t(map, start);
    planner.setNumFrontiers(fr.size());
    int32_t nf = static_cast<int32_t>(fr.size());
    std::fwrite("F", 1, 1, out); std::fwrite(&nf, 4, 1, out);
    for (const botlab_hip::frontier_t& f : fr) {
        int32_t n = static_cast<int32_t>(f.cells.size());
        std::fwrite(&n, 4, 1, out);
        for (const botlab_hip::PointT<float>& c : f.cells) { std::fwrite(&c.x, 4, 1, out); std::fwrite(&c.y, 4, 1, out); }
    }

    botlab_hip::ViewGainT view(botlab_hip::view_gain_params(std::atoi(argv[7]), std::atoi(argv[8])));
    std::vector<int32_t> ends = view.rayEnds();
    int32_t nr = static_cast<int32_t>(ends.size() / 2);
    std::fwrite("R", 1, 1, out); std::fwrite(&nr, 4, 1, out); std::fwrite(ends.data(), 4, ends.size(), out);
    if (view.debugSeen(map, 0, 0).size() != static_cast<size_t>(2 * view.radiusInCells() + 1) * (2 * view.radiusInCells() + 1)) return 3;

    botlab_hip::FrontierGainChoice c;
    robot_path_t g = botlab_hip::plan_path_to_frontier_by_gain_t<robot_path_t>(fr, start, map, planner, view, botlab_hip::FrontierGainOptions(), &c);
    if (g.path_length != static_cast<int32_t>(g.path.size())) return 3;
    int32_t len = g.path_length;
    std::fwrite("G", 1, 1, out); std::fwrite(&len, 4, 1, out); put_choice(out, c); put_path(out, g);

    botlab_hip::FrontierGainOptions zero;
    zero.gain_weight = 0; zero.stride = 2;
    botlab_hip::FrontierGainChoice cz;
    (void)botlab_hip::plan_path_to_frontier_by_gain_t<robot_path_t>(fr, start, map, planner, view, zero, &cz);
    std::fwrite("Z", 1, 1, out); put_choice(out, cz);

    botlab_hip::FrontierGainChoice ce, cn;
    robot_path_t e = botlab_hip::plan_path_to_frontier_by_gain_t<robot_path_t>(std::vector<botlab_hip::frontier_t>(), start, map, planner, view, botlab_hip::FrontierGainOptions(), &ce);
    botlab_hip::FrontierGainOptions never;
    never.min_gain = 0xFFFFFFFFu;
    robot_path_t n = botlab_hip::plan_path_to_frontier_by_gain_t<robot_path_t>(fr, start, map, planner, view, never, &cn);
    int32_t le = static_cast<int32_t>(e.path.size()), ln = static_cast<int32_t>(n.path.size()), fe = ce.frontier, fn = cn.frontier;
    std::fwrite("N", 1, 1, out); std::fwrite(&le, 4, 1, out); std::fwrite(&fe, 4, 1, out); std::fwrite(&ln, 4, 1, out); std::fwrite(&fn, 4, 1, out);
    std::fwrite("E", 1, 1, out);
    std::fclose(out);
    std::printf("view_gain_test ok: %d frontiers, %d poses to cell (%d, %d) of frontier %d, gain %u, cost %u\n", nf, len, c.x, c.y, c.frontier, c.gain, c.cost);
    return 0;
}
