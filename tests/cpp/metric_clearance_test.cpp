// metric_clearance_test.cpp -- ObstacleDistanceGrid::euclidean (include/botlab/botlab_dropin.hpp) and MotionPlannerT::setMetricClearance
// (planning_dropin.hpp) on the diagonal-gap maps, for tests/test_gpu_metric_clearance_cpp.py.
//   metric_clearance_test <gap map, offset 5> <gap map, offset 7> <fixture> <start x> <start y> <goal x> <goal y>
// The fixture (tests/golden/metric_clearance_gap.txt, written by the Python models) holds "<name> <unsigned integer>" lines: the hashes
// of the codes of either metric, and cost and length of the field's path from the start on either grid of either map.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>
#include "dropin_test_types.hpp"
#include <botlab/planning_dropin.hpp>

typedef botlab_hip::MotionPlannerT<pose_xyt_t, robot_path_t> MotionPlanner;
using botlab_hip::ObstacleDistanceGrid;

static int fails = 0;
#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); ++fails; } } while (0)

static uint64_t fnv1a64(const std::vector<uint16_t>& v)
{
    uint64_t h = 0xCBF29CE484222325ull;
    for (size_t i = 0; i < v.size(); ++i)
        for (int b = 0; b < 2; ++b) { h ^= (v[i] >> (8 * b)) & 0xFFu; h *= 0x100000001B3ull; }
    return h;
}

static bool same_path(const robot_path_t& a, const robot_path_t& b)
{
    if (a.path.size() != b.path.size()) return false;
    for (size_t i = 0; i < a.path.size(); ++i)
        if (std::memcmp(&a.path[i].x, &b.path[i].x, 4) || std::memcmp(&a.path[i].y, &b.path[i].y, 4) || std::memcmp(&a.path[i].theta, &b.path[i].theta, 4))
            return false;
    return true;
}

int main(int argc, char** argv)
{
    if (argc < 8) return 2;
    botlab_hip::OccupancyGrid gap5, gap7;
    if (!gap5.loadFromFile(argv[1]) || !gap7.loadFromFile(argv[2])) { std::fprintf(stderr, "cannot load the maps\n"); return 2; }
    std::map<std::string, uint64_t> want;
    {
        FILE* in = std::fopen(argv[3], "r");
        if (!in) return 2;
        char name[64];
        unsigned long long v;
        while (std::fscanf(in, "%63s %llu", name, &v) == 2) want[name] = v;
        std::fclose(in);
    }
    if (want.size() < 14) return 2;
    const int R = static_cast<int>(want["max_cells"]);
    pose_xyt_t start, goal;
    start.utime = 5; start.x = static_cast<float>(std::atof(argv[4])); start.y = static_cast<float>(std::atof(argv[5]));
    goal.x = static_cast<float>(std::atof(argv[6])); goal.y = static_cast<float>(std::atof(argv[7]));

    // ---- the factory, the codes, the table
    ObstacleDistanceGrid l1;
    ObstacleDistanceGrid eu = ObstacleDistanceGrid::euclidean(R);
    EXPECT(l1.metric() == BL_DIST_L1 && l1.maxCells() == 0 && eu.metric() == BL_DIST_EUCLIDEAN && eu.maxCells() == R);
    l1.setDistances(gap5);
    eu.setDistances(gap5);
    EXPECT(fnv1a64(l1.codes()) == want["l1_codes_fnv_5"] && fnv1a64(eu.codes()) == want["codes_fnv_5"]);
    EXPECT(eu.table().size() == want["table_n"] && l1.table().size() == 81u);
    EXPECT(eu.table()[16] == static_cast<float>(4.0 * static_cast<double>(eu.metersPerCell())));
    // the wall cell (0, 18) is a source; its neighbour above is one cell away in either metric
    EXPECT(eu(0, 18) == 0.0f && eu(0, 19) == eu.table()[1] && l1(0, 19) == 0.1f);

    // ---- value semantics: a copy is a grid of the same metric with the same codes; assignment takes the metric over
    ObstacleDistanceGrid copy(eu);
    EXPECT(copy.metric() == BL_DIST_EUCLIDEAN && copy.maxCells() == R && copy.codes() == eu.codes());
    eu.setDistances(gap7);
    EXPECT(fnv1a64(eu.codes()) == want["codes_fnv_7"] && fnv1a64(copy.codes()) == want["codes_fnv_5"]);      // the copy is its own grid
    ObstacleDistanceGrid other;
    other = eu;
    EXPECT(other.metric() == BL_DIST_EUCLIDEAN && fnv1a64(other.codes()) == want["codes_fnv_7"]);
    other = l1;
    EXPECT(other.metric() == BL_DIST_L1 && other.maxCells() == 0 && fnv1a64(other.codes()) == want["l1_codes_fnv_5"]);

    // ---- the search refuses a Euclidean grid (through the C ABI: the classes' check() ends the program on an error)
    {
        bl_search_params_t sp = {0.2, 1.0, 1.0};
        bl_pose_xyt_t s = botlab_hip::pose_in(start), g = botlab_hip::pose_in(goal), buf[8];
        int len = 0;
        EXPECT(bl_astar_search(botlab_hip::default_ctx(), copy.device(), &s, &g, &sp, buf, 8, &len, nullptr) == BL_ERR_ARG);
        EXPECT(std::strstr(bl_last_error(), "L1") != nullptr);
        EXPECT(fnv1a64(copy.codes()) == want["codes_fnv_5"]);
    }

    // ---- MotionPlannerT::setMetricClearance on the gap the L1 grid calls open
    botlab_hip::MotionPlannerParams mp;                              // robotRadius 0.2
    botlab_hip::SearchParams sp = {0.2, 1.0, 1.0};
    MotionPlanner plain(mp, sp), planner(mp, sp);
    plain.setMap(gap5);
    planner.setMap(gap5);
    EXPECT(!planner.metricClearance());
    uint32_t cost = 0;
    const robot_path_t astar = plain.planPath(start, goal);
    const robot_path_t l1_opt = plain.planPathOptimal(start, goal, botlab_hip::NAV_OBSTACLE_GAIN, &cost);
    EXPECT(cost == want["l1_cost_5"] && l1_opt.path.size() == want["l1_len_5"] && astar.path.size() > 1);
    planner.setMetricClearance(R);                                   // after setMap: the map already set is transformed
    EXPECT(planner.metricClearance() && planner.metricDistances().metric() == BL_DIST_EUCLIDEAN);
    EXPECT(fnv1a64(planner.metricDistances().codes()) == want["codes_fnv_5"]);
    robot_path_t p = planner.planPathOptimal(start, goal, botlab_hip::NAV_OBSTACLE_GAIN, &cost);
    EXPECT(cost == want["euclid_cost_5"] && p.path.size() == want["euclid_len_5"]);                       // closed in metres
    EXPECT(same_path(planner.planPath(start, goal), astar));                                             // the search stays on the L1 grid
    EXPECT(planner.isValidGoal(goal) && planner.isPathSafe(astar) == plain.isPathSafe(astar));
    EXPECT(planner.planPathShortcut(start, goal).path.size() == 1);
    planner.setMap(gap7);                                            // setMap transforms both grids
    plain.setMap(gap7);
    EXPECT(fnv1a64(planner.metricDistances().codes()) == want["codes_fnv_7"]);
    p = planner.planPathOptimal(start, goal, botlab_hip::NAV_OBSTACLE_GAIN, &cost);
    EXPECT(cost == want["euclid_cost_7"] && p.path.size() == want["euclid_len_7"]);
    const robot_path_t l1_opt7 = plain.planPathOptimal(start, goal, botlab_hip::NAV_OBSTACLE_GAIN, &cost);
    EXPECT(cost == want["l1_cost_7"] && l1_opt7.path.size() == want["l1_len_7"]);
    const robot_path_t s = planner.shortcutPath(p);
    EXPECT(s.path.size() >= 2 && s.path.size() < p.path.size());
    MotionPlanner copied(planner);                                   // a copied planner keeps the switch and its own grids
    EXPECT(copied.metricClearance() && same_path(copied.planPathOptimal(start, goal), p));
    planner.setMetricClearance(0);                                   // off again: as if it had never been on
    EXPECT(!planner.metricClearance() && same_path(planner.planPathOptimal(start, goal), l1_opt7));
    EXPECT(same_path(planner.shortcutPath(l1_opt7), plain.shortcutPath(l1_opt7)));

    if (fails) { std::fprintf(stderr, "metric_clearance_test: %d checks failed\n", fails); return 1; }
    std::printf("metric_clearance_test ok\n");
    return 0;
}
