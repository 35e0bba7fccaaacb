// obstacle_layer_test.cpp -- ObstacleLayerT (include/botlab/obstacle_layer.hpp) and MotionPlannerT::setMapWithObstacles
// (include/botlab/planning_dropin.hpp), driven by tests/test_gpu_obstacle_layer_cpp.py.  Arguments: input, output.
// Input:  width, height (int32), meters_per_cell, origin x, y (float), the cells (int8), the five parameters (float, 4 x int32), the
//         number of updates, then per update: rays (int32), ranges, thetas (float each), the pose (x, y, theta float).
// Output: per update 'U', rays, the classes, the stats (40 bytes);  then 'S': n, count, last;  'L': the number of live cells and
//         their x, y;  'G': the composed grid of compose();  'P': the composed grid of setMapWithObstacles and the planner's
//         distances (float per cell);  'E'.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "dropin_test_types.hpp"
#include <botlab/obstacle_layer.hpp>
#include <botlab/planning_dropin.hpp>

typedef botlab_hip::ObstacleLayerT<pose_xyt_t, lidar_t> Layer;
typedef botlab_hip::MotionPlannerT<pose_xyt_t, robot_path_t> Planner;

static void rd(FILE* f, void* p, size_t n) { if (fread(p, 1, n, f) != n) { std::fprintf(stderr, "short read\n"); std::exit(2); } }

static void put_cells(FILE* out, const botlab_hip::OccupancyGrid& g)
{
    for (int y = 0; y < g.heightInCells(); ++y)
        for (int x = 0; x < g.widthInCells(); ++x) { const int8_t v = g.logOdds(x, y); std::fwrite(&v, 1, 1, out); }
}

int main(int argc, char** argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: obstacle_layer_test input output\n"); return 2; }
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) { std::fprintf(stderr, "cannot open files\n"); return 2; }
    occupancy_grid_t msg;
    rd(in, &msg.width, 4); rd(in, &msg.height, 4); rd(in, &msg.meters_per_cell, 4); rd(in, &msg.origin_x, 4); rd(in, &msg.origin_y, 4);
    msg.num_cells = msg.width * msg.height;
    msg.cells.resize(static_cast<size_t>(msg.num_cells));
    rd(in, msg.cells.data(), msg.cells.size());
    botlab_hip::OccupancyGrid map;
    map.fromLCM(msg);
    bl_obslayer_params_t p;
    rd(in, &p.max_range, 4); rd(in, &p.occ_min, 4); rd(in, &p.tol_cells, 4); rd(in, &p.ttl_scans, 4); rd(in, &p.min_hits, 4);
    Layer layer(map.widthInCells(), map.heightInCells(), p);
    bl_obslayer_params_t bad = p;
    bad.tol_cells = 17;
    if (layer.setParams(bad)) { std::fprintf(stderr, "bad parameters accepted\n"); return 1; }      // and the layer keeps what it had
    int32_t updates = 0;
    rd(in, &updates, 4);
    for (int32_t u = 0; u < updates; ++u) {
        lidar_t scan;
        pose_xyt_t pose;
        rd(in, &scan.num_ranges, 4);
        scan.ranges.resize(static_cast<size_t>(scan.num_ranges)); scan.thetas.resize(scan.ranges.size()); scan.times.assign(scan.ranges.size(), 0);
        rd(in, scan.ranges.data(), 4 * scan.ranges.size()); rd(in, scan.thetas.data(), 4 * scan.thetas.size());
        rd(in, &pose.x, 4); rd(in, &pose.y, 4); rd(in, &pose.theta, 4);
        layer.update(map, scan, pose);
        const std::vector<uint8_t> cls = layer.classes();
        const bl_obslayer_stats_t st = layer.stats();
        const int32_t n = static_cast<int32_t>(cls.size());
        std::fwrite("U", 1, 1, out); std::fwrite(&n, 4, 1, out); std::fwrite(cls.data(), 1, cls.size(), out); std::fwrite(&st, sizeof(st), 1, out);
    }
    std::vector<uint8_t> count; std::vector<uint32_t> last; uint32_t n = 0;
    layer.download(count, last, n);
    std::fwrite("S", 1, 1, out); std::fwrite(&n, 4, 1, out);
    std::fwrite(count.data(), 1, count.size(), out); std::fwrite(last.data(), 4, last.size(), out);
    const std::vector<int32_t> live = layer.liveCells();
    const int32_t nl = static_cast<int32_t>(live.size() / 2);
    std::fwrite("L", 1, 1, out); std::fwrite(&nl, 4, 1, out); std::fwrite(live.data(), 4, live.size(), out);
    botlab_hip::OccupancyGrid composed;
    layer.compose(map, composed);
    layer.compose(map, composed);                                     // the second time into the grid as it stands
    std::fwrite("G", 1, 1, out); put_cells(out, composed);
    Planner planner;
    planner.setMapWithObstacles(map, layer);
    std::fwrite("P", 1, 1, out); put_cells(out, planner.composedMap());
    const botlab_hip::ObstacleDistanceGrid& d = planner.distances();
    for (int y = 0; y < d.heightInCells(); ++y)
        for (int x = 0; x < d.widthInCells(); ++x) { const float v = d(x, y); std::fwrite(&v, 4, 1, out); }
    // the map itself is untouched
    for (int y = 0; y < map.heightInCells(); ++y)
        for (int x = 0; x < map.widthInCells(); ++x)
            if (map.logOdds(x, y) != msg.cells[static_cast<size_t>(y) * msg.width + x]) { std::fprintf(stderr, "the map changed\n"); return 1; }
    std::fwrite("E", 1, 1, out);
    std::fclose(out); std::fclose(in);
    std::printf("obstacle_layer_test ok\n");
    return 0;
}
