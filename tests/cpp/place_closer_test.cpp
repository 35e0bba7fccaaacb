// place_closer_test.cpp -- LoopCloserT::findPlaces / places (include/botlab/loop_closer.hpp) and OccupancyGridSLAMT::closeLoopsByPlace
// (slam_driver.hpp), driven by tests/test_gpu_place_cpp.py.
//   the script is tests/test_gpu_slam_driver.py's ('P' pose, 'L' lidar); the parameter file: bl_loopclose_params_t, bl_place_params_t,
//   6 doubles chain information, double gate, bl_posegraph_params_t, int32 capacity, max rays per scan.
//   place_closer_test find <script> <params> <output>
//     a ScanHistoryT of every (pose, lidar) pair of the script, LoopCloserT::findPlaces.  Output: int32 M, M x bl_loopclose_candidate_t;
//     int32 K, K x bl_posegraph_edge_t; int32 Q, Q x bl_place_t; per candidate its submap's origin (2 floats) and cells.
//   place_closer_test driver <script> <params> <output>
//     Two mapping-only runs with a history of `capacity` scans from the same start: 'a' never calls closeLoopsByPlace, 'b' calls it
//     after its last iteration.  Output per run: 'R', tag, per iteration 'I' and the pose; 'E' and the map as the run left it.  Then
//     for 'b': 'h', the history's size and recorded poses; 'g', the call's return value and lastPoseGraphResult(); the history's poses
//     after; 'm', the driver's map after.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include "dropin_test_types.hpp"
#include <botlab/loop_closer.hpp>
#include <botlab/slam_driver.hpp>

struct odometry_t { int64_t utime = 0; float x = 0, y = 0, theta = 0; };
typedef botlab_hip::OccupancyGridSLAMT<pose_xyt_t, lidar_t, odometry_t, particle_t, particles_t, occupancy_grid_t> SLAM;
typedef botlab_hip::LoopCloserT<pose_xyt_t, lidar_t> Closer;
struct Event { char kind; pose_xyt_t pose; lidar_t scan; };
struct Params {
    bl_loopclose_params_t lc; bl_place_params_t place; double chain[6]; double gate; bl_posegraph_params_t graph; int32_t capacity, max_rays;
};

static void rd(FILE* f, void* p, size_t n) { if (n && fread(p, 1, n, f) != n) { std::fprintf(stderr, "short read\n"); std::exit(2); } }
static void write_pose(FILE* out, const pose_xyt_t& c)
{
    std::fwrite(&c.utime, 8, 1, out); std::fwrite(&c.x, 4, 1, out); std::fwrite(&c.y, 4, 1, out); std::fwrite(&c.theta, 4, 1, out);
}
static void write_map(FILE* out, const botlab_hip::OccupancyGrid& m)
{
    for (int y = 0; y < m.heightInCells(); ++y) for (int x = 0; x < m.widthInCells(); ++x) { const int8_t v = m(x, y); std::fwrite(&v, 1, 1, out); }
}

static bool read_inputs(const char* scriptPath, const char* paramsPath, std::vector<Event>& events, Params& prm)
{
    FILE* in = std::fopen(scriptPath, "rb");
    if (!in) return false;
    int32_t hdr[4];
    rd(in, hdr, 16);
    events.resize(static_cast<size_t>(hdr[2]));
    for (Event& e : events) {
        rd(in, &e.kind, 1);
        if (e.kind == 'P') { rd(in, &e.pose.utime, 8); rd(in, &e.pose.x, 4); rd(in, &e.pose.y, 4); rd(in, &e.pose.theta, 4); }
        else if (e.kind == 'L') {
            int32_t n; rd(in, &e.scan.utime, 8); rd(in, &n, 4);
            e.scan.num_ranges = n; e.scan.ranges.resize(n); e.scan.thetas.resize(n); e.scan.times.resize(n);
            rd(in, e.scan.ranges.data(), 4 * n); rd(in, e.scan.thetas.data(), 4 * n); rd(in, e.scan.times.data(), 8 * n);
        } else { std::fprintf(stderr, "unknown event %c\n", e.kind); return false; }
    }
    std::fclose(in);
    in = std::fopen(paramsPath, "rb");
    if (!in) return false;
    rd(in, &prm.lc, sizeof(prm.lc)); rd(in, &prm.place, sizeof(prm.place)); rd(in, prm.chain, 48); rd(in, &prm.gate, 8); rd(in, &prm.graph, sizeof(prm.graph));
    rd(in, &prm.capacity, 4); rd(in, &prm.max_rays, 4);
    std::fclose(in);
    return true;
}

static int run_find(const std::vector<Event>& events, const Params& prm, const char* outPath)
{
    FILE* out = std::fopen(outPath, "wb");
    if (!out) return 2;
    botlab_hip::ScanHistoryT<pose_xyt_t, lidar_t> history(prm.capacity, prm.max_rays);
    pose_xyt_t pose;
    for (const Event& e : events) {
        if (e.kind == 'P') pose = e.pose;
        else if (!history.append(e.scan, pose)) { std::fprintf(stderr, "append refused\n"); return 1; }
    }
    botlab_hip::OccupancyGrid like(6.0f, 6.0f, 0.05f);
    Closer closer(128);
    const std::vector<bl_posegraph_edge_t> edges = closer.findPlaces(history, like, prm.lc, prm.place);
    const std::vector<bl_loopclose_candidate_t> cands = closer.candidates();
    const std::vector<bl_place_t> places = closer.places();
    const int32_t M = static_cast<int32_t>(cands.size()), K = static_cast<int32_t>(edges.size()), Q = static_cast<int32_t>(places.size());
    std::fwrite(&M, 4, 1, out); std::fwrite(cands.data(), sizeof(bl_loopclose_candidate_t), cands.size(), out);
    std::fwrite(&K, 4, 1, out); std::fwrite(edges.data(), sizeof(bl_posegraph_edge_t), edges.size(), out);
    std::fwrite(&Q, 4, 1, out); std::fwrite(places.data(), sizeof(bl_place_t), places.size(), out);
    for (int m = 0; m < M; ++m) {
        float origin[2];
        const std::vector<int8_t> cells = closer.submap(m, origin);
        std::fwrite(origin, 4, 2, out); std::fwrite(cells.data(), 1, cells.size(), out);
    }
    if (closer.edges().size() != edges.size()) { std::fprintf(stderr, "edges() disagrees with findPlaces()\n"); return 1; }
    std::fclose(out);
    std::printf("place_closer_test ok: %d candidates, %d edges, %d queries, %.3f ms\n", (int)M, (int)K, (int)Q, closer.lastDeviceMs());
    return 0;
}

static std::unique_ptr<SLAM> run_driver(FILE* out, char tag, const std::vector<Event>& events, int capacity)
{
    std::srand(1);
    SLAM::Publisher pub;
    std::unique_ptr<SLAM> slamp(new SLAM(200, 3, 1, pub, false, true, false, std::string()));
    SLAM& slam = *slamp;
    slam.setScanHistory(capacity);
    std::fwrite("R", 1, 1, out); std::fwrite(&tag, 1, 1, out);
    for (const Event& e : events) {
        if (e.kind == 'P') slam.handlePose(e.pose); else slam.handleLaser(e.scan);
        while (slam.isReadyToUpdate()) {
            slam.runSLAMIteration();
            std::fwrite("I", 1, 1, out);
            write_pose(out, slam.currentPose());
        }
    }
    std::fwrite("E", 1, 1, out);
    write_map(out, slam.map());
    return slamp;
}

static int run_driver_mode(const std::vector<Event>& events, const Params& prm, const char* outPath)
{
    FILE* out = std::fopen(outPath, "wb");
    if (!out) return 2;
    {
        std::unique_ptr<SLAM> a = run_driver(out, 'a', events, prm.capacity);
        const bl_posegraph_result_t& r = a->lastPoseGraphResult();
        if (r.tries != 0 || r.status != 0 || r.cost_before != 0.0) { std::fprintf(stderr, "a result without a call\n"); return 1; }
        SLAM::Publisher pub;
        SLAM none(200, 3, 1, pub, false, true, false, std::string());
        if (none.closeLoopsByPlace(prm.lc, prm.place, prm.chain, prm.gate, prm.graph) != 0) { std::fprintf(stderr, "closeLoopsByPlace without a history did something\n"); return 1; }
    }
    std::unique_ptr<SLAM> b = run_driver(out, 'b', events, prm.capacity);
    const int32_t held = b->scanHistory()->size();
    std::fwrite("h", 1, 1, out); std::fwrite(&held, 4, 1, out);
    for (const pose_xyt_t& p : b->scanHistory()->poses()) write_pose(out, p);
    const int32_t kept = b->closeLoopsByPlace(prm.lc, prm.place, prm.chain, prm.gate, prm.graph);
    const bl_posegraph_result_t res = b->lastPoseGraphResult();
    std::fwrite("g", 1, 1, out); std::fwrite(&kept, 4, 1, out); std::fwrite(&res, sizeof(res), 1, out);
    for (const pose_xyt_t& p : b->scanHistory()->poses()) write_pose(out, p);
    std::fwrite("m", 1, 1, out);
    write_map(out, b->map());
    std::fclose(out);
    std::printf("place_closer_test ok: driver, %d scans held, %d edges kept, cost %.6g -> %.6g\n", (int)held, (int)kept, res.cost_before, res.cost_after);
    return 0;
}

int main(int argc, char** argv)
{
    std::vector<Event> events;
    Params prm;
    if (argc == 5 && (!std::strcmp(argv[1], "find") || !std::strcmp(argv[1], "driver"))) {
        if (!read_inputs(argv[2], argv[3], events, prm)) return 2;
        return !std::strcmp(argv[1], "find") ? run_find(events, prm, argv[4]) : run_driver_mode(events, prm, argv[4]);
    }
    std::fprintf(stderr, "usage: place_closer_test find|driver script params output\n");
    return 2;
}
