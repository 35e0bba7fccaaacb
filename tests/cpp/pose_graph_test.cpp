// pose_graph_test.cpp -- PoseGraphT (include/botlab/pose_graph.hpp) and OccupancyGridSLAMT::optimizeHistory (slam_driver.hpp), driven by
// tests/test_gpu_pose_graph_cpp.py.
//   pose_graph_test graph <case> <output>
//     case: int32 N, L, S, words; bl_posegraph_params_t; N x (int64 utime, float x, y, theta); (N - 1 + L) x bl_posegraph_edge_t;
//     S x words uint32 masks (S = 0: none, one subset with every loop edge on).  Output per subset: bl_posegraph_result_t, 3 N doubles,
//     N x (int64, 3 floats), N - 1 + L doubles chi2 before, the same after.
//   pose_graph_test driver <mapping-only script> <loops> <output>
//     the script is tests/test_gpu_slam_driver.py's ('P' true pose, 'L' lidar); loops: int32 L, 6 doubles chain information,
//     bl_posegraph_params_t, L x bl_posegraph_edge_t.  Two mapping-only runs with a history of 256 scans from the same start: 'a' never
//     calls optimizeHistory, 'b' calls it after its last iteration.  Output per run: 'R', tag, per iteration 'I' and the pose; 'E' and
//     the map as the run left it.  Then for 'b': 'h', the history's size and recorded poses; 'g', optimizeHistory's return value and
//     lastPoseGraphResult(); the history's poses after; 'm', the driver's map after.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include "dropin_test_types.hpp"
#include <botlab/pose_graph.hpp>
#include <botlab/slam_driver.hpp>

struct odometry_t { int64_t utime = 0; float x = 0, y = 0, theta = 0; };
typedef botlab_hip::OccupancyGridSLAMT<pose_xyt_t, lidar_t, odometry_t, particle_t, particles_t, occupancy_grid_t> SLAM;
struct Event { char kind; pose_xyt_t pose; lidar_t scan; };

static void rd(FILE* f, void* p, size_t n) { if (n && fread(p, 1, n, f) != n) { std::fprintf(stderr, "short read\n"); std::exit(2); } }
static void write_pose(FILE* out, const pose_xyt_t& c)
{
    std::fwrite(&c.utime, 8, 1, out); std::fwrite(&c.x, 4, 1, out); std::fwrite(&c.y, 4, 1, out); std::fwrite(&c.theta, 4, 1, out);
}
static void write_map(FILE* out, const botlab_hip::OccupancyGrid& m)
{
    for (int y = 0; y < m.heightInCells(); ++y) for (int x = 0; x < m.widthInCells(); ++x) { const int8_t v = m(x, y); std::fwrite(&v, 1, 1, out); }
}

static int run_graph(const char* casePath, const char* outPath)
{
    FILE* in = std::fopen(casePath, "rb");
    FILE* out = std::fopen(outPath, "wb");
    if (!in || !out) return 2;
    int32_t hdr[4];
    rd(in, hdr, 16);
    const int N = hdr[0], L = hdr[1], S = hdr[2], words = hdr[3];
    bl_posegraph_params_t prm;
    rd(in, &prm, sizeof(prm));
    std::vector<pose_xyt_t> nodes(static_cast<size_t>(N));
    for (pose_xyt_t& p : nodes) { rd(in, &p.utime, 8); rd(in, &p.x, 4); rd(in, &p.y, 4); rd(in, &p.theta, 4); }
    std::vector<bl_posegraph_edge_t> chain(static_cast<size_t>(N - 1)), loops(static_cast<size_t>(L));
    rd(in, chain.data(), chain.size() * sizeof(bl_posegraph_edge_t));
    rd(in, loops.data(), loops.size() * sizeof(bl_posegraph_edge_t));
    std::vector<uint32_t> masks(static_cast<size_t>(S * words));
    rd(in, masks.data(), masks.size() * 4);
    std::fclose(in);
    botlab_hip::PoseGraphT<pose_xyt_t> g(N, L, S > 0 ? S : 1);
    g.setNodes(nodes);
    g.setChain(chain);
    g.setLoops(loops);
    if (S > 0) g.solve(prm, S, masks); else g.solve(prm);
    const std::vector<bl_posegraph_result_t> res = g.results();
    for (size_t s = 0; s < res.size(); ++s) {
        std::vector<double> xyt, before, after;
        const std::vector<pose_xyt_t> p = g.poses(static_cast<int>(s), &xyt);
        g.edgeChi2(static_cast<int>(s), before, after);
        std::fwrite(&res[s], sizeof(bl_posegraph_result_t), 1, out);
        std::fwrite(xyt.data(), 8, xyt.size(), out);
        for (const pose_xyt_t& q : p) write_pose(out, q);
        std::fwrite(before.data(), 8, before.size(), out);
        std::fwrite(after.data(), 8, after.size(), out);
    }
    std::fclose(out);
    std::printf("pose_graph_test ok: %d nodes, %d loop edges, %d subsets, %.3f ms\n", N, L, (int)res.size(), g.lastDeviceMs());
    return 0;
}

static std::unique_ptr<SLAM> run_driver(FILE* out, char tag, const std::vector<Event>& events)
{
    std::srand(1);
    SLAM::Publisher pub;
    std::unique_ptr<SLAM> slamp(new SLAM(200, 3, 1, pub, false, true, false, std::string()));
    SLAM& slam = *slamp;
    slam.setScanHistory(256);
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

static int run_driver_mode(const char* scriptPath, const char* loopsPath, const char* outPath)
{
    FILE* in = std::fopen(scriptPath, "rb");
    if (!in) return 2;
    int32_t hdr[4];
    rd(in, hdr, 16);
    std::vector<Event> events(static_cast<size_t>(hdr[2]));
    for (Event& e : events) {
        rd(in, &e.kind, 1);
        if (e.kind == 'P') { rd(in, &e.pose.utime, 8); rd(in, &e.pose.x, 4); rd(in, &e.pose.y, 4); rd(in, &e.pose.theta, 4); }
        else if (e.kind == 'L') {
            int32_t n; rd(in, &e.scan.utime, 8); rd(in, &n, 4);
            e.scan.num_ranges = n; e.scan.ranges.resize(n); e.scan.thetas.resize(n); e.scan.times.resize(n);
            rd(in, e.scan.ranges.data(), 4 * n); rd(in, e.scan.thetas.data(), 4 * n); rd(in, e.scan.times.data(), 8 * n);
        } else { std::fprintf(stderr, "unknown event %c\n", e.kind); return 2; }
    }
    std::fclose(in);
    in = std::fopen(loopsPath, "rb");
    if (!in) return 2;
    int32_t L;
    double chainInfo[6];
    bl_posegraph_params_t prm;
    rd(in, &L, 4); rd(in, chainInfo, 48); rd(in, &prm, sizeof(prm));
    std::vector<bl_posegraph_edge_t> loops(static_cast<size_t>(L));
    rd(in, loops.data(), loops.size() * sizeof(bl_posegraph_edge_t));
    std::fclose(in);
    FILE* out = std::fopen(outPath, "wb");
    if (!out) return 2;
    {
        std::unique_ptr<SLAM> a = run_driver(out, 'a', events);
        const bl_posegraph_result_t& r = a->lastPoseGraphResult();
        if (r.tries != 0 || r.status != 0 || r.cost_before != 0.0) { std::fprintf(stderr, "a result without a call\n"); return 1; }
        SLAM::Publisher pub;
        SLAM none(200, 3, 1, pub, false, true, false, std::string());
        if (none.optimizeHistory(loops, chainInfo, prm)) { std::fprintf(stderr, "optimizeHistory without a history did something\n"); return 1; }
    }
    std::unique_ptr<SLAM> b = run_driver(out, 'b', events);
    const int32_t held = b->scanHistory()->size();
    std::fwrite("h", 1, 1, out); std::fwrite(&held, 4, 1, out);
    for (const pose_xyt_t& p : b->scanHistory()->poses()) write_pose(out, p);
    const int32_t did = b->optimizeHistory(loops, chainInfo, prm) ? 1 : 0;
    const bl_posegraph_result_t res = b->lastPoseGraphResult();
    std::fwrite("g", 1, 1, out); std::fwrite(&did, 4, 1, out); std::fwrite(&res, sizeof(res), 1, out);
    for (const pose_xyt_t& p : b->scanHistory()->poses()) write_pose(out, p);
    std::fwrite("m", 1, 1, out);
    write_map(out, b->map());
    std::fclose(out);
    std::printf("pose_graph_test ok: driver, %d scans held, cost %.6g -> %.6g\n", (int)held, res.cost_before, res.cost_after);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 4 && !std::strcmp(argv[1], "graph")) return run_graph(argv[2], argv[3]);
    if (argc == 5 && !std::strcmp(argv[1], "driver")) return run_driver_mode(argv[2], argv[3], argv[4]);
    std::fprintf(stderr, "usage: pose_graph_test graph case output | driver script loops output\n");
    return 2;
}
