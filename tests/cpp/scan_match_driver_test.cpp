// scan_match_driver_test.cpp -- drives OccupancyGridSLAMT (include/botlab/slam_driver.hpp) with setScanMatching from an event
// script written by tests/test_gpu_scan_match_driver.py: 'O' odometry, 'L' lidar (the format of slam_driver_test.cpp).
// Arguments: script, map file ("-" for full SLAM from an empty map), output, matching on (0 / 1), dump the map before every
// iteration (0 / 1), min_score.  Before an iteration (when asked): 'M', width, height, cells.  After every iteration: 'I', the
// bl_scan_match_result_t of lastScanMatch() (56 bytes), matches so far, map updates so far, current pose (utime, x, y, theta).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "dropin_test_types.hpp"
#include <botlab/slam_driver.hpp>

struct odometry_t { int64_t utime = 0; float x = 0, y = 0, theta = 0; };
typedef botlab_hip::OccupancyGridSLAMT<pose_xyt_t, lidar_t, odometry_t, particle_t, particles_t, occupancy_grid_t> SLAM;

static void rd(FILE* f, void* p, size_t n) { if (fread(p, 1, n, f) != n) { std::fprintf(stderr, "short read\n"); std::exit(2); } }

int main(int argc, char** argv)
{
    if (argc < 7) return 2;
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[3], "wb");
    if (!in || !out) return 2;
    const bool matching = std::atoi(argv[4]) != 0, dump = std::atoi(argv[5]) != 0;
    const std::string mapfile = std::strcmp(argv[2], "-") ? argv[2] : "";
    int32_t nparticles, nevents;
    rd(in, &nparticles, 4); rd(in, &nevents, 4);
    SLAM::Publisher pub;
    SLAM slam(nparticles, 4, 1, pub, false, false, false, mapfile);
    bl_scan_match_params_t p = botlab_hip::default_scan_match_params();
    p.min_score = std::atoi(argv[6]);
    if (matching) slam.setScanMatching(true, p);
    static_assert(sizeof(bl_scan_match_result_t) == 56, "layout");
    int iterations = 0;
    for (int e = 0; e < nevents; ++e) {
        char kind; rd(in, &kind, 1);
        if (kind == 'O') {
            odometry_t o; rd(in, &o.utime, 8); rd(in, &o.x, 4); rd(in, &o.y, 4); rd(in, &o.theta, 4);
            slam.handleOdometry(o);
        } else if (kind == 'L') {
            lidar_t s; int32_t n; rd(in, &s.utime, 8); rd(in, &n, 4);
            s.num_ranges = n; s.ranges.resize(n); s.thetas.resize(n); s.times.resize(n);
            rd(in, s.ranges.data(), 4 * n); rd(in, s.thetas.data(), 4 * n); rd(in, s.times.data(), 8 * n);
            slam.handleLaser(s);
        } else {
            std::fprintf(stderr, "unknown event %c\n", kind);
            return 2;
        }
        while (slam.isReadyToUpdate()) {
            if (dump) {
                const occupancy_grid_t g = slam.map().toLCM<occupancy_grid_t>();
                std::fwrite("M", 1, 1, out);
                std::fwrite(&g.width, 4, 1, out); std::fwrite(&g.height, 4, 1, out);
                std::fwrite(g.cells.data(), 1, g.cells.size(), out);
            }
            slam.runSLAMIteration();
            ++iterations;
            const pose_xyt_t c = slam.currentPose();
            const bl_scan_match_result_t r = slam.lastScanMatch();
            const int32_t st[2] = {slam.scanMatchCount(), slam.mapUpdateCount()};
            std::fwrite("I", 1, 1, out);
            std::fwrite(&r, sizeof(r), 1, out);
            std::fwrite(st, 4, 2, out);
            std::fwrite(&c.utime, 8, 1, out); std::fwrite(&c.x, 4, 1, out); std::fwrite(&c.y, 4, 1, out); std::fwrite(&c.theta, 4, 1, out);
        }
    }
    std::fwrite("E", 1, 1, out);
    std::fclose(out);
    std::printf("scan_match_driver_test ok: %d iterations\n", iterations);
    return 0;
}
