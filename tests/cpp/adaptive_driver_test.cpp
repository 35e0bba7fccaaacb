// adaptive_driver_test.cpp -- drives OccupancyGridSLAMT (include/botlab/slam_driver.hpp) in localization-only mode with
// setGlobalLocalization(true) and setAdaptiveParticles(true) from an event script written by tests/test_gpu_adaptive_driver.py: 'O'
// odometry, 'L' lidar (the format of slam_driver_test.cpp).  The driver is never told where the robot starts.  After every
// iteration it writes: 'I', converged, adaptive count on, particles in the current record, current pose (utime, x, y, theta).
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "dropin_test_types.hpp"
#include <botlab/slam_driver.hpp>

struct odometry_t { int64_t utime = 0; float x = 0, y = 0, theta = 0; };
typedef botlab_hip::OccupancyGridSLAMT<pose_xyt_t, lidar_t, odometry_t, particle_t, particles_t, occupancy_grid_t> SLAM;

static void rd(FILE* f, void* p, size_t n) { if (fread(p, 1, n, f) != n) { std::fprintf(stderr, "short read\n"); std::exit(2); } }

int main(int argc, char** argv)
{
    if (argc < 4) return 2;
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[3], "wb");
    if (!in || !out) return 2;
    int32_t nparticles, nevents;
    rd(in, &nparticles, 4); rd(in, &nevents, 4);
    int published_pose = 0;
    SLAM::Publisher pub;
    pub.slamPose = [&](const pose_xyt_t&) { ++published_pose; };
    SLAM slam(nparticles, 4, 1, pub, false, false, false, argv[2]);
    slam.setGlobalLocalization(true);
    slam.setAdaptiveParticles(true);
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
            slam.runSLAMIteration();
            ++iterations;
            const pose_xyt_t c = slam.currentPose();
            const int32_t st[3] = {slam.globalLocalizationConverged() ? 1 : 0, slam.adaptiveParticlesActive() ? 1 : 0, slam.adaptiveState().active};
            std::fwrite("I", 1, 1, out);
            std::fwrite(st, 4, 3, out);
            std::fwrite(&c.utime, 8, 1, out); std::fwrite(&c.x, 4, 1, out); std::fwrite(&c.y, 4, 1, out); std::fwrite(&c.theta, 4, 1, out);
        }
    }
    std::fwrite("E", 1, 1, out);
    std::fclose(out);
    std::printf("adaptive_driver_test ok: %d iterations, %d poses published\n", iterations, published_pose);
    return 0;
}
