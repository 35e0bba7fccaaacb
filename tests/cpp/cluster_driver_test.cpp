// cluster_driver_test.cpp -- drives OccupancyGridSLAMT (include/botlab/slam_driver.hpp) in localization-only mode with
// setGlobalLocalization(true) from an event script written by tests/test_gpu_cluster_driver.py ('O' odometry, 'L' lidar: the
// format of global_localization_test.cpp).  argv[4] = "cluster": setGlobalLocalizationByCluster with the bins and the share read
// from argv[5..7] (bin_xy, theta_bins, minShare); "spread": the whole-cloud rule on the same inputs.  The driver is never told where
// the robot starts.  After every iteration it writes: 'I', converged, map equal to the loaded file, map updates so far, current
// pose (utime, x, y, theta), the pose last published, the heaviest cluster's share (0 under the spread rule).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "dropin_test_types.hpp"
#include <botlab/slam_driver.hpp>

struct odometry_t { int64_t utime = 0; float x = 0, y = 0, theta = 0; };
typedef botlab_hip::OccupancyGridSLAMT<pose_xyt_t, lidar_t, odometry_t, particle_t, particles_t, occupancy_grid_t> SLAM;

static void rd(FILE* f, void* p, size_t n) { if (fread(p, 1, n, f) != n) { std::fprintf(stderr, "short read\n"); std::exit(2); } }

static std::vector<int8_t> cells_of(const botlab_hip::OccupancyGrid& m)
{
    std::vector<int8_t> v;
    v.reserve(static_cast<size_t>(m.widthInCells()) * m.heightInCells());
    for (int y = 0; y < m.heightInCells(); ++y) for (int x = 0; x < m.widthInCells(); ++x) v.push_back(m(x, y));
    return v;
}

int main(int argc, char** argv)
{
    if (argc < 5) return 2;
    const bool by_cluster = std::strcmp(argv[4], "cluster") == 0;
    if (by_cluster && argc < 8) return 2;
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[3], "wb");
    if (!in || !out) return 2;
    int32_t nparticles, nevents;
    rd(in, &nparticles, 4); rd(in, &nevents, 4);
    int published_pose = 0;
    pose_xyt_t published;
    SLAM::Publisher pub;
    pub.slamPose = [&](const pose_xyt_t& p) { ++published_pose; published = p; };
    SLAM slam(nparticles, 4, 1, pub, false, false, false, argv[2]);
    slam.setGlobalLocalization(true);
    if (by_cluster) {
        bl_pf_cluster_params_t q;
        q.bin_xy = std::atof(argv[5]); q.theta_bins = std::atoi(argv[6]); q.max_clusters = 1;
        slam.setGlobalLocalizationByCluster(q, std::atof(argv[7]));
    }
    const std::vector<int8_t> loaded = cells_of(slam.map());
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
            const bool was = slam.globalLocalizationConverged();
            slam.runSLAMIteration();
            ++iterations;
            const pose_xyt_t c = slam.currentPose();
            const int32_t st[3] = {slam.globalLocalizationConverged() ? 1 : 0, cells_of(slam.map()) == loaded ? 1 : 0, slam.mapUpdateCount()};
            const double share = by_cluster && !was ? slam.globalCluster().share : 0.0;
            std::fwrite("I", 1, 1, out);
            std::fwrite(st, 4, 3, out);
            std::fwrite(&c.utime, 8, 1, out); std::fwrite(&c.x, 4, 1, out); std::fwrite(&c.y, 4, 1, out); std::fwrite(&c.theta, 4, 1, out);
            std::fwrite(&published.x, 4, 1, out); std::fwrite(&published.y, 4, 1, out); std::fwrite(&published.theta, 4, 1, out);
            std::fwrite(&share, 8, 1, out);
        }
    }
    std::fwrite("E", 1, 1, out);
    std::fclose(out);
    std::printf("cluster_driver_test ok: %d iterations, %d poses published\n", iterations, published_pose);
    return 0;
}
