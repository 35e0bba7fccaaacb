// beam_driver_test.cpp -- OccupancyGridSLAMT::setBeamModel (include/botlab/slam_driver.hpp), driven by tests/test_gpu_beam_cpp.py with
// the event scripts of tests/test_gpu_slam_driver.py ('O' odometry, 'L' lidar; after every event the driver runs while ready), in
// localization-only mode on the map file given.  Arguments: script, output, map file.
// One binary runs the script three times from srand(1) and the same filter seed, so that two runs that do the same work write the same
// bytes: 'n' the switch never touched, 'o' setBeamModel(false, ...), 'B' setBeamModel(true).  Output per run: 'R', the tag, per
// iteration 'I', the pose and the bookkeeping;  'E', the final counts, the map, and whether the beam model was active (int32).
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "dropin_test_types.hpp"
#include <botlab/slam_driver.hpp>

struct odometry_t { int64_t utime = 0; float x = 0, y = 0, theta = 0; };
typedef botlab_hip::OccupancyGridSLAMT<pose_xyt_t, lidar_t, odometry_t, particle_t, particles_t, occupancy_grid_t> SLAM;
struct Event { char kind; odometry_t odo; lidar_t scan; };

static void rd(FILE* f, void* p, size_t n) { if (fread(p, 1, n, f) != n) { std::fprintf(stderr, "short read\n"); std::exit(2); } }

// mode 0: switch never touched; 1: setBeamModel(false, ...); 2: setBeamModel(true)
static void run_driver(FILE* out, char tag, int mode, int nparticles, const std::string& mapfile, const std::vector<Event>& events)
{
    std::srand(1);
    int published_pose = 0, published_map = 0;
    SLAM::Publisher pub;
    pub.slamPose = [&](const pose_xyt_t&) { ++published_pose; };
    pub.slamMap = [&](const occupancy_grid_t&) { ++published_map; };
    SLAM slam(nparticles, 4, 1, pub, false, false, false, mapfile);
    slam.setFilterSeed(20240607ull);
    if (mode == 1) slam.setBeamModel(false, botlab_hip::default_beam_params());
    if (mode == 2) slam.setBeamModel(true);
    if (out) { std::fwrite("R", 1, 1, out); std::fwrite(&tag, 1, 1, out); }
    for (const Event& e : events) {
        if (e.kind == 'O') slam.handleOdometry(e.odo); else slam.handleLaser(e.scan);
        while (slam.isReadyToUpdate()) {
            slam.runSLAMIteration();
            if (!out) continue;
            const pose_xyt_t c = slam.currentPose();
            const int32_t st[3] = {slam.numIgnoredScans(), (int32_t)slam.queuedScans(), slam.mapUpdateCount()};
            std::fwrite("I", 1, 1, out);
            std::fwrite(&c.utime, 8, 1, out); std::fwrite(&c.x, 4, 1, out); std::fwrite(&c.y, 4, 1, out); std::fwrite(&c.theta, 4, 1, out);
            std::fwrite(st, 4, 3, out);
        }
    }
    if (!out) return;
    const int32_t fin[5] = {slam.numIgnoredScans(), (int32_t)slam.queuedScans(), slam.mapUpdateCount(), published_pose, published_map};
    std::fwrite("E", 1, 1, out); std::fwrite(fin, 4, 5, out);
    const botlab_hip::OccupancyGrid& m = slam.map();
    for (int y = 0; y < m.heightInCells(); ++y) for (int x = 0; x < m.widthInCells(); ++x) { const int8_t v = m(x, y); std::fwrite(&v, 1, 1, out); }
    const int32_t active = slam.beamModelActive() ? 1 : 0;
    std::fwrite(&active, 4, 1, out);
}

int main(int argc, char** argv)
{
    if (argc < 4) { std::fprintf(stderr, "usage: beam_driver_test script output map\n"); return 2; }
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int32_t mode, nparticles, nevents, wait_opti;
    rd(in, &mode, 4); rd(in, &nparticles, 4); rd(in, &nevents, 4); rd(in, &wait_opti, 4);
    std::vector<Event> events(static_cast<size_t>(nevents));
    for (Event& e : events) {
        rd(in, &e.kind, 1);
        if (e.kind == 'O') { rd(in, &e.odo.utime, 8); rd(in, &e.odo.x, 4); rd(in, &e.odo.y, 4); rd(in, &e.odo.theta, 4); }
        else if (e.kind == 'L') {
            int32_t n; rd(in, &e.scan.utime, 8); rd(in, &n, 4);
            e.scan.num_ranges = n; e.scan.ranges.resize(n); e.scan.thetas.resize(n); e.scan.times.resize(n);
            rd(in, e.scan.ranges.data(), 4 * n); rd(in, e.scan.thetas.data(), 4 * n); rd(in, e.scan.times.data(), 8 * n);
        } else { std::fprintf(stderr, "unknown event %c\n", e.kind); return 2; }
    }
    const std::string mapfile = argv[3];
    // Two runs that write nothing come first, one per path through the driver: the updates take rand() as the reference does, one
    // sequence per process, and whatever the runtime does when a kernel is first used must not fall into one compared run alone.
    run_driver(nullptr, 'w', 2, nparticles, mapfile, events);
    run_driver(nullptr, 'w', 0, nparticles, mapfile, events);
    run_driver(out, 'n', 0, nparticles, mapfile, events);
    run_driver(out, 'o', 1, nparticles, mapfile, events);
    run_driver(out, 'B', 2, nparticles, mapfile, events);
    std::fclose(out); std::fclose(in);
    std::printf("beam_driver_test ok\n");
    return 0;
}
