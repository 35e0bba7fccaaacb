// map_rebuild_driver_test.cpp -- OccupancyGridSLAMT::setScanHistory / rebuildMap (include/botlab/slam_driver.hpp), driven by
// tests/test_gpu_map_rebuild_cpp.py with the event scripts of tests/test_gpu_slam_driver.py ('O' odometry, 'P' true pose, 'L' lidar;
// after every event the driver runs while ready).  Arguments: the full-SLAM script, the mapping-only script (the same scans), output.
// One binary, every run from srand(1) and the same filter seed, so that two runs that do the same work write the same bytes:
//   'n' full SLAM, the switch never touched;  'o' full SLAM, setScanHistory(0);  'H' full SLAM, setScanHistory(64);
//   'M' mapping-only at the true poses, the switch never touched.
// Output per run: 'R', the tag, per iteration 'I', the pose and the bookkeeping; 'E', the final counts, the map.  Then for 'H':
// 'h', the history's size and its recorded poses; 'r', the map after rebuildMap(); 't', the map after rebuildMap(poses) with the poses
// run 'M' mapped at.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>
#include "dropin_test_types.hpp"
#include <botlab/slam_driver.hpp>

struct odometry_t { int64_t utime = 0; float x = 0, y = 0, theta = 0; };
typedef botlab_hip::OccupancyGridSLAMT<pose_xyt_t, lidar_t, odometry_t, particle_t, particles_t, occupancy_grid_t> SLAM;
struct Event { char kind; odometry_t odo; pose_xyt_t pose; lidar_t scan; };

static void rd(FILE* f, void* p, size_t n) { if (fread(p, 1, n, f) != n) { std::fprintf(stderr, "short read\n"); std::exit(2); } }

static void write_pose(FILE* out, const pose_xyt_t& c)
{
    std::fwrite(&c.utime, 8, 1, out); std::fwrite(&c.x, 4, 1, out); std::fwrite(&c.y, 4, 1, out); std::fwrite(&c.theta, 4, 1, out);
}

static void write_map(FILE* out, const botlab_hip::OccupancyGrid& m)
{
    for (int y = 0; y < m.heightInCells(); ++y) for (int x = 0; x < m.widthInCells(); ++x) { const int8_t v = m(x, y); std::fwrite(&v, 1, 1, out); }
}

static std::vector<Event> read_script(const char* path, int32_t* mode, int32_t* nparticles)
{
    FILE* in = std::fopen(path, "rb");
    if (!in) { std::fprintf(stderr, "cannot open %s\n", path); std::exit(2); }
    int32_t nevents, wait_opti;
    rd(in, mode, 4); rd(in, nparticles, 4); rd(in, &nevents, 4); rd(in, &wait_opti, 4);
    std::vector<Event> events(static_cast<size_t>(nevents));
    for (Event& e : events) {
        rd(in, &e.kind, 1);
        if (e.kind == 'O') { rd(in, &e.odo.utime, 8); rd(in, &e.odo.x, 4); rd(in, &e.odo.y, 4); rd(in, &e.odo.theta, 4); }
        else if (e.kind == 'P') { rd(in, &e.pose.utime, 8); rd(in, &e.pose.x, 4); rd(in, &e.pose.y, 4); rd(in, &e.pose.theta, 4); }
        else if (e.kind == 'L') {
            int32_t n; rd(in, &e.scan.utime, 8); rd(in, &n, 4);
            e.scan.num_ranges = n; e.scan.ranges.resize(n); e.scan.thetas.resize(n); e.scan.times.resize(n);
            rd(in, e.scan.ranges.data(), 4 * n); rd(in, e.scan.thetas.data(), 4 * n); rd(in, e.scan.times.data(), 8 * n);
        } else { std::fprintf(stderr, "unknown event %c\n", e.kind); std::exit(2); }
    }
    std::fclose(in);
    return events;
}

// history: -1 the switch never touched, otherwise setScanHistory(history).  mapped: the pose of every iteration that updated the map.
static std::unique_ptr<SLAM> run_driver(FILE* out, char tag, bool mappingOnly, int history, int nparticles, const std::vector<Event>& events,
                                        std::vector<pose_xyt_t>* mapped)
{
    std::srand(1);
    SLAM::Publisher pub;
    std::unique_ptr<SLAM> slamp(new SLAM(nparticles, 4, 1, pub, false, mappingOnly, false, std::string()));
    SLAM& slam = *slamp;
    slam.setFilterSeed(20240607ull);
    if (history >= 0) slam.setScanHistory(history);
    if (out) { std::fwrite("R", 1, 1, out); std::fwrite(&tag, 1, 1, out); }
    for (const Event& e : events) {
        if (e.kind == 'O') slam.handleOdometry(e.odo); else if (e.kind == 'P') slam.handlePose(e.pose); else slam.handleLaser(e.scan);
        while (slam.isReadyToUpdate()) {
            const int before = slam.mapUpdateCount();
            slam.runSLAMIteration();
            const pose_xyt_t c = slam.currentPose();
            if (mapped && slam.mapUpdateCount() > before) mapped->push_back(c);
            if (!out) continue;
            const int32_t st[3] = {slam.numIgnoredScans(), (int32_t)slam.queuedScans(), slam.mapUpdateCount()};
            std::fwrite("I", 1, 1, out);
            write_pose(out, c);
            std::fwrite(st, 4, 3, out);
        }
    }
    if (out) {
        const int32_t fin[5] = {slam.numIgnoredScans(), (int32_t)slam.queuedScans(), slam.mapUpdateCount(), 0, 0};
        std::fwrite("E", 1, 1, out); std::fwrite(fin, 4, 5, out);
        write_map(out, slam.map());
    }
    return slamp;
}

int main(int argc, char** argv)
{
    if (argc < 4) { std::fprintf(stderr, "usage: map_rebuild_driver_test slam_script mapping_script output\n"); return 2; }
    int32_t mode, nparticles, mode_m, np_m;
    const std::vector<Event> slam_events = read_script(argv[1], &mode, &nparticles);
    const std::vector<Event> map_events = read_script(argv[2], &mode_m, &np_m);
    FILE* out = std::fopen(argv[3], "wb");
    if (!out) return 2;
    // Two runs that write nothing come first, one per path through the driver: whatever the runtime does when a kernel is first used
    // must not fall into one compared run alone.
    (void)run_driver(nullptr, 'w', false, 64, nparticles, slam_events, nullptr);
    (void)run_driver(nullptr, 'w', false, -1, nparticles, slam_events, nullptr);
    (void)run_driver(out, 'n', false, -1, nparticles, slam_events, nullptr);
    {
        std::unique_ptr<SLAM> off = run_driver(out, 'o', false, 0, nparticles, slam_events, nullptr);
        if (off->scanHistory() != nullptr) { std::fprintf(stderr, "a history exists with the switch off\n"); return 1; }
    }
    std::vector<pose_xyt_t> mapped_h, mapped_m;
    std::unique_ptr<SLAM> with = run_driver(out, 'H', false, 64, nparticles, slam_events, &mapped_h);
    (void)run_driver(out, 'M', true, -1, np_m, map_events, &mapped_m);
    if (!with->scanHistory()) { std::fprintf(stderr, "no history with the switch on\n"); return 1; }
    const int32_t held = with->scanHistory()->size();
    const std::vector<pose_xyt_t> recorded = with->scanHistory()->poses();
    std::fwrite("h", 1, 1, out); std::fwrite(&held, 4, 1, out);
    for (const pose_xyt_t& p : recorded) write_pose(out, p);
    const int32_t nm = static_cast<int32_t>(mapped_h.size());
    std::fwrite(&nm, 4, 1, out);
    for (const pose_xyt_t& p : mapped_h) write_pose(out, p);
    with->rebuildMap();
    std::fwrite("r", 1, 1, out);
    write_map(out, with->map());
    if (static_cast<int>(mapped_m.size()) != held) { std::fprintf(stderr, "the two runs mapped %d and %d scans\n", (int)mapped_m.size(), (int)held); return 1; }
    with->rebuildMap(mapped_m);
    std::fwrite("t", 1, 1, out);
    write_map(out, with->map());
    const bl_scanlog_stats_t st = with->scanHistory()->stats();
    std::fclose(out);
    std::printf("map_rebuild_driver_test ok: %d scans held, %d chunks, %d pairs\n", (int)held, (int)st.chunks, (int)st.pairs);
    return 0;
}
