// likelihood_field_test.cpp -- LikelihoodFieldT (include/botlab/likelihood_field.hpp) and OccupancyGridSLAMT::setLikelihoodField
// (include/botlab/slam_driver.hpp), driven by tests/test_gpu_likelihood_field_cpp.py from an event script: 'O' odometry, 'L'
// lidar (the format of slam_driver_test.cpp).  Arguments: script, map file ("-" for full SLAM from an empty map), output.
// Every run starts from srand(1) and the same filter seed, so two runs that do the same work publish the same poses.
// Output, one section per run -- 'R', a tag byte, the count, then (utime, x, y, theta) per published SLAM pose, then the final map
// and the final sensor map (width, height, cells each):
//   'F'  the driver with setLikelihoodField(true)          'H'  a hand-written loop over the classes
//   'o'  the driver with setLikelihoodField(false)         'n'  the driver, switch never touched
// then 'C': LikelihoodFieldT against the C ABI on the final map of 'F' (1 if the cells and the tables are equal), the table;
// then, with a map file, 'S': the matches of a run with the switch and setScanMatching both on (run_matching below).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "dropin_test_types.hpp"
#include <botlab/slam_driver.hpp>

struct odometry_t { int64_t utime = 0; float x = 0, y = 0, theta = 0; };
typedef botlab_hip::OccupancyGridSLAMT<pose_xyt_t, lidar_t, odometry_t, particle_t, particles_t, occupancy_grid_t> SLAM;
typedef botlab_hip::ParticleFilterT<pose_xyt_t, lidar_t, particle_t, particles_t> Filter;
typedef botlab_hip::MappingT<pose_xyt_t, lidar_t> Mapper;

static const uint64_t kSeed = 20240607ull;

struct Event { char kind; odometry_t odo; lidar_t scan; };

static void rd(FILE* f, void* p, size_t n) { if (fread(p, 1, n, f) != n) { std::fprintf(stderr, "short read\n"); std::exit(2); } }

static void put_grid(FILE* out, const botlab_hip::OccupancyGrid& g)
{
    const occupancy_grid_t m = g.toLCM<occupancy_grid_t>();
    std::fwrite(&m.width, 4, 1, out); std::fwrite(&m.height, 4, 1, out);
    std::fwrite(m.cells.data(), 1, m.cells.size(), out);
}

static void put_run(FILE* out, char tag, const std::vector<pose_xyt_t>& poses, const botlab_hip::OccupancyGrid& map, const botlab_hip::OccupancyGrid& sensor)
{
    const int32_t n = static_cast<int32_t>(poses.size());
    std::fwrite("R", 1, 1, out); std::fwrite(&tag, 1, 1, out); std::fwrite(&n, 4, 1, out);
    for (const pose_xyt_t& p : poses) { std::fwrite(&p.utime, 8, 1, out); std::fwrite(&p.x, 4, 1, out); std::fwrite(&p.y, 4, 1, out); std::fwrite(&p.theta, 4, 1, out); }
    put_grid(out, map);
    put_grid(out, sensor);
}

// mode 0: switch never touched; 1: setLikelihoodField(false); 2: setLikelihoodField(true)
static void run_driver(FILE* out, char tag, int mode, int nparticles, const std::string& mapfile, const std::vector<Event>& events,
                       const bl_lfield_params_t& p, botlab_hip::OccupancyGrid* final_map)
{
    std::srand(1);
    std::vector<pose_xyt_t> poses;
    SLAM::Publisher pub;
    pub.slamPose = [&poses](const pose_xyt_t& q) { poses.push_back(q); };
    SLAM slam(nparticles, 4, 1, pub, false, false, false, mapfile);
    slam.setFilterSeed(kSeed);
    if (mode) slam.setLikelihoodField(mode == 2, p);
    for (const Event& e : events) {
        if (e.kind == 'O') slam.handleOdometry(e.odo); else slam.handleLaser(e.scan);
        while (slam.isReadyToUpdate()) slam.runSLAMIteration();
    }
    if (slam.likelihoodFieldActive() != (mode == 2)) { std::fprintf(stderr, "likelihoodFieldActive() is wrong\n"); std::exit(3); }
    if (out) put_run(out, tag, poses, slam.map(), slam.sensorMap());
    if (final_map) *final_map = slam.map();
}

// What the driver does under the switch, written out over the classes: the field, updateFilter on the field, updateMap on the map.
static void run_by_hand(FILE* out, int nparticles, const std::string& mapfile, const std::vector<Event>& events, const bl_lfield_params_t& p)
{
    std::srand(1);
    std::vector<pose_xyt_t> poses;
    botlab_hip::OccupancyGrid grid(10.0f, 10.0f, 0.05f);
    const bool from_file = !mapfile.empty() && grid.loadFromFile(mapfile);
    Filter pf(nparticles);
    Mapper mapping(5.0f, 4, 1);
    botlab_hip::LikelihoodFieldT lf(p);
    botlab_hip::PoseTraceT<pose_xyt_t> odom;
    bool started = false, map_known = from_file;
    pose_xyt_t now;
    for (const Event& e : events) {
        if (e.kind == 'O') {
            pose_xyt_t q; q.utime = e.odo.utime; q.x = e.odo.x; q.y = e.odo.y; q.theta = e.odo.theta;
            odom.addPose(q);
            continue;
        }
        const lidar_t& scan = e.scan;
        const pose_xyt_t odo = odom.poseAt(scan.times.back());
        if (!started) {
            pose_xyt_t before;                                    // the start pose: the origin
            before.utime = scan.times.front();
            now = before;
            now.utime = scan.times.back();
            pf.initializeFilterAtPose(before, kSeed);
            lf.compute(grid);
            started = true;
        }
        if (map_known) {
            now = pf.updateFilter(odo, scan, lf.grid());
            poses.push_back(now);
        }
        mapping.updateMap(scan, now, grid);
        if (!from_file) lf.compute(grid);
        map_known = true;
    }
    put_run(out, 'H', poses, grid, lf.grid());
}

// The switch and setScanMatching together (localization-only: the field is that of the map as loaded): 'S', the count, then the
// bl_scan_match_result_t of every iteration's match (56 bytes each).
static void run_matching(FILE* out, int nparticles, const std::string& mapfile, const std::vector<Event>& events, const bl_lfield_params_t& p)
{
    std::srand(1);
    SLAM::Publisher pub;
    SLAM slam(nparticles, 4, 1, pub, false, false, false, mapfile);
    slam.setFilterSeed(kSeed);
    slam.setLikelihoodField(true, p);
    slam.setScanMatching(true, botlab_hip::default_scan_match_params());
    std::vector<bl_scan_match_result_t> results;
    for (const Event& e : events) {
        if (e.kind == 'O') slam.handleOdometry(e.odo); else slam.handleLaser(e.scan);
        while (slam.isReadyToUpdate()) { slam.runSLAMIteration(); results.push_back(slam.lastScanMatch()); }
    }
    static_assert(sizeof(bl_scan_match_result_t) == 56, "layout");
    const int32_t n = static_cast<int32_t>(results.size());
    std::fwrite("S", 1, 1, out); std::fwrite(&n, 4, 1, out);
    std::fwrite(results.data(), sizeof(bl_scan_match_result_t), results.size(), out);
}

static void class_against_c_abi(FILE* out, const botlab_hip::OccupancyGrid& map, const bl_lfield_params_t& p)
{
    botlab_hip::LikelihoodFieldT lf(p);
    const occupancy_grid_t a = lf.compute(map).toLCM<occupancy_grid_t>();
    const std::vector<int8_t> ta = lf.table();
    bl_lfield* h = nullptr;
    botlab_hip::check(bl_lfield_create(botlab_hip::default_ctx(), &h), "bl_lfield_create");
    botlab_hip::check(bl_lfield_set_params(h, &p), "bl_lfield_set_params");
    botlab_hip::check(bl_lfield_compute(h, map.device()), "bl_lfield_compute");
    std::vector<int8_t> b(a.cells.size()), tb(4098);
    int n = 0, w = 0, hgt = 0;
    botlab_hip::check(bl_grid_shape(bl_lfield_grid(h), &w, &hgt), "bl_grid_shape");
    botlab_hip::check(bl_grid_download(const_cast<bl_grid*>(bl_lfield_grid(h)), b.data()), "bl_grid_download");
    botlab_hip::check(bl_lfield_table(h, tb.data(), &n), "bl_lfield_table");
    tb.resize(static_cast<size_t>(n));
    bl_lfield_destroy(h);
    const botlab_hip::OccupancyGrid copy(lf.grid());              // a copy of the view owns its cells
    const occupancy_grid_t c = copy.toLCM<occupancy_grid_t>();
    const int32_t same = (w == a.width && hgt == a.height && a.cells == b && ta == tb && c.cells == a.cells && lf.lastDeviceMs() > 0.0f) ? 1 : 0;
    const int32_t tn = static_cast<int32_t>(ta.size());
    std::fwrite("C", 1, 1, out); std::fwrite(&same, 4, 1, out); std::fwrite(&tn, 4, 1, out); std::fwrite(ta.data(), 1, ta.size(), out);
}

int main(int argc, char** argv)
{
    if (argc < 4) return 2;
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[3], "wb");
    if (!in || !out) return 2;
    const std::string mapfile = std::strcmp(argv[2], "-") ? argv[2] : "";
    int32_t nparticles, nevents;
    rd(in, &nparticles, 4); rd(in, &nevents, 4);
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
    const bl_lfield_params_t p = botlab_hip::default_lfield_params();
    botlab_hip::OccupancyGrid final_map;
    // Two runs that write nothing come first, one per path through the driver (call by call, fused step).  The updates take
    // rand() as the reference does, and that is one sequence per process: whatever the runtime does when a kernel is used for the
    // first time must not sit between a run's srand(1) and its updates in one of the runs compared and not in the other.
    run_driver(nullptr, 'w', 2, nparticles, mapfile, events, p, nullptr);
    run_driver(nullptr, 'w', 0, nparticles, mapfile, events, p, nullptr);
    run_driver(out, 'F', 2, nparticles, mapfile, events, p, &final_map);
    run_by_hand(out, nparticles, mapfile, events, p);
    run_driver(out, 'o', 1, nparticles, mapfile, events, p, nullptr);
    run_driver(out, 'n', 0, nparticles, mapfile, events, p, nullptr);
    class_against_c_abi(out, final_map, p);
    if (!mapfile.empty()) run_matching(out, nparticles, mapfile, events, p);
    std::fwrite("E", 1, 1, out);
    std::fclose(out);
    std::printf("likelihood_field_test ok\n");
    return 0;
}
