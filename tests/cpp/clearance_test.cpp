// clearance_test.cpp -- ClearanceGridT (include/botlab/clearance_grid.hpp), BeamModelT::scoresLeap / debugLeap / reweighLeap,
// ParticleFilterT::reweighBeamLeap and OccupancyGridSLAMT::setBeamLeapCast, driven by tests/test_gpu_clearance_cpp.py.
//
// clearance_test model input output
//   Input:  width, height (int32), meters_per_cell, origin x, y (float), the cells (int8), bl_beam_params_t (56 bytes), cap (int32),
//           rays (int32), ranges, thetas (float each), poses (int32) and their x, y, theta (float), particles (int32) and that many
//           bl_particle_t.
//   Output: 'I' bl_clearance_info_t;  'D' the whole grid (uint8 each);  'S' the scores by leaps (int64 each) and their units (uint32
//           each);  'C' the used rays (int32) and first, K, z, z*, p, rounds of pose 0;  'F' the poses reweighBeamLeap and
//           BeamModelT::reweighLeap return and poseEstimate() (x, y, theta float each), the units (uint32 per particle) and the weights
//           of particles() (double each);  'E'.
// clearance_test driver script output map
//   The event scripts of tests/test_gpu_slam_driver.py in localization-only mode on the map file, as tests/cpp/range_table_test.cpp
//   runs them, each run from srand(1) and the same filter seed: 'n' no switch touched, 'o' setBeamLeapCast(false), 'B' setBeamModel(true),
//   'b' that and setBeamLeapCast(false), 'L' setBeamModel(true) and setBeamLeapCast(true), 't' setBeamModel(true) and
//   setBeamRangeTable(true), 'T' that and setBeamLeapCast(true).
//   Output per run: 'R', the tag, per iteration 'I', the pose and the bookkeeping, 'P' and the particles (x, y, theta float, weight
//   double each);  'E', the final counts, the map, and whether the beam model was active, the grid's builds, updates and reweighs, the
//   table's reweighs, and whether the driver's grid equals a fresh build on the final map (1, 0; -1 without a grid) (int32 each).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "dropin_test_types.hpp"
#include <botlab/clearance_grid.hpp>
#include <botlab/slam_driver.hpp>

typedef botlab_hip::BeamModelT<pose_xyt_t, lidar_t> Beam;
typedef botlab_hip::ClearanceGridT<pose_xyt_t, lidar_t> Clearance;
typedef botlab_hip::ParticleFilterT<pose_xyt_t, lidar_t, particle_t, particles_t> Filter;
struct odometry_t { int64_t utime = 0; float x = 0, y = 0, theta = 0; };
typedef botlab_hip::OccupancyGridSLAMT<pose_xyt_t, lidar_t, odometry_t, particle_t, particles_t, occupancy_grid_t> SLAM;
struct Event { char kind; odometry_t odo; lidar_t scan; };

static void rd(FILE* f, void* p, size_t n) { if (fread(p, 1, n, f) != n) { std::fprintf(stderr, "short read\n"); std::exit(2); } }

static int run_model(FILE* in, FILE* out)
{
    occupancy_grid_t msg;
    rd(in, &msg.width, 4); rd(in, &msg.height, 4); rd(in, &msg.meters_per_cell, 4); rd(in, &msg.origin_x, 4); rd(in, &msg.origin_y, 4);
    msg.num_cells = msg.width * msg.height;
    msg.cells.resize(static_cast<size_t>(msg.num_cells));
    rd(in, msg.cells.data(), msg.cells.size());
    botlab_hip::OccupancyGrid map;
    map.fromLCM(msg);
    bl_beam_params_t p;
    rd(in, &p, sizeof(p));
    int32_t cap = 0;
    rd(in, &cap, 4);
    Beam beam(p);
    Clearance grid(cap);
    if (grid.info().built != 0) { std::fprintf(stderr, "a fresh grid says it is built\n"); return 1; }
    grid.build(map, p.occ_min);
    const bl_clearance_info_t info = grid.info();
    const std::vector<uint8_t> D = grid.read(0, 0, msg.width, msg.height);
    std::fwrite("I", 1, 1, out); std::fwrite(&info, sizeof(info), 1, out);
    std::fwrite("D", 1, 1, out); std::fwrite(D.data(), 1, D.size(), out);
    grid.update(map, 1, 1, 2, 2);                                           // nothing changed: the grid stays what it is
    if (grid.read(0, 0, msg.width, msg.height) != D) { std::fprintf(stderr, "an update over unchanged cells changed the grid\n"); return 1; }
    lidar_t scan;
    rd(in, &scan.num_ranges, 4);
    scan.ranges.resize(static_cast<size_t>(scan.num_ranges)); scan.thetas.resize(scan.ranges.size()); scan.times.assign(scan.ranges.size(), 0);
    rd(in, scan.ranges.data(), 4 * scan.ranges.size()); rd(in, scan.thetas.data(), 4 * scan.thetas.size());
    int32_t np = 0;
    rd(in, &np, 4);
    std::vector<pose_xyt_t> poses(static_cast<size_t>(np));
    for (int32_t i = 0; i < np; ++i) { rd(in, &poses[i].x, 4); rd(in, &poses[i].y, 4); rd(in, &poses[i].theta, 4); }
    const std::vector<int64_t> S = beam.scoresLeap(grid, scan, poses);
    const std::vector<uint32_t> U = beam.units(np);
    std::fwrite("S", 1, 1, out); std::fwrite(S.data(), 8, S.size(), out); std::fwrite(U.data(), 4, U.size(), out);
    std::vector<int32_t> rounds;
    const botlab_hip::BeamCast c = beam.debugLeap(grid, scan, poses[0], &rounds);
    const int32_t r = static_cast<int32_t>(c.p.size());
    std::fwrite("C", 1, 1, out); std::fwrite(&r, 4, 1, out);
    std::fwrite(c.first.data(), 4, c.first.size(), out); std::fwrite(c.K.data(), 4, c.K.size(), out); std::fwrite(c.z.data(), 4, c.z.size(), out);
    std::fwrite(c.zstar.data(), 4, c.zstar.size(), out); std::fwrite(c.p.data(), 4, c.p.size(), out); std::fwrite(rounds.data(), 4, rounds.size(), out);
    int32_t n = 0;
    rd(in, &n, 4);
    std::vector<bl_particle_t> cloud(static_cast<size_t>(n));
    rd(in, cloud.data(), sizeof(bl_particle_t) * cloud.size());
    Filter pf(n), pf2(n);
    botlab_hip::check(bl_pf_set_particles(pf.device(), cloud.data(), nullptr), "bl_pf_set_particles");
    botlab_hip::check(bl_pf_set_particles(pf2.device(), cloud.data(), nullptr), "bl_pf_set_particles");
    const pose_xyt_t est = pf.reweighBeamLeap(beam, grid, scan);
    const pose_xyt_t est2 = beam.reweighLeap(pf2, grid, scan);
    const pose_xyt_t again = pf.poseEstimate();
    const float ef[9] = {est.x, est.y, est.theta, est2.x, est2.y, est2.theta, again.x, again.y, again.theta};
    const std::vector<uint32_t> fu = beam.units(n);
    const particles_t ps = pf.particles();
    std::fwrite("F", 1, 1, out); std::fwrite(ef, 4, 9, out); std::fwrite(fu.data(), 4, fu.size(), out);
    for (int32_t i = 0; i < n; ++i) std::fwrite(&ps.particles[static_cast<size_t>(i)].weight, 8, 1, out);
    std::fwrite("E", 1, 1, out);
    return 0;
}

// beam: setBeamModel(true);  leap: 0 untouched, 1 setBeamLeapCast(false), 2 setBeamLeapCast(true);  table: setBeamRangeTable(true)
static void run_driver(FILE* out, char tag, bool beam, int leap, bool table, int nparticles, const std::string& mapfile, const std::vector<Event>& events)
{
    std::srand(1);
    int published_pose = 0, published_map = 0;
    SLAM::Publisher pub;
    pub.slamPose = [&](const pose_xyt_t&) { ++published_pose; };
    pub.slamMap = [&](const occupancy_grid_t&) { ++published_map; };
    particles_t cloud;                                                      // the last cloud published
    pub.slamParticles = [&](const particles_t& ps) { cloud = ps; };
    SLAM slam(nparticles, 4, 1, pub, false, false, false, mapfile);
    slam.setFilterSeed(20240607ull);
    if (beam) slam.setBeamModel(true);
    if (leap == 1) slam.setBeamLeapCast(false, 16);
    if (leap == 2) slam.setBeamLeapCast(true);
    if (table) slam.setBeamRangeTable(true);
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
            std::fwrite("P", 1, 1, out);
            for (const particle_t& q : cloud.particles) {
                std::fwrite(&q.pose.x, 4, 1, out); std::fwrite(&q.pose.y, 4, 1, out); std::fwrite(&q.pose.theta, 4, 1, out); std::fwrite(&q.weight, 8, 1, out);
            }
        }
    }
    if (!out) return;
    const int32_t fin[5] = {slam.numIgnoredScans(), (int32_t)slam.queuedScans(), slam.mapUpdateCount(), published_pose, published_map};
    std::fwrite("E", 1, 1, out); std::fwrite(fin, 4, 5, out);
    const botlab_hip::OccupancyGrid& m = slam.map();
    for (int y = 0; y < m.heightInCells(); ++y) for (int x = 0; x < m.widthInCells(); ++x) { const int8_t v = m(x, y); std::fwrite(&v, 1, 1, out); }
    int32_t same = -1;
    if (slam.beamLeapGrid()) {
        const bl_clearance_info_t i = slam.beamLeapGrid()->info();
        Clearance fresh(i.cap);
        fresh.build(m, i.occ_min);
        same = fresh.read(0, 0, i.width, i.height) == slam.beamLeapGrid()->read(0, 0, i.width, i.height) ? 1 : 0;
    }
    const int32_t tail[6] = {slam.beamModelActive() ? 1 : 0, slam.beamLeapBuilds(), slam.beamLeapUpdates(), slam.beamLeapReweighs(),
                             slam.beamRangeTableReweighs(), same};
    std::fwrite(tail, 4, 6, out);
}

static int run_drivers(FILE* in, FILE* out, const std::string& mapfile)
{
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
    // Runs that write nothing come first, one per path through the driver (beam_driver_test.cpp says why).
    run_driver(nullptr, 'w', true, 2, true, nparticles, mapfile, events);
    run_driver(nullptr, 'w', false, 0, false, nparticles, mapfile, events);
    run_driver(out, 'n', false, 0, false, nparticles, mapfile, events);
    run_driver(out, 'o', false, 1, false, nparticles, mapfile, events);
    run_driver(out, 'B', true, 0, false, nparticles, mapfile, events);
    run_driver(out, 'b', true, 1, false, nparticles, mapfile, events);
    run_driver(out, 'L', true, 2, false, nparticles, mapfile, events);
    run_driver(out, 't', true, 0, true, nparticles, mapfile, events);
    run_driver(out, 'T', true, 2, true, nparticles, mapfile, events);
    return 0;
}

int main(int argc, char** argv)
{
    const bool model = argc >= 4 && std::strcmp(argv[1], "model") == 0, driver = argc >= 5 && std::strcmp(argv[1], "driver") == 0;
    if (!model && !driver) { std::fprintf(stderr, "usage: clearance_test model input output | driver script output map\n"); return 2; }
    FILE* in = std::fopen(argv[2], "rb");
    FILE* out = std::fopen(argv[3], "wb");
    if (!in || !out) { std::fprintf(stderr, "cannot open files\n"); return 2; }
    const int rc = model ? run_model(in, out) : run_drivers(in, out, argv[4]);
    std::fclose(out); std::fclose(in);
    if (rc == 0) std::printf("clearance_test ok\n");
    return rc;
}
