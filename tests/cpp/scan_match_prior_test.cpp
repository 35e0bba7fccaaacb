// scan_match_prior_test.cpp -- the C++ layer of the scan match with a prior (include/botlab/scan_matcher.hpp,
// include/botlab/slam_driver.hpp), driven by tests/test_gpu_scan_match_prior_cpp.py.  Three modes:
//   sigmas sx sy rho st score_per_nat mpc dtheta
//       prints the four coefficients of scan_match_prior_from_sigmas (no device).
//   match mapfile casefile out
//       ScanMatcherT::matchWithPrior on a map file and a case (centre: 3 floats; bl_scan_match_params_t; bl_scan_match_prior_t;
//       ray count; ranges; thetas).  Writes the result (56 bytes), the moments (112 bytes), the volume's size and the volume.
//   drive script mapfile|- out prior|- subcell dump min_score
//       OccupancyGridSLAMT with setScanMatching from an event script ('O' odometry, 'L' lidar: the format of
//       scan_match_driver_test.cpp), "-" for full SLAM from an empty map.  prior: "a_xx,a_xy,a_yy,a_tt,half_life,want_moments" for
//       setScanMatchingPrior, "-" to leave it unset; subcell: setScanMatchingSubCell.  Before an iteration (when asked): 'M', width,
//       height, cells.  After every iteration: 'I', lastScanMatch() (56 bytes), lastScanMatchMoments() (112 bytes), matches and map
//       updates so far, the current pose and correctedPose() (utime, x, y, theta each).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "dropin_test_types.hpp"
#include <botlab/slam_driver.hpp>

struct odometry_t { int64_t utime = 0; float x = 0, y = 0, theta = 0; };
typedef botlab_hip::OccupancyGridSLAMT<pose_xyt_t, lidar_t, odometry_t, particle_t, particles_t, occupancy_grid_t> SLAM;
typedef botlab_hip::ScanMatcherT<pose_xyt_t, lidar_t> Matcher;

static_assert(sizeof(bl_scan_match_result_t) == 56 && sizeof(bl_scan_match_moments_t) == 112 && sizeof(bl_scan_match_prior_t) == 24 &&
              sizeof(bl_scan_match_params_t) == 28, "layout");

static void rd(FILE* f, void* p, size_t n) { if (fread(p, 1, n, f) != n) { std::fprintf(stderr, "short read\n"); std::exit(2); } }

static void write_pose(FILE* out, const pose_xyt_t& c)
{
    std::fwrite(&c.utime, 8, 1, out); std::fwrite(&c.x, 4, 1, out); std::fwrite(&c.y, 4, 1, out); std::fwrite(&c.theta, 4, 1, out);
}

static int sigmas(char** a)
{
    try {
        const bl_scan_match_prior_t p = botlab_hip::scan_match_prior_from_sigmas(std::atof(a[0]), std::atof(a[1]), std::atof(a[2]), std::atof(a[3]),
                                                                                 std::atof(a[4]), std::atof(a[5]), std::atof(a[6]));
        std::printf("%d %d %d %d %d %d\n", p.a_xx, p.a_xy, p.a_yy, p.a_tt, p.half_life, p.want_moments);
    } catch (const std::invalid_argument&) {
        std::printf("invalid\n");
    }
    return 0;
}

static int match(char** a)
{
    botlab_hip::OccupancyGrid map;
    if (!map.loadFromFile(a[0])) return 2;
    FILE* in = std::fopen(a[1], "rb");
    FILE* out = std::fopen(a[2], "wb");
    if (!in || !out) return 2;
    pose_xyt_t centre; centre.utime = 7;
    bl_scan_match_params_t params; bl_scan_match_prior_t prior; int32_t n;
    rd(in, &centre.x, 4); rd(in, &centre.y, 4); rd(in, &centre.theta, 4);
    rd(in, &params, sizeof params); rd(in, &prior, sizeof prior); rd(in, &n, 4);
    lidar_t s; s.utime = 4321; s.num_ranges = n; s.ranges.resize(n); s.thetas.resize(n); s.times.assign(n, 0);
    rd(in, s.ranges.data(), 4 * n); rd(in, s.thetas.data(), 4 * n);
    Matcher m;
    bl_scan_match_moments_t mom = bl_scan_match_moments_t();
    const bl_scan_match_result_t r = m.matchWithPrior(s, centre, map, params, prior, &mom);
    const std::vector<int32_t> vol = m.volume();
    const int32_t nv = static_cast<int32_t>(vol.size());
    std::fwrite(&r, sizeof r, 1, out); std::fwrite(&mom, sizeof mom, 1, out); std::fwrite(&nv, 4, 1, out);
    std::fwrite(vol.data(), 4, vol.size(), out);
    // without the moments nothing is kept, and the result is the same
    bl_scan_match_prior_t plain = prior; plain.want_moments = 0;
    const bl_scan_match_result_t r2 = m.matchWithPrior(s, centre, map, params, plain);
    const int32_t after[2] = {std::memcmp(&r, &r2, sizeof r) == 0 ? 1 : 0, m.volume().empty() ? 1 : 0};
    std::fwrite(after, 4, 2, out);
    std::fclose(out);
    std::printf("scan_match_prior_test ok: match\n");
    return 0;
}

static int drive(char** a)
{
    FILE* in = std::fopen(a[0], "rb");
    FILE* out = std::fopen(a[2], "wb");
    if (!in || !out) return 2;
    const std::string mapfile = std::strcmp(a[1], "-") ? a[1] : "";
    const bool subcell = std::atoi(a[4]) != 0, dump = std::atoi(a[5]) != 0;
    int32_t nparticles, nevents;
    rd(in, &nparticles, 4); rd(in, &nevents, 4);
    SLAM::Publisher pub;
    SLAM slam(nparticles, 4, 1, pub, false, false, false, mapfile);
    bl_scan_match_params_t p = botlab_hip::default_scan_match_params();
    p.min_score = std::atoi(a[6]);
    slam.setScanMatching(true, p);
    if (std::strcmp(a[3], "-")) {
        bl_scan_match_prior_t pr;
        if (std::sscanf(a[3], "%d,%d,%d,%d,%d,%d", &pr.a_xx, &pr.a_xy, &pr.a_yy, &pr.a_tt, &pr.half_life, &pr.want_moments) != 6) return 2;
        slam.setScanMatchingPrior(pr);
    }
    if (subcell) slam.setScanMatchingSubCell(true);
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
            const bl_scan_match_result_t r = slam.lastScanMatch();
            const bl_scan_match_moments_t m = slam.lastScanMatchMoments();
            const int32_t st[2] = {slam.scanMatchCount(), slam.mapUpdateCount()};
            std::fwrite("I", 1, 1, out);
            std::fwrite(&r, sizeof r, 1, out);
            std::fwrite(&m, sizeof m, 1, out);
            std::fwrite(st, 4, 2, out);
            write_pose(out, slam.currentPose());
            write_pose(out, slam.correctedPose());
        }
    }
    std::fwrite("E", 1, 1, out);
    std::fclose(out);
    std::printf("scan_match_prior_test ok: %d iterations\n", iterations);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 9 && !std::strcmp(argv[1], "sigmas")) return sigmas(argv + 2);
    if (argc == 5 && !std::strcmp(argv[1], "match")) return match(argv + 2);
    if (argc == 9 && !std::strcmp(argv[1], "drive")) return drive(argv + 2);
    return 2;
}
