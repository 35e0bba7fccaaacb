// rb_slam_match_test: RaoBlackwellizedSLAMT (include/botlab/rb_slam.hpp) with setScanMatching on a short recorded run: matching is on
// until update `off_from`, then cleared.  Reads the run from argv[1] (written by tests/test_gpu_rb_slam_match_cpp.py), writes the result
// of every update, the best map and the particles to argv[2].
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>

#include <botlab/rb_slam.hpp>
#include "dropin_test_types.hpp"

typedef botlab_hip::RaoBlackwellizedSLAMT<pose_xyt_t, lidar_t, particle_t, particles_t> RBSlam;

template <class T> static T rd(std::ifstream& in) { T v; in.read(reinterpret_cast<char*>(&v), sizeof(T)); return v; }
template <class T> static void wr(std::ofstream& out, const T& v) { out.write(reinterpret_cast<const char*>(&v), sizeof(T)); }
static pose_xyt_t rd_pose(std::ifstream& in) { pose_xyt_t p; p.utime = rd<int64_t>(in); p.x = rd<float>(in); p.y = rd<float>(in); p.theta = rd<float>(in); return p; }
static void wr_pose(std::ofstream& out, const pose_xyt_t& p) { wr(out, p.utime); wr(out, p.x); wr(out, p.y); wr(out, p.theta); }

int main(int argc, char** argv)
{
    if (argc < 4) { std::fprintf(stderr, "usage: rb_slam_match_test run.bin out.bin map.map\n"); return 2; }
    std::ifstream in(argv[1], std::ios::binary);
    std::ofstream out(argv[2], std::ios::binary);
    botlab_hip::OccupancyGrid like;
    if (!in.is_open() || !out.is_open() || !like.loadFromFile(argv[3])) return 2;
    const int32_t P = rd<int32_t>(in), K = rd<int32_t>(in), R = rd<int32_t>(in), num = rd<int32_t>(in), den = rd<int32_t>(in);
    const float maxLaser = rd<float>(in);
    const int32_t hit = rd<int32_t>(in), miss = rd<int32_t>(in);
    RBSlam slam(P, like, maxLaser, static_cast<int8_t>(hit), static_cast<int8_t>(miss));
    slam.setResampling(num, den);
    const int32_t nx = rd<int32_t>(in), ny = rd<int32_t>(in), ntheta = rd<int32_t>(in);
    const float dtheta = rd<float>(in), maxRange = rd<float>(in);
    const int32_t minScore = rd<int32_t>(in), offFrom = rd<int32_t>(in);
    slam.setScanMatching(nx, ny, ntheta, dtheta, maxRange, minScore);
    slam.initializeAtPose(rd_pose(in), 1);
    std::vector<particle_t> parts(P);
    for (int i = 0; i < P; ++i) { parts[i].pose = rd_pose(in); parts[i].parent_pose = rd_pose(in); parts[i].weight = rd<double>(in); }
    slam.setParticles(parts);
    for (int k = 0; k < K; ++k) {
        if (k == offFrom) slam.clearScanMatching();
        const pose_xyt_t odo = rd_pose(in);
        const int32_t rnd = rd<int32_t>(in);
        lidar_t scan;
        scan.utime = odo.utime; scan.num_ranges = R;
        scan.ranges.resize(R); scan.thetas.resize(R); scan.times.resize(R);
        in.read(reinterpret_cast<char*>(scan.ranges.data()), R * 4);
        in.read(reinterpret_cast<char*>(scan.thetas.data()), R * 4);
        in.read(reinterpret_cast<char*>(scan.times.data()), R * 8);
        std::vector<float> noise(3 * P);
        in.read(reinterpret_cast<char*>(noise.data()), noise.size() * 4);
        const pose_xyt_t pose = slam.update(odo, scan, rnd, &noise);
        const bl_rbslam_result_t& r = slam.lastResult();
        wr(out, r.moved); wr(out, r.resampled); wr(out, r.best);
        wr_pose(out, pose);
    }
    if (!in.good()) { std::fprintf(stderr, "short input\n"); return 2; }
    const botlab_hip::OccupancyGrid best = slam.bestMap();
    for (int y = 0; y < best.heightInCells(); ++y)
        for (int x = 0; x < best.widthInCells(); ++x) wr(out, best.logOdds(x, y));
    const particles_t ps = slam.particles();
    for (const particle_t& p : ps.particles) { wr_pose(out, p.pose); wr_pose(out, p.parent_pose); }
    std::printf("rb_slam_match_test ok\n");
    return 0;
}
