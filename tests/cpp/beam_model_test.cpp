// beam_model_test.cpp -- BeamModelT (include/botlab/beam_model.hpp) and ParticleFilterT::reweighBeam (include/botlab/botlab_dropin.hpp),
// driven by tests/test_gpu_beam_cpp.py.  Arguments: input, output.
// Input:  width, height (int32), meters_per_cell, origin x, y (float), the cells (int8), bl_beam_params_t (56 bytes), rays (int32),
//         ranges, thetas (float each), poses (int32) and their x, y, theta (float), particles (int32) and that many bl_particle_t.
// Output: 'S' the scores (int64 each) and their units (uint32 each);  'C' the used rays (int32) and first, K, z, z*, p of pose 0;
//         'T' Rand, MaxFree, MaxBlocked, LN2, reach;  'F' the pose reweighBeam returns and poseEstimate() (x, y, theta float each), the
//         units (uint32 per particle) and the weights of particles() (double each);  'H' whether there is a heaviest cluster (int32) and
//         its mean_x, mean_y, share (double);  'E'.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "dropin_test_types.hpp"
#include <botlab/beam_model.hpp>

typedef botlab_hip::BeamModelT<pose_xyt_t, lidar_t> Beam;
typedef botlab_hip::ParticleFilterT<pose_xyt_t, lidar_t, particle_t, particles_t> Filter;

static void rd(FILE* f, void* p, size_t n) { if (fread(p, 1, n, f) != n) { std::fprintf(stderr, "short read\n"); std::exit(2); } }

int main(int argc, char** argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: beam_model_test input output\n"); return 2; }
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) { std::fprintf(stderr, "cannot open files\n"); return 2; }
    occupancy_grid_t msg;
    rd(in, &msg.width, 4); rd(in, &msg.height, 4); rd(in, &msg.meters_per_cell, 4); rd(in, &msg.origin_x, 4); rd(in, &msg.origin_y, 4);
    msg.num_cells = msg.width * msg.height;
    msg.cells.resize(static_cast<size_t>(msg.num_cells));
    rd(in, msg.cells.data(), msg.cells.size());
    botlab_hip::OccupancyGrid map;
    map.fromLCM(msg);
    bl_beam_params_t p;
    rd(in, &p, sizeof(p));
    Beam beam(p);
    bl_beam_params_t bad = p;
    bad.z_rand = 0.0f;
    if (beam.setParams(bad)) { std::fprintf(stderr, "bad parameters accepted\n"); return 1; }      // and the model keeps what it had
    lidar_t scan;
    rd(in, &scan.num_ranges, 4);
    scan.ranges.resize(static_cast<size_t>(scan.num_ranges)); scan.thetas.resize(scan.ranges.size()); scan.times.assign(scan.ranges.size(), 0);
    rd(in, scan.ranges.data(), 4 * scan.ranges.size()); rd(in, scan.thetas.data(), 4 * scan.thetas.size());
    int32_t np = 0;
    rd(in, &np, 4);
    std::vector<pose_xyt_t> poses(static_cast<size_t>(np));
    for (int32_t i = 0; i < np; ++i) { rd(in, &poses[i].x, 4); rd(in, &poses[i].y, 4); rd(in, &poses[i].theta, 4); }
    const std::vector<int64_t> S = beam.scores(map, scan, poses);
    const std::vector<uint32_t> U = beam.units(np);
    std::fwrite("S", 1, 1, out); std::fwrite(S.data(), 8, S.size(), out); std::fwrite(U.data(), 4, U.size(), out);
    const botlab_hip::BeamCast c = beam.debugCast(map, scan, poses[0]);
    const int32_t r = static_cast<int32_t>(c.p.size());
    std::fwrite("C", 1, 1, out); std::fwrite(&r, 4, 1, out);
    std::fwrite(c.first.data(), 4, c.first.size(), out); std::fwrite(c.K.data(), 4, c.K.size(), out); std::fwrite(c.z.data(), 4, c.z.size(), out);
    std::fwrite(c.zstar.data(), 4, c.zstar.size(), out); std::fwrite(c.p.data(), 4, c.p.size(), out);
    const botlab_hip::BeamTables t = beam.tables(map.cellsPerMeter());
    const uint32_t sc[5] = {t.rand, t.max_free, t.max_blocked, t.ln2, t.reach};
    std::fwrite("T", 1, 1, out); std::fwrite(sc, 4, 5, out);
    int32_t n = 0;
    rd(in, &n, 4);
    std::vector<bl_particle_t> cloud(static_cast<size_t>(n));
    rd(in, cloud.data(), sizeof(bl_particle_t) * cloud.size());
    Filter pf(n);
    botlab_hip::check(bl_pf_set_particles(pf.device(), cloud.data(), nullptr), "bl_pf_set_particles");
    const pose_xyt_t est = pf.reweighBeam(beam, map, scan);
    const pose_xyt_t again = pf.poseEstimate();
    const float ef[6] = {est.x, est.y, est.theta, again.x, again.y, again.theta};
    const std::vector<uint32_t> fu = beam.units(n);
    const particles_t ps = pf.particles();
    std::fwrite("F", 1, 1, out); std::fwrite(ef, 4, 6, out); std::fwrite(fu.data(), 4, fu.size(), out);
    for (int32_t i = 0; i < n; ++i) std::fwrite(&ps.particles[static_cast<size_t>(i)].weight, 8, 1, out);
    bl_pf_cluster_pose_t h = bl_pf_cluster_pose_t();
    const int32_t have = pf.heaviestCluster(Filter::defaultClusterParams(), &h) ? 1 : 0;
    const double hv[3] = {h.mean_x, h.mean_y, h.share};
    std::fwrite("H", 1, 1, out); std::fwrite(&have, 4, 1, out); std::fwrite(hv, 8, 3, out);
    std::fwrite("E", 1, 1, out);
    std::fclose(out); std::fclose(in);
    std::printf("beam_model_test ok\n");
    return 0;
}
