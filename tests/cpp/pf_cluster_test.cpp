// pf_cluster_test.cpp -- ParticleFilterT::clusters / heaviestCluster (include/botlab/botlab_dropin.hpp) on a cloud written by
// tests/test_gpu_pf_cluster_cpp.py: int32 n, then n records (x, y, theta as floats, units as uint32); then bin_xy (double),
// theta_bins, max_clusters (int32).  Writes: bl_pf_clusters_t as returned, n labels, has-pose (int32), bl_pf_cluster_pose_t of
// heaviestCluster, bl_pf_spread_t.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "dropin_test_types.hpp"

typedef botlab_hip::ParticleFilterT<pose_xyt_t, lidar_t, particle_t, particles_t> Filter;

static void rd(FILE* f, void* p, size_t n) { if (fread(p, 1, n, f) != n) { std::fprintf(stderr, "short read\n"); std::exit(2); } }

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int32_t n;
    rd(in, &n, 4);
    std::vector<bl_particle_t> parts(static_cast<size_t>(n), bl_particle_t());
    std::vector<uint32_t> units(static_cast<size_t>(n));
    for (int32_t i = 0; i < n; ++i) {
        float v[3];
        rd(in, v, 12); rd(in, &units[static_cast<size_t>(i)], 4);
        bl_particle_t& p = parts[static_cast<size_t>(i)];
        p.pose.x = p.parent_pose.x = v[0]; p.pose.y = p.parent_pose.y = v[1]; p.pose.theta = p.parent_pose.theta = v[2];
    }
    bl_pf_cluster_params_t q;
    rd(in, &q.bin_xy, 8); rd(in, &q.theta_bins, 4); rd(in, &q.max_clusters, 4);
    Filter pf(n);
    if (bl_pf_set_particles(pf.device(), parts.data(), units.data()) != BL_OK) { std::fprintf(stderr, "%s\n", bl_last_error()); return 1; }
    std::vector<int32_t> labels;
    const bl_pf_clusters_t c = pf.clusters(q, &labels);
    if (static_cast<int32_t>(labels.size()) != n) return 1;
    bl_pf_cluster_pose_t pose = bl_pf_cluster_pose_t();
    const int32_t has = pf.heaviestCluster(q, &pose) ? 1 : 0;
    const bl_pf_spread_t s = pf.spread();
    std::fwrite(&c, sizeof(c), 1, out);
    std::fwrite(labels.data(), 4, labels.size(), out);
    std::fwrite(&has, 4, 1, out);
    std::fwrite(&pose, sizeof(pose), 1, out);
    std::fwrite(&s, sizeof(s), 1, out);
    std::fclose(out);
    std::printf("pf_cluster_test ok: %llu clusters, share %.17g\n", static_cast<unsigned long long>(c.num_clusters), pose.share);
    return 0;
}
