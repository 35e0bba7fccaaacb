// rb_slam.hpp -- RaoBlackwellizedSLAMT: the Rao-Blackwellized grid SLAM of libbotlab_hip.so (bl_rbslam_*, botlab_hip.h) for C++ hosts:
// a particle filter in which every particle owns a map built from its own trajectory and is weighed against it.  No reference
// counterpart; header-only over the C ABI and templated over the message types like the rest of include/botlab/.
#ifndef BOTLAB_RB_SLAM_HPP
#define BOTLAB_RB_SLAM_HPP

#include <cstdint>
#include <cstdlib>
#include <vector>

#include <botlab/botlab_dropin.hpp>

namespace botlab_hip {

template <class Pose, class Lidar, class Particle, class Particles>
class RaoBlackwellizedSLAMT {
public:
    // every particle's map has the shape and frame of `like` (its cells are not used)
    RaoBlackwellizedSLAMT(int numParticles, const OccupancyGrid& like, float maxLaserDistance, int8_t hitOdds, int8_t missOdds)
        : h_(nullptr), n_(numParticles), frame_(like)
    {
        frame_.reset();
        const PointT<float> o = like.originInGlobalFrame();
        check(bl_rbslam_create(default_ctx(), numParticles, like.widthInCells(), like.heightInCells(), like.metersPerCell(), like.cellsPerMeter(),
                               o.x, o.y, maxLaserDistance, hitOdds, missOdds, &h_), "bl_rbslam_create");
        last_ = bl_rbslam_result_t();
    }
    ~RaoBlackwellizedSLAMT() { if (h_) bl_rbslam_destroy(h_); }
    RaoBlackwellizedSLAMT(const RaoBlackwellizedSLAMT&) = delete;
    RaoBlackwellizedSLAMT& operator=(const RaoBlackwellizedSLAMT&) = delete;

    // resampling is due when den * (sum u)^2 <= num * P * sum u^2: 1 / 1 on every moved update, the default 1 / 2 at N_eff <= P / 2
    void setResampling(uint32_t num, uint32_t den) { check(bl_rbslam_set_resampling(h_, num, den), "bl_rbslam_set_resampling"); }
    void setNoiseSeed(uint64_t seed) { check(bl_rbslam_set_noise_seed(h_, seed), "bl_rbslam_set_noise_seed"); }
    // scan-matched proposals (GMapping's structure): after the action of a moved update every particle matches the scan against its own
    // map in the window +-nx, +-ny cells, +-ntheta steps of dtheta around its pose and moves to the best pose there, if that scores at
    // least minScore.  Off by default.
    void setScanMatching(int nx = 2, int ny = 2, int ntheta = 4, float dtheta = 0.00872664626f, float maxRange = 8.0f, int minScore = 0)
    {
        bl_rbslam_match_params_t p;
        p.nx = nx; p.ny = ny; p.ntheta = ntheta; p.dtheta = dtheta; p.max_range = maxRange; p.min_score = minScore;
        check(bl_rbslam_set_scan_matching(h_, &p), "bl_rbslam_set_scan_matching");
    }
    void clearScanMatching() { check(bl_rbslam_set_scan_matching(h_, nullptr), "bl_rbslam_set_scan_matching"); }
    void initializeAtPose(const Pose& pose, uint64_t seed = 0)
    {
        const bl_pose_xyt_t p = pose_in(pose);
        check(bl_rbslam_init_at_pose(h_, &p, seed), "bl_rbslam_init_at_pose");
    }
    void setParticles(const std::vector<Particle>& particles, const std::vector<int64_t>* cumScores = nullptr)
    {
        std::vector<bl_particle_t> in(particles.size());
        for (size_t i = 0; i < in.size(); ++i) {
            in[i].pose = pose_in(particles[i].pose); in[i].parent_pose = pose_in(particles[i].parent_pose); in[i].weight = particles[i].weight;
        }
        if (static_cast<int>(in.size()) != n_ || (cumScores && cumScores->size() != in.size())) { std::fprintf(stderr, "botlab_hip: setParticles: wrong count\n"); std::abort(); }
        check(bl_rbslam_set_particles(h_, in.data(), cumScores ? cumScores->data() : nullptr), "bl_rbslam_set_particles");
    }
    // one update; the SLAM pose is the best particle's.  noise: 3 * numParticles samples (rot1, trans, rot2) in place of the device's own
    Pose update(const Pose& odometry, const Lidar& scan) { return update(odometry, scan, std::rand(), nullptr); }
    Pose update(const Pose& odometry, const Lidar& scan, int randValue, const std::vector<float>* noise)
    {
        const bl_pose_xyt_t o = pose_in(odometry);
        const bl_lidar_t v = lidar_view(scan);
        check(bl_rbslam_update(h_, &o, &v, randValue, noise ? noise->data() : nullptr, &last_), "bl_rbslam_update");
        return pose_out<Pose>(last_.best_pose);
    }
    const bl_rbslam_result_t& lastResult() const { return last_; }
    // the best particle's map, copied on the device into an ordinary grid: MotionPlanner::setMap, the frontier search and the view gain take it
    OccupancyGrid bestMap() const
    {
        OccupancyGrid g(frame_);
        check(bl_rbslam_best_map(h_, g.device()), "bl_rbslam_best_map");
        g.markDeviceWritten();
        return g;
    }
    Particles particles() const
    {
        std::vector<bl_particle_t> out(static_cast<size_t>(n_));
        check(bl_rbslam_get_particles(h_, out.data(), nullptr, nullptr), "bl_rbslam_get_particles");
        Particles ps;
        ps.num_particles = n_;
        ps.particles.resize(out.size());
        for (size_t i = 0; i < out.size(); ++i) {
            ps.particles[i].pose = pose_out<Pose>(out[i].pose); ps.particles[i].parent_pose = pose_out<Pose>(out[i].parent_pose);
            ps.particles[i].weight = out[i].weight;
        }
        ps.utime = out.empty() ? 0 : out[0].pose.utime;
        return ps;
    }
    int numParticles() const { return n_; }
    bl_rbslam* device() const { return h_; }

private:
    bl_rbslam* h_;
    int n_;
    OccupancyGrid frame_;
    bl_rbslam_result_t last_;
};

}  // namespace botlab_hip

#endif  // BOTLAB_RB_SLAM_HPP
