// scan_matcher.hpp -- correlative scan matching over the C ABI (bl_scanmatch_*, include/botlab_hip.h): the pose of a scan against
// the map from a bounded window of whole-cell shifts and heading steps around a centre pose, without odometry.  C++11, templated
// on the caller's pose and lidar message types like the other classes of botlab_dropin.hpp.
#ifndef BOTLAB_SCAN_MATCHER_HPP
#define BOTLAB_SCAN_MATCHER_HPP

#include <cmath>
#include <cstddef>
#include <stdexcept>
#include <vector>

#include "botlab_dropin.hpp"

namespace botlab_hip {

// +-4 cells, +-12 steps of half a degree, the simulator's 8 m lidar, every best score accepted
inline bl_scan_match_params_t default_scan_match_params()
{
    bl_scan_match_params_t p;
    p.nx = 4; p.ny = 4; p.ntheta = 12;
    p.dtheta = static_cast<float>(0.5 * M_PI / 180.0);
    p.max_range = 8.0f;
    p.min_score = 0;
    p.keep_volume = 0;
    return p;
}

// the whole map around its middle and the whole circle in steps of a degree, the simulator's 8 m lidar, the library's block size
inline bl_scan_match_wide_params_t whole_map_scan_match_params(const OccupancyGrid& map)
{
    bl_scan_match_wide_params_t p;
    p.nx = (map.widthInCells() + 1) / 2 > 4096 ? 4096 : (map.widthInCells() + 1) / 2;
    p.ny = (map.heightInCells() + 1) / 2 > 4096 ? 4096 : (map.heightInCells() + 1) / 2;
    p.ntheta = 180;
    p.dtheta = static_cast<float>(M_PI / 180.0);
    p.max_range = 8.0f;
    p.min_score = 0;
    p.block_log2 = 0;
    p.exhaustive = 0;
    return p;
}

// The four coefficients of bl_scan_match_prior_t from a Gaussian on the motion since the centre pose: standard deviations
// sigma_x, sigma_y (metres, correlation rho, |rho| < 1) and sigma_theta (radians), all > 0 (infinity: no prior on that axis);
// score_per_nat >= 0 is the number of score units one nat of log-likelihood is worth.  half_life and want_moments are left 0.
// The rule, in double arithmetic: the Gaussian's information matrix in cells and heading steps (s_x = sigma_x / meters_per_cell,
// s_y likewise, s_t = sigma_theta / dtheta, q = 1 - rho^2: 1 / (q s_x^2), -rho / (q s_x s_y), 1 / (q s_y^2), 1 / s_t^2) times
// 256 score_per_nat / 2, each clamped to [0, 32767] (a_xy to [-32767, 32767]; NaN gives 0) and rounded to nearest as
// floor(v + 0.5); then |a_xy| is lowered to floor(sqrt(a_xx a_yy)) if it exceeds it, so that the clamped form is still never
// negative.  Anything else throws std::invalid_argument.
inline bl_scan_match_prior_t scan_match_prior_from_sigmas(double sigma_x, double sigma_y, double rho, double sigma_theta,
                                                          double score_per_nat, double meters_per_cell, double dtheta)
{
    if (!(sigma_x > 0 && sigma_y > 0 && sigma_theta > 0 && std::fabs(rho) < 1 && score_per_nat >= 0))
        throw std::invalid_argument("scan_match_prior_from_sigmas: sigmas must be > 0, |rho| < 1, score_per_nat >= 0");
    struct R {
        static int32_t coeff(double v, double lo)
        {
            if (v != v) return 0;
            v = v < lo ? lo : (v > 32767.0 ? 32767.0 : v);
            return static_cast<int32_t>(std::floor(v + 0.5));
        }
    };
    const double k = 128.0 * score_per_nat;
    const double sx = sigma_x / meters_per_cell, sy = sigma_y / meters_per_cell, st = sigma_theta / dtheta;
    const double q = 1.0 - rho * rho;
    bl_scan_match_prior_t p;
    p.a_xx = R::coeff(k * (1.0 / (q * sx * sx)), 0.0);
    p.a_yy = R::coeff(k * (1.0 / (q * sy * sy)), 0.0);
    p.a_xy = R::coeff(k * (-rho / (q * sx * sy)), -32767.0);
    p.a_tt = R::coeff(k * (1.0 / (st * st)), 0.0);
    if (static_cast<int64_t>(p.a_xy) * p.a_xy > static_cast<int64_t>(p.a_xx) * p.a_yy) {
        int64_t r = 0;
        while ((r + 1) * (r + 1) <= static_cast<int64_t>(p.a_xx) * p.a_yy) ++r;       // at most 32767 steps, off any hot path
        p.a_xy = static_cast<int32_t>(p.a_xy < 0 ? -r : r);
    }
    p.half_life = 0; p.want_moments = 0;
    return p;
}

template <class Pose, class Lidar>
class ScanMatcherT {
public:
    ScanMatcherT() : h_(nullptr) { check(bl_scanmatch_create(default_ctx(), &h_), "bl_scanmatch_create"); }
    ~ScanMatcherT() { bl_scanmatch_destroy(h_); }
    ScanMatcherT(const ScanMatcherT&) = delete;
    ScanMatcherT& operator=(const ScanMatcherT&) = delete;

    // The best candidate of the window around `centre`; result.pose is the corrected pose (the centre when not accepted).
    bl_scan_match_result_t match(const Lidar& scan, const Pose& centre, const OccupancyGrid& map, const bl_scan_match_params_t& params)
    {
        bl_lidar_t v = lidar_view(scan);
        bl_pose_xyt_t c = pose_in(centre);
        bl_scan_match_result_t r;
        kept_ = false;
        check(bl_scanmatch_match(h_, map.device(), &v, &c, &params, &r), "bl_scanmatch_match");
        kept_ = params.keep_volume != 0;
        keptParams_ = params;
        return r;
    }
    // The match under a motion prior (bl_scanmatch_match_prior): the best objective score - pen of the window; result.score is the
    // winner's raw score.  With prior.want_moments != 0 `moments` (not null then) receives the weighted sums of the window, the best
    // objective and the winner's sub-cell fractions -- bl_scanmatch_covariance and bl_scanmatch_refined_pose read them -- and
    // volume() returns the objective volume, as it does with params.keep_volume.
    bl_scan_match_result_t matchWithPrior(const Lidar& scan, const Pose& centre, const OccupancyGrid& map, const bl_scan_match_params_t& params,
                                          const bl_scan_match_prior_t& prior, bl_scan_match_moments_t* moments = nullptr)
    {
        bl_lidar_t v = lidar_view(scan);
        bl_pose_xyt_t c = pose_in(centre);
        bl_scan_match_result_t r;
        kept_ = false;
        check(bl_scanmatch_match_prior(h_, map.device(), &v, &c, &params, &prior, &r, moments), "bl_scanmatch_match_prior");
        kept_ = params.keep_volume != 0 || prior.want_moments != 0;
        keptParams_ = params;
        return r;
    }
    // The same over windows up to the whole map (bl_scanmatch_match_wide): exact, by scoring coarse blocks first.  It leaves a kept
    // volume of match() as it is.
    bl_scan_match_result_t matchWide(const Lidar& scan, const Pose& centre, const OccupancyGrid& map, const bl_scan_match_wide_params_t& params)
    {
        bl_lidar_t v = lidar_view(scan);
        bl_pose_xyt_t c = pose_in(centre);
        bl_scan_match_result_t r;
        check(bl_scanmatch_match_wide(h_, map.device(), &v, &c, &params, &r), "bl_scanmatch_match_wide");
        return r;
    }
    // what the last matchWide pruned
    bl_scan_match_wide_stats_t wideStats() const
    {
        bl_scan_match_wide_stats_t s;
        check(bl_scanmatch_wide_stats(h_, &s), "bl_scanmatch_wide_stats");
        return s;
    }
    // scores [2 ntheta + 1][2 ny + 1][2 nx + 1] of the last match, sized by the window of that match; empty if it did not keep them
    std::vector<int32_t> volume()
    {
        if (!kept_) return std::vector<int32_t>();
        std::vector<int32_t> out(static_cast<std::size_t>(2 * keptParams_.ntheta + 1) * (2 * keptParams_.ny + 1) * (2 * keptParams_.nx + 1));
        check(bl_scanmatch_volume(h_, out.data()), "bl_scanmatch_volume");
        return out;
    }
    bl_scanmatch* device() const { return h_; }
private:
    bl_scanmatch* h_;
    bool kept_ = false;                    // the last match kept its volume, for the window keptParams_
    bl_scan_match_params_t keptParams_ = bl_scan_match_params_t();
};

}  // namespace botlab_hip

#endif  // BOTLAB_SCAN_MATCHER_HPP
