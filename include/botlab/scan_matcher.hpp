// scan_matcher.hpp -- correlative scan matching over the C ABI (bl_scanmatch_*, include/botlab_hip.h): the pose of a scan against
// the map from a bounded window of whole-cell shifts and heading steps around a centre pose, without odometry.  C++11, templated
// on the caller's pose and lidar message types like the other classes of botlab_dropin.hpp.
#ifndef BOTLAB_SCAN_MATCHER_HPP
#define BOTLAB_SCAN_MATCHER_HPP

#include <cmath>
#include <cstddef>
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
