// path_shortcut.hpp -- PathShortcutT: path shortcutting of libbotlab_hip.so (bl_shortcut_*, botlab_hip.h) for C++ hosts: any-angle
// waypoints from the pose-per-cell paths the planners emit -- all-pairs line of sight over the path's cells and the cheapest chain of
// segments over the visibility graph.  No reference counterpart; header-only over the C ABI like the rest of include/botlab/.
// MotionPlannerT::shortcutPath and planPathShortcut (planning_dropin.hpp) are built on it.
#ifndef BOTLAB_PATH_SHORTCUT_HPP
#define BOTLAB_PATH_SHORTCUT_HPP

#include <cstdint>
#include <vector>

#include <botlab/botlab_dropin.hpp>

namespace botlab_hip {

inline bl_shortcut_params_t shortcut_params(double clearance = 0.2, int32_t max_span = 64, int32_t waypoint_cost = 1024)
{
    bl_shortcut_params_t p;
    p.clearance = clearance; p.max_span = max_span; p.waypoint_cost = waypoint_cost;
    return p;
}

template <class Path, class Pose>
class PathShortcutT {
public:
    explicit PathShortcutT(const bl_shortcut_params_t& params = shortcut_params()) : h_(nullptr)
    {
        check(bl_shortcut_create(default_ctx(), &h_), "bl_shortcut_create");
        setParams(params);
    }
    ~PathShortcutT() { if (h_) bl_shortcut_destroy(h_); }
    PathShortcutT(const PathShortcutT&) = delete;
    PathShortcutT& operator=(const PathShortcutT&) = delete;

    void setParams(const bl_shortcut_params_t& params)
    {
        check(bl_shortcut_set_params(h_, &params), "bl_shortcut_set_params");
        params_ = params;
    }
    const bl_shortcut_params_t& params() const { return params_; }

    // the kept poses of `path`: x, y and utime as they were, headings along the segments; cost, if given: the shortened path's and
    // the input path's (1/1024 cell)
    Path shortcut(const Path& path, const ObstacleDistanceGrid& distances, int64_t* cost = nullptr) const
    {
        const int n = static_cast<int>(path.path.size());
        std::vector<bl_pose_xyt_t> in(static_cast<size_t>(n) + 1), out(static_cast<size_t>(n) + 1);
        for (int i = 0; i < n; ++i) in[static_cast<size_t>(i)] = pose_in(path.path[static_cast<size_t>(i)]);
        int len = 0;
        int64_t c[2] = {0, 0};
        check(bl_shortcut_poses(h_, distances.device(), in.data(), n, &n, 1, out.data(), &len, c), "bl_shortcut_poses");
        if (cost) { cost[0] = c[0]; cost[1] = c[1]; }
        Path r;
        r.utime = path.utime;
        for (int i = 0; i < len; ++i) r.path.push_back(pose_out<Pose>(out[static_cast<size_t>(i)]));
        r.path_length = static_cast<int32_t>(r.path.size());
        return r;
    }
    // the kept indices of P paths of cells (x0, y0, x1, y1, ... with offsets[P + 1]) in one launch sequence
    std::vector<std::vector<int32_t> > cells(const std::vector<int32_t>& xy, const std::vector<int32_t>& offsets, const ObstacleDistanceGrid& distances,
                                             std::vector<int64_t>* cost = nullptr) const
    {
        const int P = static_cast<int>(offsets.size()) - 1;
        std::vector<std::vector<int32_t> > out;
        if (P <= 0) return out;
        std::vector<int32_t> keep(xy.size() / 2 + 1), counts(static_cast<size_t>(P));
        std::vector<int64_t> c(static_cast<size_t>(P) * 2);
        check(bl_shortcut_cells(h_, distances.device(), xy.data(), offsets.data(), P, keep.data(), counts.data(), c.data()), "bl_shortcut_cells");
        for (int p = 0; p < P; ++p)
            out.push_back(std::vector<int32_t>(keep.begin() + offsets[static_cast<size_t>(p)], keep.begin() + offsets[static_cast<size_t>(p)] + counts[static_cast<size_t>(p)]));
        if (cost) *cost = c;
        return out;
    }
    bl_shortcut* device() const { return h_; }

private:
    bl_shortcut* h_;
    bl_shortcut_params_t params_;
};

}  // namespace botlab_hip

#endif  // BOTLAB_PATH_SHORTCUT_HPP
