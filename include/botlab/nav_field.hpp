// nav_field.hpp -- NavigationFieldT: the goal-rooted navigation field of libbotlab_hip.so (bl_navfield_*, botlab_hip.h) for C++
// hosts: the exact cost-to-go of every cell of an ObstacleDistanceGrid to a set of goal cells over 8-connected moves, and the
// cheapest paths read off it.  No reference counterpart; header-only over the C ABI like the rest of include/botlab/.
// MotionPlannerT::planPathOptimal and plan_path_to_frontier_by_cost_t (planning_dropin.hpp) are built on it.
#ifndef BOTLAB_NAV_FIELD_HPP
#define BOTLAB_NAV_FIELD_HPP

#include <cstdint>
#include <vector>

#include <botlab/botlab_dropin.hpp>

namespace botlab_hip {

const uint32_t NAV_UNREACHED = 0xFFFFFFFFu;
const int32_t NAV_OBSTACLE_GAIN = 50;

inline bl_navfield_params_t nav_params(const SearchParams& s, int32_t obstacle_gain = NAV_OBSTACLE_GAIN, int32_t reach_cells = 0)
{
    bl_navfield_params_t p;
    p.minDistanceToObstacle = s.minDistanceToObstacle;
    p.maxDistanceWithCost = s.maxDistanceWithCost;
    p.distanceCostExponent = s.distanceCostExponent;
    p.obstacle_gain = obstacle_gain;
    p.reach_cells = reach_cells;
    return p;
}

// n_min: the smallest L1 distance (cells) that is traversable under `s` on this grid -- f[n] > minDistanceToObstacle * 1.000001 with
// the distance grid's table f[n] = f[n - 1] + 0.1f; -1 if none is
inline int nav_min_traversable_cells(const ObstacleDistanceGrid& d, const SearchParams& s)
{
    float f = 0.0f;
    const int n_max = d.widthInCells() + d.heightInCells();
    for (int n = 0; n <= n_max; ++n) {
        if (f > s.minDistanceToObstacle * 1.000001) return n;
        f = f + 0.1f;
    }
    return -1;
}

template <class Pose, class Path>
class NavigationFieldT {
public:
    struct Result {
        Path path;               // path_length == 1: no path
        int32_t goal;            // index of the listed goal cell the path reached, -1 if none
        uint32_t cost;           // field(start)
    };

    NavigationFieldT() : h_(nullptr) { check(bl_navfield_create(default_ctx(), &h_), "bl_navfield_create"); }
    ~NavigationFieldT() { if (h_) bl_navfield_destroy(h_); }
    NavigationFieldT(const NavigationFieldT&) = delete;
    NavigationFieldT& operator=(const NavigationFieldT&) = delete;

    // goal_xy_cells: x0, y0, x1, y1, ...  `distances` must outlive the queries and stay as it is while paths are asked for
    void compute(const ObstacleDistanceGrid& distances, const bl_navfield_params_t& params, const std::vector<int32_t>& goal_xy_cells)
    {
        check(bl_navfield_compute(h_, distances.device(), &params, goal_xy_cells.empty() ? nullptr : goal_xy_cells.data(),
                                  static_cast<int>(goal_xy_cells.size() / 2)), "bl_navfield_compute");
    }
    void computeToPose(const ObstacleDistanceGrid& distances, const bl_navfield_params_t& params, const Pose& goal)
    {
        bl_pose_xyt_t g = pose_in(goal);
        check(bl_navfield_compute_to_pose(h_, distances.device(), &params, &g), "bl_navfield_compute_to_pose");
    }

    std::vector<Result> paths(const std::vector<Pose>& starts, int cap_each = 4096) const
    {
        const int n = static_cast<int>(starts.size());
        std::vector<Result> out(static_cast<size_t>(n));
        if (n == 0) return out;
        std::vector<bl_pose_xyt_t> s(static_cast<size_t>(n));
        for (int i = 0; i < n; ++i) s[static_cast<size_t>(i)] = pose_in(starts[static_cast<size_t>(i)]);
        std::vector<int> lens(static_cast<size_t>(n));
        std::vector<int32_t> goal(static_cast<size_t>(n));
        std::vector<uint32_t> cost(static_cast<size_t>(n));
        std::vector<bl_pose_xyt_t> buf;
        for (;;) {
            buf.resize(static_cast<size_t>(n) * cap_each);
            check(bl_navfield_paths(h_, s.data(), n, buf.data(), cap_each, lens.data(), goal.data(), cost.data()), "bl_navfield_paths");
            int longest = 0;
            for (int i = 0; i < n; ++i) if (lens[static_cast<size_t>(i)] > longest) longest = lens[static_cast<size_t>(i)];
            if (longest <= cap_each) break;
            cap_each = longest;                                                    // a path was cut off: once more with room for it
        }
        for (int i = 0; i < n; ++i) {
            Result& r = out[static_cast<size_t>(i)];
            r.goal = goal[static_cast<size_t>(i)];
            r.cost = cost[static_cast<size_t>(i)];
            r.path.utime = starts[static_cast<size_t>(i)].utime;
            for (int k = 0; k < lens[static_cast<size_t>(i)]; ++k) r.path.path.push_back(pose_out<Pose>(buf[static_cast<size_t>(i) * cap_each + k]));
            r.path.path_length = static_cast<int32_t>(r.path.path.size());
        }
        return out;
    }
    Result path(const Pose& start, int cap = 4096) const { return paths(std::vector<Pose>(1, start), cap)[0]; }

    std::vector<uint32_t> gather(const std::vector<int32_t>& xy_cells) const
    {
        std::vector<uint32_t> out(xy_cells.size() / 2);
        if (!out.empty()) check(bl_navfield_gather(h_, xy_cells.data(), static_cast<int>(out.size()), out.data()), "bl_navfield_gather");
        return out;
    }
    std::vector<uint32_t> cells() const
    {
        int w = 0, h = 0;
        check(bl_navfield_shape(h_, &w, &h), "bl_navfield_shape");
        std::vector<uint32_t> out(static_cast<size_t>(w) * h);
        check(bl_navfield_download(h_, out.data()), "bl_navfield_download");
        return out;
    }
    int widthInCells() const { int w = 0, h = 0; check(bl_navfield_shape(h_, &w, &h), "bl_navfield_shape"); return w; }
    int heightInCells() const { int w = 0, h = 0; check(bl_navfield_shape(h_, &w, &h), "bl_navfield_shape"); return h; }
    void tables(std::vector<uint8_t>& traversable, std::vector<int32_t>& penalty) const
    {
        int n = 0;
        check(bl_navfield_tables(h_, nullptr, nullptr, &n), "bl_navfield_tables");
        traversable.resize(static_cast<size_t>(n)); penalty.resize(static_cast<size_t>(n));
        check(bl_navfield_tables(h_, traversable.data(), penalty.data(), &n), "bl_navfield_tables");
    }
    // rounds, tile sweeps, traversable cells, reached cells, goal-set cells of the last compute
    std::vector<int64_t> stats() const
    {
        std::vector<int64_t> v(5);
        check(bl_navfield_stats(h_, v.data()), "bl_navfield_stats");
        return v;
    }
    bl_navfield* device() const { return h_; }

private:
    bl_navfield* h_;
};

}  // namespace botlab_hip

#endif  // BOTLAB_NAV_FIELD_HPP
