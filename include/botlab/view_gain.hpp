// view_gain.hpp -- ViewGainT: the view gain of libbotlab_hip.so (bl_viewgain_*, botlab_hip.h) for C++ hosts -- the number of distinct
// unknown cells a fan of rays cast from a candidate cell reaches --, and plan_path_to_frontier_by_gain_t, the frontier planner that
// weighs it against the navigation field's travel cost.  No reference counterpart; header-only over the C ABI like the rest of
// include/botlab/.  planning_dropin.hpp includes this header.
#ifndef BOTLAB_VIEW_GAIN_HPP
#define BOTLAB_VIEW_GAIN_HPP

#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include <botlab/planning_dropin.hpp>

namespace botlab_hip {

inline bl_viewgain_params_t view_gain_params(int32_t radius_cells = 60, int32_t n_rays = 360, int32_t occupied_above = 0, int32_t unknown_lo = 0,
                                             int32_t unknown_hi = 0)
{
    bl_viewgain_params_t p;
    p.radius_cells = radius_cells; p.n_rays = n_rays;
    p.occupied_above = occupied_above; p.unknown_lo = unknown_lo; p.unknown_hi = unknown_hi;
    return p;
}

class ViewGainT {
public:
    explicit ViewGainT(const bl_viewgain_params_t& params = view_gain_params()) : h_(nullptr)
    {
        check(bl_viewgain_create(default_ctx(), &h_), "bl_viewgain_create");
        setParams(params);
    }
    ~ViewGainT() { if (h_) bl_viewgain_destroy(h_); }
    ViewGainT(const ViewGainT&) = delete;
    ViewGainT& operator=(const ViewGainT&) = delete;

    void setParams(const bl_viewgain_params_t& params)
    {
        check(bl_viewgain_set_params(h_, &params), "bl_viewgain_set_params");
        radius_ = params.radius_cells;
    }
    // x0, y0, x1, y1, ...: the end offset of every ray, as the kernel uses it
    std::vector<int32_t> rayEnds() const
    {
        int n = 0;
        check(bl_viewgain_ray_ends(h_, nullptr, &n), "bl_viewgain_ray_ends");
        std::vector<int32_t> xy(static_cast<size_t>(n) * 2);
        check(bl_viewgain_ray_ends(h_, xy.data(), &n), "bl_viewgain_ray_ends");
        return xy;
    }
    // xy_cells: x0, y0, x1, y1, ...
    std::vector<uint32_t> compute(const OccupancyGrid& map, const std::vector<int32_t>& xy_cells) const
    {
        std::vector<uint32_t> out(xy_cells.size() / 2);
        if (!out.empty()) check(bl_viewgain_compute(h_, map.device(), xy_cells.data(), static_cast<int>(out.size()), out.data()), "bl_viewgain_compute");
        return out;
    }
    // the seen set of one candidate: (2R + 1)^2 bytes, 0 / 1, row-major window around the cell
    std::vector<uint8_t> debugSeen(const OccupancyGrid& map, int x, int y) const
    {
        const size_t side = 2 * static_cast<size_t>(radius_) + 1;
        std::vector<uint8_t> out(side * side);
        check(bl_viewgain_debug_seen(h_, map.device(), x, y, out.data()), "bl_viewgain_debug_seen");
        return out;
    }
    int radiusInCells() const { return radius_; }
    bl_viewgain* device() const { return h_; }

private:
    bl_viewgain* h_;
    int radius_;
};

struct FrontierGainOptions {
    int reach_cells;         // < 0: n_min, as plan_path_to_frontier_by_cost_t
    int stride;              // candidates are thinned to x % stride == 0 && y % stride == 0
    uint32_t min_gain;       // candidates that would see fewer cells are dropped
    int64_t gain_weight;     // UNTUNED: 1 prices a newly seen cell at a tenth of a straight step.  A knob for the caller, not a result.
    int32_t obstacle_gain;
    FrontierGainOptions() : reach_cells(-1), stride(1), min_gain(1), gain_weight(1), obstacle_gain(NAV_OBSTACLE_GAIN) {}
};

struct FrontierGainChoice {
    int frontier;            // index of the chosen candidate's frontier, -1: none
    int32_t x, y;            // the chosen cell
    uint32_t gain, cost;
    FrontierGainChoice() : frontier(-1), x(-1), y(-1), gain(0), cost(NAV_UNREACHED) {}
};

// The viewpoint near a frontier that weighs expected new map against travel cost (no reference counterpart).  Candidates: the cells
// within Chebyshev reach_cells of a frontier cell that the robot can reach -- cost(c), the navigation field rooted at the robot's
// cell, is not UNREACHED --, in row-major order, thinned by `stride`; a candidate's frontier is the owner of the lowest-indexed
// frontier cell within reach of it.  gain(c) comes from `view` in one bl_viewgain_compute.  Of the candidates with
// gain >= min_gain the one maximising gain_weight * gain - cost is chosen, ties by lower cost, then lower y, then lower x, and the
// path is the cheapest one to that cell (a second field, rooted there): what planPathOptimal gives.  An empty frontier list gives
// the empty path; no surviving candidate gives the robot's 1-pose path; both leave choice->frontier at -1.
template <class Path, class Pose, class Planner>
Path plan_path_to_frontier_by_gain_t(const std::vector<frontier_t>& frontiers, const Pose& robotPose, const OccupancyGrid& map, const Planner& planner,
                                     const ViewGainT& view, const FrontierGainOptions& opt = FrontierGainOptions(), FrontierGainChoice* choice = nullptr)
{
    FrontierGainChoice none;
    if (choice) *choice = none;
    Path path;
    if (frontiers.empty()) return path;
    path.utime = robotPose.utime;
    path.path.push_back(robotPose);
    path.path_length = 1;
    const ObstacleDistanceGrid& d = planner.distances();
    int reach = opt.reach_cells;
    if (reach < 0) {
        reach = nav_min_traversable_cells(d, planner.searchParams());
        if (reach < 0) reach = 0;
    }
    const int stride = opt.stride < 1 ? 1 : opt.stride;
    const PointT<float> o = d.originInGlobalFrame();
    const float cpm = d.cellsPerMeter();
    const int w = d.widthInCells(), h = d.heightInCells();
    const double rvx = (static_cast<double>(robotPose.x) - o.x) * cpm, rvy = (static_cast<double>(robotPose.y) - o.y) * cpm;
    if (!(rvx > -1.0 && rvx < w && rvy > -1.0 && rvy < h)) return path;
    // (cell, index of the frontier cell) for every cell within reach of a frontier cell inside the grid
    std::vector<std::pair<int64_t, int32_t> > near;
    std::vector<int32_t> owner;
    for (size_t k = 0; k < frontiers.size(); ++k)
        for (const PointT<float>& c : frontiers[k].cells) {                         // global_position_to_grid_cell (grid_utils.hpp:33-38)
            const int fx = static_cast<int>((static_cast<double>(c.x) - o.x) * cpm), fy = static_cast<int>((static_cast<double>(c.y) - o.y) * cpm);
            const int32_t idx = static_cast<int32_t>(owner.size());
            owner.push_back(static_cast<int32_t>(k));
            if (fx < 0 || fy < 0 || fx >= w || fy >= h) continue;
            for (int y = std::max(fy - reach, 0); y <= std::min(fy + reach, h - 1); ++y)
                for (int x = std::max(fx - reach, 0); x <= std::min(fx + reach, w - 1); ++x)
                    if (x % stride == 0 && y % stride == 0) near.push_back(std::make_pair(static_cast<int64_t>(y) * w + x, idx));
        }
    std::sort(near.begin(), near.end());                                            // row-major; the lowest frontier cell first
    std::vector<int32_t> cand, who;
    for (size_t i = 0; i < near.size(); ++i) {
        if (i > 0 && near[i].first == near[i - 1].first) continue;
        cand.push_back(static_cast<int32_t>(near[i].first % w)); cand.push_back(static_cast<int32_t>(near[i].first / w));
        who.push_back(near[i].second);
    }
    if (who.empty()) return path;
    NavigationFieldT<Pose, Path> field;
    const bl_navfield_params_t np = nav_params(planner.searchParams(), opt.obstacle_gain, 0);
    std::vector<int32_t> root(2);
    root[0] = static_cast<int32_t>(rvx); root[1] = static_cast<int32_t>(rvy);
    field.compute(d, np, root);
    const std::vector<uint32_t> cost_all = field.gather(cand);
    std::vector<int32_t> xy, who2;
    std::vector<uint32_t> cost;
    for (size_t i = 0; i < who.size(); ++i) {
        if (cost_all[i] == NAV_UNREACHED) continue;                                 // UNREACHED also where the cell is not traversable
        xy.push_back(cand[2 * i]); xy.push_back(cand[2 * i + 1]);
        who2.push_back(who[i]); cost.push_back(cost_all[i]);
    }
    const std::vector<uint32_t> gain = view.compute(map, xy);
    int best = -1;
    int64_t best_u = 0;
    for (size_t i = 0; i < gain.size(); ++i) {                                      // row-major order: the first of equals has the lower y, then x
        if (gain[i] < opt.min_gain) continue;
        const int64_t u = opt.gain_weight * static_cast<int64_t>(gain[i]) - static_cast<int64_t>(cost[i]);
        if (best < 0 || u > best_u || (u == best_u && cost[i] < cost[static_cast<size_t>(best)])) { best = static_cast<int>(i); best_u = u; }
    }
    if (best < 0) return path;
    std::vector<int32_t> goal(xy.begin() + 2 * best, xy.begin() + 2 * best + 2);
    field.compute(d, np, goal);
    typename NavigationFieldT<Pose, Path>::Result r = field.path(robotPose, 65536);
    if (choice) {
        choice->frontier = owner[static_cast<size_t>(who2[static_cast<size_t>(best)])];
        choice->x = goal[0]; choice->y = goal[1];
        choice->gain = gain[static_cast<size_t>(best)]; choice->cost = cost[static_cast<size_t>(best)];
    }
    return r.path;
}

}  // namespace botlab_hip

#endif  // BOTLAB_VIEW_GAIN_HPP
