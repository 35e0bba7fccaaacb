// obstacle_layer.hpp -- the obstacle layer over the C ABI (bl_obslayer_*, include/botlab_hip.h, "obstacle layer"): what the scan
// sees and the map does not.  update(map, scan, pose) casts the scan against the static map and keeps a per-cell hit / clear /
// expire state; compose(map, out) writes the map with 127 where the layer is live into another OccupancyGrid, which
// ObstacleDistanceGrid::setDistances (and so every planner) takes where the map went.  MotionPlannerT::setMapWithObstacles
// (planning_dropin.hpp) does both steps behind setMap.
//
// What the layer is not: a tracker.  Rays at or beyond max_range neither hit nor clear, so an obstacle that left with nothing behind
// it goes by expiry (ttl_scans).  C++11.
#ifndef BOTLAB_OBSTACLE_LAYER_HPP
#define BOTLAB_OBSTACLE_LAYER_HPP

#include <cstdint>
#include <vector>

#include "botlab_dropin.hpp"

namespace botlab_hip {

// 5 m of range, every cell with positive log-odds occupied, a return within a cell of the map is the map's, a hit lives 50 scans,
// and one hit makes a cell live
inline bl_obslayer_params_t default_obslayer_params()
{
    bl_obslayer_params_t p;
    p.max_range = 5.0f; p.occ_min = 1; p.tol_cells = 1; p.ttl_scans = 50; p.min_hits = 1;
    return p;
}

template <class Pose, class Lidar>
class ObstacleLayerT {
public:
    ObstacleLayerT(int widthInCells, int heightInCells, const bl_obslayer_params_t& params = default_obslayer_params())
        : h_(nullptr), width_(widthInCells), height_(heightInCells)
    {
        check(bl_obslayer_create(default_ctx(), widthInCells, heightInCells, &h_), "bl_obslayer_create");
        const int rc = bl_obslayer_set_params(h_, &params);
        if (rc != BL_OK) { bl_obslayer_destroy(h_); h_ = nullptr; check(rc, "bl_obslayer_set_params"); }
    }
    ~ObstacleLayerT() { bl_obslayer_destroy(h_); }
    ObstacleLayerT(const ObstacleLayerT&) = delete;
    ObstacleLayerT& operator=(const ObstacleLayerT&) = delete;

    // false (and the layer keeps the parameters it had) when the library refuses them
    bool setParams(const bl_obslayer_params_t& params) { return bl_obslayer_set_params(h_, &params) == BL_OK; }

    // One update from `scan`, taken at `pose`, against the static map: enqueued on the stream every class of this thread uses
    void update(const OccupancyGrid& map, const Lidar& scan, const Pose& pose)
    {
        bl_lidar_t v = lidar_view(scan);
        bl_pose_xyt_t p = pose_in(pose);
        check(bl_obslayer_update(h_, map.device(), &v, &p), "bl_obslayer_update");
    }
    // `out` = the map with 127 where the layer is live.  `out` is made a copy of the map first when its shape or frame differs;
    // it must not be the map itself.
    void compose(const OccupancyGrid& map, OccupancyGrid& out)
    {
        if (out.widthInCells() != map.widthInCells() || out.heightInCells() != map.heightInCells() || out.metersPerCell() != map.metersPerCell() ||
            out.cellsPerMeter() != map.cellsPerMeter() || out.originInGlobalFrame().x != map.originInGlobalFrame().x ||
            out.originInGlobalFrame().y != map.originInGlobalFrame().y)
            out = map;
        check(bl_obslayer_compose(h_, map.device(), out.device()), "bl_obslayer_compose");
        out.markDeviceWritten();
    }
    void reset() { check(bl_obslayer_reset(h_), "bl_obslayer_reset"); }

    // the class (BL_OBS_*) of every ray of the last update's scan, in scan order
    std::vector<uint8_t> classes()
    {
        int n = 0;
        check(bl_obslayer_classes(h_, nullptr, &n), "bl_obslayer_classes");
        std::vector<uint8_t> c(static_cast<std::size_t>(n > 0 ? n : 1));
        check(bl_obslayer_classes(h_, c.data(), &n), "bl_obslayer_classes");
        c.resize(static_cast<std::size_t>(n));
        return c;
    }
    bl_obslayer_stats_t stats()
    {
        bl_obslayer_stats_t s;
        check(bl_obslayer_stats(h_, &s), "bl_obslayer_stats");
        return s;
    }
    // x, y of the live cells, row-major
    std::vector<int32_t> liveCells()
    {
        int n = 0;
        check(bl_obslayer_live_cells(h_, nullptr, 0, &n), "bl_obslayer_live_cells");
        std::vector<int32_t> xy(2 * static_cast<std::size_t>(n > 0 ? n : 1));
        check(bl_obslayer_live_cells(h_, xy.data(), n, &n), "bl_obslayer_live_cells");
        xy.resize(2 * static_cast<std::size_t>(n));
        return xy;
    }
    // the state, row-major (for tests and for saving a layer); upload replaces it
    void download(std::vector<uint8_t>& count, std::vector<uint32_t>& last, uint32_t& n)
    {
        count.resize(static_cast<std::size_t>(width_) * height_);
        last.resize(count.size());
        check(bl_obslayer_download(h_, count.data(), last.data(), &n), "bl_obslayer_download");
    }
    void upload(const std::vector<uint8_t>& count, const std::vector<uint32_t>& last, uint32_t n)
    {
        check(bl_obslayer_upload(h_, count.data(), last.data(), n), "bl_obslayer_upload");
    }
    float lastUpdateMs() const                                        // device time of the last update (waits for it)
    {
        float ms = 0.0f;
        check(bl_obslayer_last_device_ms(h_, &ms, nullptr), "bl_obslayer_last_device_ms");
        return ms;
    }
    float lastComposeMs() const
    {
        float ms = 0.0f;
        check(bl_obslayer_last_device_ms(h_, nullptr, &ms), "bl_obslayer_last_device_ms");
        return ms;
    }
    bl_obslayer* device() const { return h_; }

    int widthInCells() const { return width_; }
    int heightInCells() const { return height_; }

private:
    bl_obslayer* h_;
    int width_, height_;
};

}  // namespace botlab_hip

#endif  // BOTLAB_OBSTACLE_LAYER_HPP
