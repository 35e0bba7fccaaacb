// obstacle_tracks.hpp -- the obstacle tracks over the C ABI (bl_obstracks_*, include/botlab_hip.h, "obstacle tracks"): the obstacle
// layer's live cells grouped into blobs, the blobs followed from update to update, and a composed grid that also holds where the
// moving ones are heading.  update() once after each ObstacleLayerT::update; compose(map, out, horizon, ...) where the layer's
// compose went.  MotionPlannerT::setMapWithTracks (planning_dropin.hpp) does the compose behind setMap.
//
// Every parameter is an untuned knob.  C++11.
#ifndef BOTLAB_OBSTACLE_TRACKS_HPP
#define BOTLAB_OBSTACLE_TRACKS_HPP

#include <cstdint>
#include <vector>

#include "obstacle_layer.hpp"

namespace botlab_hip {

// any blob is an object, a gate of four cells, half the residual into the position and a quarter into the velocity, three hits
// confirm, three misses are coasted, and 1/16 cell per update is moving
inline bl_obstracks_params_t default_obstracks_params()
{
    bl_obstracks_params_t p;
    p.min_cells = 1; p.max_cells = BL_OBSTRACKS_MAX_CELLS; p.gate_cells = 4; p.alpha = 128; p.beta = 64; p.confirm_hits = 3; p.max_missed = 3;
    p.min_speed = 16;
    return p;
}

// a track in metres and metres per second, in the frame of `map`, one update taking scanPeriod seconds (double on the host)
struct ObstacleTrackMetric { double x, y, vx, vy; };
inline ObstacleTrackMetric obstacle_track_metric(const bl_obstrack_t& t, const OccupancyGrid& map, double scanPeriod)
{
    const double mpc = map.metersPerCell();
    ObstacleTrackMetric m;
    m.x = map.originInGlobalFrame().x + t.px / 256.0 * mpc; m.y = map.originInGlobalFrame().y + t.py / 256.0 * mpc;
    m.vx = t.vx / 256.0 * mpc / scanPeriod; m.vy = t.vy / 256.0 * mpc / scanPeriod;
    return m;
}

template <class Layer>
class ObstacleTrackerT {
public:
    explicit ObstacleTrackerT(Layer& layer, const bl_obstracks_params_t& params = default_obstracks_params()) : h_(nullptr), layer_(layer)
    {
        check(bl_obstracks_create(default_ctx(), layer.widthInCells(), layer.heightInCells(), &h_), "bl_obstracks_create");
        const int rc = bl_obstracks_set_params(h_, &params);
        if (rc != BL_OK) { bl_obstracks_destroy(h_); h_ = nullptr; check(rc, "bl_obstracks_set_params"); }
    }
    ~ObstacleTrackerT() { bl_obstracks_destroy(h_); }
    ObstacleTrackerT(const ObstacleTrackerT&) = delete;
    ObstacleTrackerT& operator=(const ObstacleTrackerT&) = delete;

    // false (and the tracker keeps the parameters it had) when the library refuses them
    bool setParams(const bl_obstracks_params_t& params) { return bl_obstracks_set_params(h_, &params) == BL_OK; }

    // One update from the layer's state as it stands (enqueued).  The status: BL_ERR_STATE when the order of calls is wrong.
    // Two refusals are found on the device only -- more than BL_OBSTRACKS_MAX_CELLS live cells, a birth that would need id 2^32 - 1 --
    // and give BL_OK: the slots stay as they were, there are no blobs, and stats().refused is BL_OBSTRACKS_REFUSED_*.  A caller
    // that never reads stats() never learns of them.
    int tryUpdate() { return bl_obstracks_update(h_, layer_.device()); }
    void update() { check(tryUpdate(), "bl_obstracks_update"); }
    // `out` = the layer's compose, and 127 also where the confirmed moving tracks' cells will be within `horizon` updates, except
    // within keepClear cells (Chebyshev; -1: nowhere) of the robot's cell.  `out` is made a copy of the map first when its shape or
    // frame differs; it must not be the map itself.
    void compose(const OccupancyGrid& map, OccupancyGrid& out, int horizon, int robotX = 0, int robotY = 0, int keepClear = -1)
    {
        if (out.widthInCells() != map.widthInCells() || out.heightInCells() != map.heightInCells() || out.metersPerCell() != map.metersPerCell() ||
            out.cellsPerMeter() != map.cellsPerMeter() || out.originInGlobalFrame().x != map.originInGlobalFrame().x ||
            out.originInGlobalFrame().y != map.originInGlobalFrame().y)
            out = map;
        bl_obstracks_compose_t c;
        c.horizon = horizon; c.robot_x = robotX; c.robot_y = robotY; c.keep_clear = keepClear;
        check(bl_obstracks_compose(h_, layer_.device(), map.device(), out.device(), &c), "bl_obstracks_compose");
        out.markDeviceWritten();
    }
    // `out` = the layer's compose without the cells of the confirmed moving tracks' blobs, which keep the map's value: the grid for the
    // field under LocalPlannerT::commandMoving (local_planner.hpp), which meets the moving obstacles where they will be.
    void composeStatic(const OccupancyGrid& map, OccupancyGrid& out)
    {
        if (out.widthInCells() != map.widthInCells() || out.heightInCells() != map.heightInCells() || out.metersPerCell() != map.metersPerCell() ||
            out.cellsPerMeter() != map.cellsPerMeter() || out.originInGlobalFrame().x != map.originInGlobalFrame().x ||
            out.originInGlobalFrame().y != map.originInGlobalFrame().y)
            out = map;
        check(bl_obstracks_compose_static(h_, layer_.device(), map.device(), out.device()), "bl_obstracks_compose_static");
        out.markDeviceWritten();
    }
    void reset() { check(bl_obstracks_reset(h_), "bl_obstracks_reset"); }

    std::vector<bl_obstrack_t> tracks()                               // the occupied slots in slot order
    {
        std::vector<bl_obstrack_t> t(BL_OBSTRACKS_MAX_TRACKS);
        int n = 0;
        check(bl_obstracks_tracks(h_, t.data(), BL_OBSTRACKS_MAX_TRACKS, &n), "bl_obstracks_tracks");
        t.resize(static_cast<std::size_t>(n));
        return t;
    }
    std::vector<bl_obsblob_t> blobs()                                 // the kept blobs of the last update in rank order
    {
        std::vector<bl_obsblob_t> b(BL_OBSTRACKS_MAX_BLOBS);
        int n = 0;
        check(bl_obstracks_blobs(h_, b.data(), BL_OBSTRACKS_MAX_BLOBS, &n), "bl_obstracks_blobs");
        b.resize(static_cast<std::size_t>(n));
        return b;
    }
    std::vector<int32_t> labels()                                     // per live cell of the last update: its blob's rank or -1
    {
        int n = 0;
        check(bl_obstracks_labels(h_, nullptr, 0, &n), "bl_obstracks_labels");
        std::vector<int32_t> l(static_cast<std::size_t>(n > 0 ? n : 1));
        check(bl_obstracks_labels(h_, l.data(), n, &n), "bl_obstracks_labels");
        l.resize(static_cast<std::size_t>(n));
        return l;
    }
    bl_obstracks_stats_t stats()
    {
        bl_obstracks_stats_t s;
        check(bl_obstracks_stats(h_, &s), "bl_obstracks_stats");
        return s;
    }
    // the whole state (for tests and for saving a tracker); upload replaces it and is false when the library refuses it
    void download(std::vector<bl_obstrack_t>& slots, bl_obstracks_state_t& state)
    {
        slots.resize(BL_OBSTRACKS_MAX_TRACKS);
        check(bl_obstracks_download(h_, slots.data(), &state), "bl_obstracks_download");
    }
    bool upload(const std::vector<bl_obstrack_t>& slots, const bl_obstracks_state_t& state)
    {
        return slots.size() == BL_OBSTRACKS_MAX_TRACKS && bl_obstracks_upload(h_, slots.data(), &state) == BL_OK;
    }
    float lastUpdateMs() const                                        // device time of the last update (waits for it)
    {
        float ms = 0.0f;
        check(bl_obstracks_last_device_ms(h_, &ms, nullptr), "bl_obstracks_last_device_ms");
        return ms;
    }
    float lastComposeMs() const
    {
        float ms = 0.0f;
        check(bl_obstracks_last_device_ms(h_, nullptr, &ms), "bl_obstracks_last_device_ms");
        return ms;
    }
    bl_obstracks* device() const { return h_; }
    Layer& layer() const { return layer_; }

private:
    bl_obstracks* h_;
    Layer& layer_;
};

}  // namespace botlab_hip

#endif  // BOTLAB_OBSTACLE_TRACKS_HPP
