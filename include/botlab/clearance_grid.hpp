// clearance_grid.hpp -- the clearance grid over the C ABI (bl_clearance_*, include/botlab_hip.h, "clearance grid"): per cell of a map
// the Chebyshev distance to the nearest occupied cell, capped, one byte.  BeamModelT::scoresLeap / reweighLeap / debugLeap
// (beam_model.hpp) and ParticleFilterT::reweighBeamLeap (botlab_dropin.hpp) leap over it where the cast reads every cell of a ray,
// with the cast's results value for value; it is kept current in a box, so it serves a map that changes.
//
// The grid is never checked against the live map: after cells changed, update(map, x0, y0, x1, y1) over their box (inclusive), or
// build again.  The cap is an untuned knob.  C++11.
#ifndef BOTLAB_CLEARANCE_GRID_HPP
#define BOTLAB_CLEARANCE_GRID_HPP

#include <cstdint>
#include <vector>

#include "beam_model.hpp"

namespace botlab_hip {

template <class Pose, class Lidar>
class ClearanceGridT {
public:
    // cap: 1 .. 255, the largest distance an entry holds
    explicit ClearanceGridT(int cap = 64) : h_(nullptr) { check(bl_clearance_create(default_ctx(), cap, &h_), "bl_clearance_create"); }
    ~ClearanceGridT() { bl_clearance_destroy(h_); }
    ClearanceGridT(const ClearanceGridT&) = delete;
    ClearanceGridT& operator=(const ClearanceGridT&) = delete;

    // occ_min: the beam model's, 1 .. 127
    void build(const OccupancyGrid& map, int occ_min = 1) { check(bl_clearance_build(h_, map.device(), occ_min), "bl_clearance_build"); }
    void update(const OccupancyGrid& map, int x0, int y0, int x1, int y1)
    {
        check(bl_clearance_update(h_, map.device(), x0, y0, x1, y1), "bl_clearance_update");
    }
    bl_clearance_info_t info() const
    {
        bl_clearance_info_t i;
        check(bl_clearance_info(h_, &i), "bl_clearance_info");
        return i;
    }
    // the entries of the cells x0 .. x0 + w - 1, y0 .. y0 + h - 1: [h][w]
    std::vector<uint8_t> read(int x0, int y0, int w, int h) const
    {
        std::vector<uint8_t> out(static_cast<std::size_t>(w > 0 ? w : 1) * static_cast<std::size_t>(h > 0 ? h : 1));
        check(bl_clearance_read(h_, x0, y0, w, h, out.data()), "bl_clearance_read");
        return out;
    }
    float lastDeviceMs() const
    {
        float ms = 0.0f;
        check(bl_clearance_last_device_ms(h_, &ms), "bl_clearance_last_device_ms");
        return ms;
    }
    bl_clearance* device() const { return h_; }

private:
    bl_clearance* h_;
};

}  // namespace botlab_hip

#endif  // BOTLAB_CLEARANCE_GRID_HPP
