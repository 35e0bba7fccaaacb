// range_table.hpp -- the range table over the C ABI (bl_rangetable_*, include/botlab_hip.h, "range table"): the beam model's expected
// range of every (cell, heading) of a map that does not change, built once on the device.  BeamModelT::scoresTable / reweighTable
// (beam_model.hpp) and ParticleFilterT::reweighBeamTable (botlab_dropin.hpp) read it in place of the cast;
// OccupancyGridSLAMT::setBeamRangeTable (slam_driver.hpp) does that while the driver leaves its map alone.
//
// The table is never checked against the live map: after cells changed, update(map, x0, y0, x1, y1) over their box (inclusive), or
// build again.  C++11.
#ifndef BOTLAB_RANGE_TABLE_HPP
#define BOTLAB_RANGE_TABLE_HPP

#include <cstdint>
#include <vector>

#include "beam_model.hpp"

namespace botlab_hip {

template <class Pose, class Lidar>
class RangeTableT {
public:
    // headings: a power of two in 64 .. 1024
    explicit RangeTableT(int headings = 256) : h_(nullptr) { check(bl_rangetable_create(default_ctx(), headings, &h_), "bl_rangetable_create"); }
    ~RangeTableT() { bl_rangetable_destroy(h_); }
    RangeTableT(const RangeTableT&) = delete;
    RangeTableT& operator=(const RangeTableT&) = delete;

    // reach and occ_min from the beam model's parameters, the rest from the map
    void build(const BeamModelT<Pose, Lidar>& beam, const OccupancyGrid& map) { check(bl_rangetable_build(h_, beam.device(), map.device()), "bl_rangetable_build"); }
    void update(const OccupancyGrid& map, int x0, int y0, int x1, int y1)
    {
        check(bl_rangetable_update(h_, map.device(), x0, y0, x1, y1), "bl_rangetable_update");
    }
    bl_rangetable_info_t info() const
    {
        bl_rangetable_info_t i;
        check(bl_rangetable_info(h_, &i), "bl_rangetable_info");
        return i;
    }
    // the entries of the cells x0 .. x0 + w - 1, y0 .. y0 + h - 1: [h][w][headings]
    std::vector<uint16_t> read(int x0, int y0, int w, int h) const
    {
        std::vector<uint16_t> out(static_cast<std::size_t>(w > 0 ? w : 1) * static_cast<std::size_t>(h > 0 ? h : 1) * static_cast<std::size_t>(info().headings));
        check(bl_rangetable_read(h_, x0, y0, w, h, out.data()), "bl_rangetable_read");
        return out;
    }
    // x, y per heading
    std::vector<int32_t> directions() const
    {
        std::vector<int32_t> out(2 * static_cast<std::size_t>(info().headings));
        check(bl_rangetable_directions(h_, out.data()), "bl_rangetable_directions");
        return out;
    }
    float lastDeviceMs() const
    {
        float ms = 0.0f;
        check(bl_rangetable_last_device_ms(h_, &ms), "bl_rangetable_last_device_ms");
        return ms;
    }
    bl_rangetable* device() const { return h_; }

private:
    bl_rangetable* h_;
};

}  // namespace botlab_hip

#endif  // BOTLAB_RANGE_TABLE_HPP
