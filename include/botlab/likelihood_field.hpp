// likelihood_field.hpp -- the likelihood field over the C ABI (bl_lfield_*, include/botlab_hip.h, "likelihood field"): a smoothed
// map for whatever scores ray end points.  Every cell holds peak * exp(-d^2 / (2 sigma^2)) of its distance d to the nearest cell
// with log-odds >= occ_min, cut off beyond max_cells cells.  compute(map) returns an OccupancyGrid that
// ParticleFilterT::updateFilter / updateFilterBegin and ScanMatcherT::match / matchWithPrior / matchWide take where the map went.
//
// What the field is not: a map.  It has no free / unknown distinction and no negative cell, so initializeFilterUniformly,
// enableRecovery, MappingT, the frontiers, the view gain and the distance grids keep taking the real grid.  Nothing enforces this.
// C++11.
#ifndef BOTLAB_LIKELIHOOD_FIELD_HPP
#define BOTLAB_LIKELIHOOD_FIELD_HPP

#include <cstdint>
#include <memory>
#include <vector>

#include "botlab_dropin.hpp"

namespace botlab_hip {

// sigma 0.10 m, cut off at 6 cells (3 sigma at 5 cm cells), every cell with positive log-odds a source, the int8 range as the peak
inline bl_lfield_params_t default_lfield_params()
{
    bl_lfield_params_t p;
    p.sigma = 0.1f; p.max_cells = 6; p.occ_min = 1; p.peak = 127;
    return p;
}

class LikelihoodFieldT {
public:
    explicit LikelihoodFieldT(const bl_lfield_params_t& params = default_lfield_params()) : h_(nullptr), raw_(nullptr)
    {
        check(bl_lfield_create(default_ctx(), &h_), "bl_lfield_create");
        check(bl_lfield_set_params(h_, &params), "bl_lfield_set_params");
    }
    ~LikelihoodFieldT() { view_.reset(); bl_lfield_destroy(h_); }
    LikelihoodFieldT(const LikelihoodFieldT&) = delete;
    LikelihoodFieldT& operator=(const LikelihoodFieldT&) = delete;

    // false (and the field keeps the parameters it had) when the library refuses them
    bool setParams(const bl_lfield_params_t& params) { return bl_lfield_set_params(h_, &params) == BL_OK; }

    // The field of `map` as it stands: enqueued on the stream every class of this thread uses, nothing waits.  The grid returned is
    // a view of the field's own (it has the map's shape and frame); it stays the same object while the map's shape stays the same
    // and dies with this field.
    const OccupancyGrid& compute(const OccupancyGrid& map)
    {
        check(bl_lfield_compute(h_, map.device()), "bl_lfield_compute");
        const bl_grid* g = bl_lfield_grid(h_);
        if (!view_ || g != raw_ || view_->widthInCells() != map.widthInCells() || view_->heightInCells() != map.heightInCells() ||
            view_->metersPerCell() != map.metersPerCell() || view_->cellsPerMeter() != map.cellsPerMeter() ||
            view_->originInGlobalFrame().x != map.originInGlobalFrame().x || view_->originInGlobalFrame().y != map.originInGlobalFrame().y) {
            view_.reset(new OccupancyGrid(OccupancyGrid::View(), g, map));
            raw_ = g;
        }
        view_->markDeviceWritten();
        return *view_;
    }
    bool computed() const { return static_cast<bool>(view_); }
    const OccupancyGrid& grid() const { return *view_; }              // of the last compute (computed() first)

    // T[0 .. max_cells^2 + 1] of the last compute: the field's value by squared distance in cells; the last entry (FAR) is 0
    std::vector<int8_t> table() const
    {
        int n = 0;
        std::vector<int8_t> t(static_cast<std::size_t>(BL_LFIELD_MAX_CELLS) * BL_LFIELD_MAX_CELLS + 2);
        check(bl_lfield_table(h_, t.data(), &n), "bl_lfield_table");
        t.resize(static_cast<std::size_t>(n));
        return t;
    }
    float lastDeviceMs() const                                        // device time of the last compute (waits for it)
    {
        float ms = 0.0f;
        check(bl_lfield_last_device_ms(h_, &ms), "bl_lfield_last_device_ms");
        return ms;
    }
    bl_lfield* device() const { return h_; }

private:
    bl_lfield* h_;
    const bl_grid* raw_;
    std::unique_ptr<OccupancyGrid> view_;
};

}  // namespace botlab_hip

#endif  // BOTLAB_LIKELIHOOD_FIELD_HPP
