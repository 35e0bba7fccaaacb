// beam_model.hpp -- the ray-cast (beam) sensor model over the C ABI (bl_beam_*, include/botlab_hip.h, "beam model"): every used ray of
// a scan cast against the map as far as max_range and the measured range scored against the expected one, for many poses at once.
// scores(map, scan, poses) for poses of the caller's; ParticleFilterT::reweighBeam(beam, map, scan) (botlab_dropin.hpp) replaces a
// filter's weight units in place and returns the beam-weighted posterior pose; OccupancyGridSLAMT::setBeamModel (slam_driver.hpp) does
// that behind every localisation update.
//
// Every parameter is an untuned knob.  span (Q16 nats) is the score gap at which a particle reaches the floor.  C++11.
#ifndef BOTLAB_BEAM_MODEL_HPP
#define BOTLAB_BEAM_MODEL_HPP

#include <cstdint>
#include <vector>

#include "botlab_dropin.hpp"

namespace botlab_hip {

// 5 m of range, every cell with positive log-odds occupied, a hit term one cell wide cut at 16 cells, the usual mixture, a max reading
// through a mapped wall a tenth as likely as a free one, the floor 64 nats below the best particle, every ray
inline bl_beam_params_t default_beam_params()
{
    bl_beam_params_t p;
    p.max_range = 5.0f; p.sigma_cells = 1.0f; p.z_hit = 0.7f; p.z_short = 0.1f; p.z_max = 0.05f; p.z_rand = 0.15f; p.lambda = 0.1f;
    p.blocked_factor = 0.1f; p.occ_min = 1; p.hit_cut = 64; p.ray_stride = 1; p.pad = 0; p.span = static_cast<int64_t>(1) << 22;
    return p;
}

struct BeamTables {
    std::vector<uint32_t> hit, short_, lt;                            // 1024, 1024, 256
    uint32_t rand, max_free, max_blocked, ln2, reach;
};

struct BeamCast { std::vector<int32_t> first, K, z, zstar; std::vector<uint32_t> p; };

template <class Pose, class Lidar>
class BeamModelT {
public:
    explicit BeamModelT(const bl_beam_params_t& params = default_beam_params()) : h_(nullptr)
    {
        check(bl_beam_create(default_ctx(), &h_), "bl_beam_create");
        const int rc = bl_beam_set_params(h_, &params);
        if (rc != BL_OK) { bl_beam_destroy(h_); h_ = nullptr; check(rc, "bl_beam_set_params"); }
    }
    ~BeamModelT() { bl_beam_destroy(h_); }
    BeamModelT(const BeamModelT&) = delete;
    BeamModelT& operator=(const BeamModelT&) = delete;

    // false (and the model keeps the parameters it had) when the library refuses them
    bool setParams(const bl_beam_params_t& params) { return bl_beam_set_params(h_, &params) == BL_OK; }

    // S of every pose (BL_BEAM_OFF_GRID for one that takes no part)
    std::vector<int64_t> scores(const OccupancyGrid& map, const Lidar& scan, const std::vector<Pose>& poses)
    {
        return scoresBy(bl_beam_scores, map.device(), "bl_beam_scores", scan, poses);
    }
    // the units of the last scores() or reweighBeam(); n: that call's count
    std::vector<uint32_t> units(int n)
    {
        std::vector<uint32_t> out(static_cast<std::size_t>(n > 0 ? n : 1));
        check(bl_beam_units(h_, out.data(), n), "bl_beam_units");
        out.resize(static_cast<std::size_t>(n > 0 ? n : 0));
        return out;
    }
    // the per-ray values of one pose's used rays
    BeamCast debugCast(const OccupancyGrid& map, const Lidar& scan, const Pose& pose)
    {
        BeamCast c;
        debugPlanes(bl_beam_debug_cast, map.device(), "bl_beam_debug_cast", scan, pose, c.first, c.K, c.z, c.zstar, c.p);
        return c;
    }
    // scores() with the expected ranges looked up in a built range table (RangeTableT, range_table.hpp) instead of cast against the
    // map.  The table is not checked against the live map.
    template <class Table>
    std::vector<int64_t> scoresTable(const Table& table, const Lidar& scan, const std::vector<Pose>& poses)
    {
        return scoresBy(bl_rangetable_scores, table.device(), "bl_rangetable_scores", scan, poses);
    }
    // a filter's weight units replaced in place by the scoring by table (Filter: ParticleFilterT); the beam-weighted posterior pose
    template <class Filter, class Table>
    Pose reweighTable(Filter& pf, const Table& table, const Lidar& scan)
    {
        bl_lidar_t v = lidar_view(scan);
        bl_pose_xyt_t out;
        check(bl_rangetable_reweigh_pf(h_, pf.device(), table.device(), &v, &out), "bl_rangetable_reweigh_pf");
        return pose_out<Pose>(out);
    }
    // the per-ray values of one pose's used rays by table (first and K stay empty; h: the heading looked up)
    template <class Table>
    BeamCast debugLookup(const Table& table, const Lidar& scan, const Pose& pose, std::vector<int32_t>* h)
    {
        BeamCast c;
        debugPlanes(bl_rangetable_debug_lookup, table.device(), "bl_rangetable_debug_lookup", scan, pose, *h, c.z, c.zstar, c.p);
        return c;
    }
    // scores() with the expected ranges found by leaps over a built clearance grid (ClearanceGridT, clearance_grid.hpp): value for
    // value the cast's on the map the grid was built on.  The grid is not checked against the live map.
    template <class Clearance>
    std::vector<int64_t> scoresLeap(const Clearance& clearance, const Lidar& scan, const std::vector<Pose>& poses)
    {
        return scoresBy(bl_clearance_scores, clearance.device(), "bl_clearance_scores", scan, poses);
    }
    // a filter's weight units replaced in place by the scoring by leaps (Filter: ParticleFilterT); the beam-weighted posterior pose
    template <class Filter, class Clearance>
    Pose reweighLeap(Filter& pf, const Clearance& clearance, const Lidar& scan)
    {
        bl_lidar_t v = lidar_view(scan);
        bl_pose_xyt_t out;
        check(bl_clearance_reweigh_pf(h_, pf.device(), clearance.device(), &v, &out), "bl_clearance_reweigh_pf");
        return pose_out<Pose>(out);
    }
    // debugCast's columns by leaps; rounds: the entries of the clearance grid each ray read (-1 for a dropped ray)
    template <class Clearance>
    BeamCast debugLeap(const Clearance& clearance, const Lidar& scan, const Pose& pose, std::vector<int32_t>* rounds)
    {
        BeamCast c;
        debugPlanes(bl_clearance_debug_cast, clearance.device(), "bl_clearance_debug_cast", scan, pose, c.first, c.K, c.z, c.zstar, c.p, *rounds);
        return c;
    }
    BeamTables tables(float cellsPerMeter) const
    {
        BeamTables t;
        t.hit.resize(1024); t.short_.resize(1024); t.lt.resize(256);
        uint32_t s[5];
        check(bl_beam_tables(h_, cellsPerMeter, t.hit.data(), t.short_.data(), t.lt.data(), s), "bl_beam_tables");
        t.rand = s[0]; t.max_free = s[1]; t.max_blocked = s[2]; t.ln2 = s[3]; t.reach = s[4];
        return t;
    }
    static std::vector<uint32_t> unitTable()
    {
        std::vector<uint32_t> u(257);
        bl_beam_unit_table(u.data());
        return u;
    }
    int debugPath() const { return bl_beam_debug_path(h_); }           // 0 staged, 1 direct, 2 both, -1 none yet
    float lastDeviceMs() const
    {
        float ms = 0.0f;
        check(bl_beam_last_device_ms(h_, &ms), "bl_beam_last_device_ms");
        return ms;
    }
    bl_beam* device() const { return h_; }

private:
    // poses in, scores out through fn (bl_beam_scores or bl_rangetable_scores) on its map or table
    template <class Fn, class Source>
    std::vector<int64_t> scoresBy(Fn fn, const Source* source, const char* what, const Lidar& scan, const std::vector<Pose>& poses)
    {
        bl_lidar_t v = lidar_view(scan);
        std::vector<bl_pose_xyt_t> in(poses.size() ? poses.size() : 1);
        for (std::size_t i = 0; i < poses.size(); ++i) in[i] = pose_in(poses[i]);
        std::vector<int64_t> out(in.size());
        check(fn(h_, source, &v, in.data(), static_cast<int>(poses.size()), out.data()), what);
        out.resize(poses.size());
        return out;
    }
    // the debug planes of one pose through fn (bl_beam_debug_cast or bl_rangetable_debug_lookup): sized for the whole scan, filled,
    // cut to the used rays
    template <class Fn, class Source, class... Planes>
    void debugPlanes(Fn fn, const Source* source, const char* what, const Lidar& scan, const Pose& pose, Planes&... planes)
    {
        bl_lidar_t v = lidar_view(scan);
        bl_pose_xyt_t p = pose_in(pose);
        const int sized[] = {(planes.resize(static_cast<std::size_t>(v.num_ranges > 0 ? v.num_ranges : 1)), 0)...};
        check(fn(h_, source, &v, &p, planes.data()...), what);
        const int cut[] = {(planes.resize(static_cast<std::size_t>(bl_beam_last_rays(h_))), 0)...};
        (void)sized; (void)cut;
    }

    bl_beam* h_;
};

}  // namespace botlab_hip

#endif  // BOTLAB_BEAM_MODEL_HPP
