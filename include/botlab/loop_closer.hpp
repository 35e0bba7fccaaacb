// loop_closer.hpp -- the loop-closure front end over the C ABI (bl_loopclose_*, include/botlab_hip.h, "loop closure"):
// find() makes the loop edges of a ScanHistoryT (map_rebuild.hpp) -- every candidate pair, submap, match and edge in one sequence of
// launches -- and close() gates them through a PoseGraphT (pose_graph.hpp) and writes the corrected poses back into the history.
// OccupancyGridSLAMT::closeLoops (slam_driver.hpp) is find, close and rebuildMap on the driver's history.
// findPlaces() is find() with the partner chosen by the scans' descriptors instead of the recorded poses ("loop closure by place
// recognition"), for a drift larger than the radius; closeLoopsByPlace is the driver's call with it.
//
// Every rule is the C header's.  C++11.
#ifndef BOTLAB_LOOP_CLOSER_HPP
#define BOTLAB_LOOP_CLOSER_HPP

#include <cstdint>
#include <vector>

#include "botlab_dropin.hpp"
#include "map_rebuild.hpp"
#include "pose_graph.hpp"

namespace botlab_hip {

// botlab_amd.find_loop_closures' defaults; every one is an untuned knob
inline bl_loopclose_params_t loopCloseParams()
{
    bl_loopclose_params_t p;
    p.stride = 4; p.min_gap = 40; p.radius = 1.0f; p.w = 5; p.submap_cells = 200;
    p.max_laser = 5.0f; p.hit = 3; p.miss = 1;
    p.match.nx = 8; p.match.ny = 8; p.match.ntheta = 12; p.match.dtheta = 0.00872664625997164788f; p.match.max_range = 8.0f;
    p.match.min_score = 0; p.match.keep_volume = 0;
    p.prior.a_xx = 0; p.prior.a_xy = 0; p.prior.a_yy = 0; p.prior.a_tt = 0; p.prior.half_life = 64; p.prior.want_moments = 1;
    return p;
}

// botlab_amd.LoopCloser.find_places' defaults; bins_per_meter, dilate, min_key and min_bits are untuned knobs
inline bl_place_params_t placeParams()
{
    bl_place_params_t p;
    p.bins_per_meter = 4.0f; p.max_range = 8.0f; p.dilate = 1; p.min_key = 16384; p.min_bits = 8;
    return p;
}

// what close() leaves behind
struct LoopCloseOutcome {
    std::vector<bl_posegraph_edge_t> kept;      // the candidates that passed both gates, in their order
    std::vector<double> alone;                  // per candidate: the cost of the graph with that candidate alone
    bl_posegraph_result_t result;               // of the last solve
    LoopCloseOutcome() : result(bl_posegraph_result_t()) {}
};

template <class Pose, class Lidar>
class LoopCloserT {
public:
    explicit LoopCloserT(int maxCandidates) : h_(nullptr), m_(0), cells_(0)
    {
        check(bl_loopclose_create(default_ctx(), maxCandidates, &h_), "bl_loopclose_create");
    }
    ~LoopCloserT() { bl_loopclose_destroy(h_); }
    LoopCloserT(const LoopCloserT&) = delete;
    LoopCloserT& operator=(const LoopCloserT&) = delete;

    // the kept candidates' edges, ascending q; of `like` only the resolution is read
    std::vector<bl_posegraph_edge_t> find(const ScanHistoryT<Pose, Lidar>& history, OccupancyGrid& like, const bl_loopclose_params_t& params)
    {
        return find(history.device(), like.device(), params);
    }
    std::vector<bl_posegraph_edge_t> find(bl_scanlog* log, const bl_grid* like, const bl_loopclose_params_t& params)
    {
        int m = 0;
        check(bl_loopclose_find(h_, log, like, &params, &m), "bl_loopclose_find");
        m_ = m; cells_ = params.submap_cells;
        return edges();
    }
    // find with the partners by place recognition: params.radius is not read
    std::vector<bl_posegraph_edge_t> findPlaces(const ScanHistoryT<Pose, Lidar>& history, OccupancyGrid& like, const bl_loopclose_params_t& params,
                                                const bl_place_params_t& place)
    {
        return findPlaces(history.device(), like.device(), params, place);
    }
    std::vector<bl_posegraph_edge_t> findPlaces(bl_scanlog* log, const bl_grid* like, const bl_loopclose_params_t& params,
                                                const bl_place_params_t& place)
    {
        int m = 0;
        check(bl_loopclose_find_places(h_, log, like, &params, &place, &m), "bl_loopclose_find_places");
        m_ = m; cells_ = params.submap_cells;
        return edges();
    }
    // every query's best pair of the last findPlaces that launched
    std::vector<bl_place_t> places() const
    {
        int n = 0;
        check(bl_loopclose_places(h_, &n, nullptr), "bl_loopclose_places");
        std::vector<bl_place_t> p(static_cast<std::size_t>(n > 0 ? n : 1));
        check(bl_loopclose_places(h_, &n, p.data()), "bl_loopclose_places");
        p.resize(static_cast<std::size_t>(n));
        return p;
    }
    std::vector<bl_posegraph_edge_t> edges() const
    {
        std::vector<bl_posegraph_edge_t> e(static_cast<std::size_t>(m_ > 0 ? m_ : 1));
        int n = 0;
        check(bl_loopclose_edges(h_, &n, e.data()), "bl_loopclose_edges");
        e.resize(static_cast<std::size_t>(n));
        return e;
    }
    // every candidate of the last find: pair, window, flags, match, edge
    std::vector<bl_loopclose_candidate_t> candidates() const
    {
        std::vector<bl_loopclose_candidate_t> c(static_cast<std::size_t>(m_ > 0 ? m_ : 1));
        check(bl_loopclose_candidates(h_, c.data()), "bl_loopclose_candidates");
        c.resize(static_cast<std::size_t>(m_));
        return c;
    }
    // submap m's cells (row-major, submap_cells a side) and origin
    std::vector<int8_t> submap(int m, float originXY[2]) const
    {
        std::vector<int8_t> cells(static_cast<std::size_t>(cells_) * static_cast<std::size_t>(cells_));
        check(bl_loopclose_submap(h_, m, cells.data(), originXY), "bl_loopclose_submap");
        return cells;
    }
    float lastDeviceMs() const
    {
        float ms = 0.0f;
        check(bl_loopclose_last_device_ms(h_, &ms, nullptr), "bl_loopclose_last_device_ms");
        return ms;
    }

    // botlab_amd.close_loops' three-stage gating.  The nodes are the history's recorded poses, the chain is made from them with the
    // information chainInfo on every edge.  One solve with L + 1 subsets -- each candidate alone and all together (the graph needs
    // maxSubsets >= L + 1) -- drops the candidates whose alone-cost exceeds `gate`; the survivors are solved, those whose own chi2
    // exceeds the gate are dropped, and if any fell the rest is solved again.  The poses are written back to the history.
    static LoopCloseOutcome close(ScanHistoryT<Pose, Lidar>& history, PoseGraphT<Pose>& graph, const std::vector<bl_posegraph_edge_t>& candidates,
                                  const double chainInfo[6], double gate = 11.345, const bl_posegraph_params_t& params = poseGraphParams())
    {
        LoopCloseOutcome out;
        const int L = static_cast<int>(candidates.size()), n = history.size();
        graph.setNodesFromLog(history.device(), 0, n);
        graph.setChainFromNodes(chainInfo);
        out.kept = candidates;
        if (L > 0) {
            graph.setLoops(candidates);
            const int words = (L + 31) / 32;
            std::vector<uint32_t> masks(static_cast<std::size_t>(L + 1) * static_cast<std::size_t>(words), 0u);
            for (int l = 0; l < L; ++l) {
                masks[static_cast<std::size_t>(l) * words + (l >> 5)] = 1u << (l & 31);
                masks[static_cast<std::size_t>(L) * words + (l >> 5)] |= 1u << (l & 31);
            }
            graph.solve(params, L + 1, masks);
            const std::vector<bl_posegraph_result_t> r = graph.results();
            out.kept.clear();
            for (int l = 0; l < L; ++l) {
                out.alone.push_back(r[static_cast<std::size_t>(l)].cost_after);
                if (r[static_cast<std::size_t>(l)].cost_after <= gate) out.kept.push_back(candidates[static_cast<std::size_t>(l)]);
            }
        }
        graph.setLoops(out.kept);
        graph.solve(params);
        if (!out.kept.empty()) {
            std::vector<double> before, after;
            graph.edgeChi2(0, before, after);
            std::vector<bl_posegraph_edge_t> still;
            for (std::size_t l = 0; l < out.kept.size(); ++l)
                if (after[static_cast<std::size_t>(n - 1) + l] <= gate) still.push_back(out.kept[l]);
            if (still.size() != out.kept.size()) {
                out.kept = still;
                graph.setLoops(out.kept);
                graph.solve(params);
            }
        }
        graph.posesToLog(0, history.device(), 0);
        out.result = graph.results()[0];
        return out;
    }

    bl_loopclose* device() const { return h_; }

private:
    bl_loopclose* h_;
    int m_, cells_;
};

}  // namespace botlab_hip

#endif  // BOTLAB_LOOP_CLOSER_HPP
