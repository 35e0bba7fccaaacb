// pose_graph.hpp -- the pose-graph back end over the C ABI (bl_posegraph_*, include/botlab_hip.h, "pose graph"):
// nodes, a chain of odometry edges, loop edges, and solve() -- Gauss-Newton with Levenberg-Marquardt step control, one workgroup per
// subset of the loop edges, every subset in one launch.  The corrected poses go back into a ScanHistoryT (map_rebuild.hpp), whose
// rebuild() makes the map at them.  OccupancyGridSLAMT::optimizeHistory (slam_driver.hpp) is that sequence on the driver's history.
//
// Every rule is the C header's.  C++11.
#ifndef BOTLAB_POSE_GRAPH_HPP
#define BOTLAB_POSE_GRAPH_HPP

#include <cstdint>
#include <vector>

#include "botlab_dropin.hpp"

namespace botlab_hip {

// the defaults are untuned: they end the loop graphs of the tests in 3 - 4 accepted steps
inline bl_posegraph_params_t poseGraphParams(int fixed = 0)
{
    bl_posegraph_params_t p;
    p.fixed = fixed; p.max_tries = 20; p.max_cg = 500; p.pad = 0;
    p.lambda0 = 1e-6; p.lambda_up = 10.0; p.lambda_down = 0.1;
    p.step_tol = 1e-6; p.rel_tol = 1e-6; p.cg_tol = 1e-8;
    return p;
}

inline bl_posegraph_edge_t poseGraphEdge(int i, int j, double zx, double zy, double ztheta, const double info6[6])
{
    bl_posegraph_edge_t e;
    e.i = i; e.j = j; e.z[0] = zx; e.z[1] = zy; e.z[2] = ztheta;
    for (int q = 0; q < 6; ++q) e.info[q] = info6[q];
    return e;
}

template <class Pose>
class PoseGraphT {
public:
    PoseGraphT(int maxNodes, int maxLoopEdges, int maxSubsets = 1) : h_(nullptr), n_(0), loops_(0), subsets_(0)
    {
        check(bl_posegraph_create(default_ctx(), maxNodes, maxLoopEdges, maxSubsets, &h_), "bl_posegraph_create");
    }
    ~PoseGraphT() { bl_posegraph_destroy(h_); }
    PoseGraphT(const PoseGraphT&) = delete;
    PoseGraphT& operator=(const PoseGraphT&) = delete;

    // new nodes drop the chain and the loop edges
    void setNodes(const std::vector<Pose>& poses)
    {
        std::vector<bl_pose_xyt_t> raw;
        for (std::size_t i = 0; i < poses.size(); ++i) raw.push_back(pose_in(poses[i]));
        check(bl_posegraph_set_nodes(h_, static_cast<int>(raw.size()), raw.data()), "bl_posegraph_set_nodes");
        n_ = static_cast<int>(raw.size()); loops_ = 0;
    }
    // entries first .. first + count - 1 of a scan log, device to device
    void setNodesFromLog(bl_scanlog* log, int first, int count)
    {
        check(bl_posegraph_set_nodes_from_log(h_, log, first, count), "bl_posegraph_set_nodes_from_log");
        n_ = count; loops_ = 0;
    }
    void setChain(const std::vector<bl_posegraph_edge_t>& edges) { check(bl_posegraph_set_chain(h_, edges.data()), "bl_posegraph_set_chain"); }
    // z_k = the relative pose of the nodes k, k + 1; the same information for every chain edge: xx, xy, yy, xt, yt, tt
    void setChainFromNodes(const double info6[6]) { check(bl_posegraph_set_chain_from_nodes(h_, info6), "bl_posegraph_set_chain_from_nodes"); }
    void setLoops(const std::vector<bl_posegraph_edge_t>& edges)
    {
        check(bl_posegraph_set_loops(h_, static_cast<int>(edges.size()), edges.empty() ? nullptr : edges.data()), "bl_posegraph_set_loops");
        loops_ = static_cast<int>(edges.size());
    }

    // one subset with every loop edge on
    void solve(const bl_posegraph_params_t& params)
    {
        check(bl_posegraph_solve(h_, &params, 1, nullptr), "bl_posegraph_solve");
        subsets_ = 1;
    }
    // masks: nSubsets x ((loop edges + 31) / 32) words, bit l of a subset's words: loop edge l is in force
    void solve(const bl_posegraph_params_t& params, int nSubsets, const std::vector<uint32_t>& masks)
    {
        check(bl_posegraph_solve(h_, &params, nSubsets, masks.data()), "bl_posegraph_solve");
        subsets_ = nSubsets;
    }
    std::vector<bl_posegraph_result_t> results() const
    {
        std::vector<bl_posegraph_result_t> r(static_cast<std::size_t>(subsets_ > 0 ? subsets_ : 1));
        check(bl_posegraph_results(h_, r.data()), "bl_posegraph_results");
        r.resize(static_cast<std::size_t>(subsets_));
        return r;
    }
    // a subset's poses narrowed once to the floats of Pose, utime carried through; xyt (optional): x, y, theta in double, 3 a node
    std::vector<Pose> poses(int subset = 0, std::vector<double>* xyt = nullptr) const
    {
        std::vector<bl_pose_xyt_t> raw(static_cast<std::size_t>(n_ > 0 ? n_ : 1));
        if (xyt) xyt->resize(static_cast<std::size_t>(3 * n_));
        check(bl_posegraph_poses(h_, subset, raw.data(), xyt ? xyt->data() : nullptr), "bl_posegraph_poses");
        std::vector<Pose> out;
        for (int i = 0; i < n_; ++i) out.push_back(pose_out<Pose>(raw[static_cast<std::size_t>(i)]));
        return out;
    }
    // e' Omega e of every edge, chain first, at the nodes and at the subset's result
    void edgeChi2(int subset, std::vector<double>& before, std::vector<double>& after) const
    {
        before.assign(static_cast<std::size_t>(n_ - 1 + loops_), 0.0); after = before;
        check(bl_posegraph_edge_chi2(h_, subset, before.data(), after.data()), "bl_posegraph_edge_chi2");
    }
    // over the recorded poses of entries first .. first + nodes - 1, device to device
    void posesToLog(int subset, bl_scanlog* log, int first) { check(bl_posegraph_poses_to_log(h_, subset, log, first), "bl_posegraph_poses_to_log"); }
    float lastDeviceMs() const
    {
        float ms = 0.0f;
        check(bl_posegraph_last_device_ms(h_, &ms), "bl_posegraph_last_device_ms");
        return ms;
    }
    int nodes() const { return n_; }
    bl_posegraph* device() const { return h_; }

private:
    bl_posegraph* h_;
    int n_, loops_, subsets_;
};

}  // namespace botlab_hip

#endif  // BOTLAB_POSE_GRAPH_HPP
