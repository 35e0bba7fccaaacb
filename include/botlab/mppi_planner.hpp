// mppi_planner.hpp -- MppiPlannerT: the sampling local planner of libbotlab_hip.so (bl_mppi_*, botlab_hip.h) for C++ hosts:
// model-predictive path-integral control over a computed NavigationFieldT.  Where LocalPlannerT scores constant (v, w) arcs, this one
// draws perturbed control sequences around the sequence it holds from the previous tick, rolls them out and commands the first
// control of their softmin-weighted average.  Header-only over the C ABI like the rest of include/botlab/.  Sample count, horizon,
// lambda, the noises and the weights are untuned knobs, and nothing here publishes the command.
#ifndef BOTLAB_MPPI_PLANNER_HPP
#define BOTLAB_MPPI_PLANNER_HPP

#include <cstdint>
#include <vector>

#include <botlab/local_planner.hpp>

namespace botlab_hip {

inline bl_mppi_params_t mppi_params(float v_max = 0.5f, float w_max = 2.5f, uint64_t seed = 1)
{
    bl_mppi_params_t p;
    p.v_min = 0.0f; p.v_max = v_max; p.w_max = w_max;
    p.acc_v = 2.0f; p.acc_w = 12.0f;
    p.dt_sim = 0.05f;
    p.noise_v = 0.25f; p.noise_w = 1.5f;
    p.n_samples = 1024; p.horizon = 10; p.n_sub = 2;         // a control period is n_sub * dt_sim = 0.1 s
    p.lambda = 64;
    p.w_field = 16; p.w_heading = 1; p.w_clear = 1;
    p.pad = 0;
    p.seed = seed;
    return p;
}

template <class Pose, class Path, class Command = motor_command_t>
class MppiPlannerT {
public:
    typedef NavigationFieldT<Pose, Path> NavigationField;

    explicit MppiPlannerT(const bl_mppi_params_t& params = mppi_params()) : h_(nullptr), tick_(0), stream_(0)
    {
        check(bl_mppi_create(default_ctx(), &h_), "bl_mppi_create");
        setParams(params);
    }
    ~MppiPlannerT() { if (h_) bl_mppi_destroy(h_); }
    MppiPlannerT(const MppiPlannerT&) = delete;
    MppiPlannerT& operator=(const MppiPlannerT&) = delete;

    // forgets the held sequence: its length is the horizon's
    void setParams(const bl_mppi_params_t& params)
    {
        check(bl_mppi_set_params(h_, &params), "bl_mppi_set_params");
        params_ = params;
        seq_.assign(static_cast<size_t>(2 * params.horizon), 0);
        last_flags_ = 0;
    }
    const bl_mppi_params_t& params() const { return params_; }
    void setStream(uint32_t stream) { stream_ = stream; }    // which robot or hypothesis draws
    uint32_t tick() const { return tick_; }

    // The command for a robot at `pose` moving at (v, w), warm-started from the held sequence, which the call replaces; utime is
    // the pose's.  REACHED, OFF_FIELD and BLOCKED all command (0, 0): `result`, if given, tells them apart.  Call advance() once
    // per control period, after the command is taken.
    Command command(const Pose& pose, float v, float w, const NavigationField& field, bl_mppi_result_t* result = nullptr)
    {
        return plan(pose, v, w, field, nullptr, nullptr, result);
    }
    // command(), with every rollout -- the samples' and the averaged sequence's -- timed against the confirmed moving tracks of an
    // ObstacleTrackerT (obstacle_tracks.hpp); `field` is computed over the tracker's composeStatic
    template <class Tracker>
    Command commandMoving(const Pose& pose, float v, float w, const NavigationField& field, const Tracker& tracker, const bl_localplan_moving_t& moving,
                          bl_mppi_result_t* result = nullptr)
    {
        return plan(pose, v, w, field, tracker.device(), &moving, result);
    }
    // the next tick: the held sequence shifted by one period, its last control repeated; zeros after any flag but FELL_BACK
    void advance()
    {
        const size_t T = seq_.size() / 2;
        if (last_flags_ & ~BL_MPPI_FELL_BACK) seq_.assign(seq_.size(), 0);
        else for (size_t t = 0; t + 1 < T; ++t) { seq_[2 * t] = seq_[2 * t + 2]; seq_[2 * t + 1] = seq_[2 * t + 3]; }
        ++tick_;
    }
    // the held sequence: int32 [horizon][2], (v, w) in units of 2^-16
    const std::vector<int32_t>& sequence() const { return seq_; }
    // what a GUI draws: the horizon * n_sub poses of the held sequence from `pose`
    std::vector<Pose> rollout(const Pose& pose, float v, float w, const NavigationField& field) const
    {
        bl_mppi_state_t s = state(pose, v, w);
        std::vector<bl_pose_xyt_t> buf(static_cast<size_t>(params_.horizon * params_.n_sub));
        check(bl_mppi_debug_rollout(h_, field.device(), &s, seq_.data(), buf.data()), "bl_mppi_debug_rollout");
        std::vector<Pose> out;
        for (size_t k = 0; k < buf.size(); ++k) out.push_back(pose_out<Pose>(buf[k]));
        return out;
    }
    bl_mppi* device() const { return h_; }

private:
    bl_mppi_state_t state(const Pose& pose, float v, float w) const
    {
        bl_mppi_state_t s;
        s.s.pose = pose_in(pose); s.s.v = v; s.s.w = w;
        s.tick = tick_; s.stream = stream_;
        return s;
    }
    Command plan(const Pose& pose, float v, float w, const NavigationField& field, bl_obstracks* tracker, const bl_localplan_moving_t* moving,
                 bl_mppi_result_t* result)
    {
        bl_mppi_state_t s = state(pose, v, w);
        bl_mppi_result_t r;
        std::vector<int32_t> out(seq_.size());
        check(bl_mppi_plan(h_, field.device(), tracker, moving, &s, 1, seq_.data(), out.data(), &r), "bl_mppi_plan");
        seq_.swap(out);
        last_flags_ = r.flags;
        if (result) *result = r;
        Command c;
        c.utime = pose.utime; c.trans_v = r.trans_v; c.angular_v = r.angular_v;
        return c;
    }

    bl_mppi* h_;
    bl_mppi_params_t params_;
    std::vector<int32_t> seq_;
    int32_t last_flags_;
    uint32_t tick_, stream_;
};

}  // namespace botlab_hip

#endif  // BOTLAB_MPPI_PLANNER_HPP
