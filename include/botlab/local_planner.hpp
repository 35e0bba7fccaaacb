// local_planner.hpp -- LocalPlannerT: the local planner of libbotlab_hip.so (bl_localplan_*, botlab_hip.h) for C++ hosts: the
// velocity command of the next control period, by rollout of every reachable (v, w) pair over a computed NavigationFieldT.  It
// stands where the reference's MotionController (src/mbot/motion_controller.cpp) forms an mbot_motor_command_t; header-only over
// the C ABI like the rest of include/botlab/.
#ifndef BOTLAB_LOCAL_PLANNER_HPP
#define BOTLAB_LOCAL_PLANNER_HPP

#include <cstdint>
#include <vector>

#include <botlab/nav_field.hpp>

namespace botlab_hip {

// the fields of lcmtypes/mbot_motor_command_t.lcm, for hosts without the lcm-gen header
struct motor_command_t { int64_t utime; float trans_v; float angular_v; };

inline bl_localplan_params_t local_plan_params(float v_max = 0.5f, float w_max = 2.5f, float dt_control = 0.1f)
{
    bl_localplan_params_t p;
    p.v_min = 0.0f; p.v_max = v_max; p.w_max = w_max;
    p.acc_v = 2.0f; p.acc_w = 12.0f;
    p.dt_control = dt_control; p.dt_sim = 0.05f;
    p.n_v = 32; p.n_w = 129; p.n_steps = 40;
    p.w_field = 16; p.w_heading = 1; p.w_clear = 1; p.w_speed = 8;
    return p;
}

// how the rollout's steps relate to a tracker's updates (commandMoving): stepsPerUpdate steps of dt_sim make one update, leadSteps of
// them have passed since the last one, and a moving box is widened by marginCells
inline bl_localplan_moving_t local_plan_moving(int stepsPerUpdate, int marginCells = 0, int leadSteps = 0)
{
    bl_localplan_moving_t m;
    m.steps_per_update = stepsPerUpdate; m.margin_cells = marginCells; m.lead_steps = leadSteps; m.reserved = 0;
    return m;
}

template <class Pose, class Path, class Command = motor_command_t>
class LocalPlannerT {
public:
    typedef NavigationFieldT<Pose, Path> NavigationField;

    explicit LocalPlannerT(const bl_localplan_params_t& params = local_plan_params()) : h_(nullptr)
    {
        check(bl_localplan_create(default_ctx(), &h_), "bl_localplan_create");
        setParams(params);
    }
    ~LocalPlannerT() { if (h_) bl_localplan_destroy(h_); }
    LocalPlannerT(const LocalPlannerT&) = delete;
    LocalPlannerT& operator=(const LocalPlannerT&) = delete;

    void setParams(const bl_localplan_params_t& params)
    {
        check(bl_localplan_set_params(h_, &params), "bl_localplan_set_params");
        params_ = params;
    }
    const bl_localplan_params_t& params() const { return params_; }

    // the command for a robot at `pose` moving at (v, w); utime is the pose's.  REACHED, OFF_FIELD and BLOCKED all command (0, 0):
    // `result`, if given, tells them apart.
    Command command(const Pose& pose, float v, float w, const NavigationField& field, bl_localplan_result_t* result = nullptr) const
    {
        bl_localplan_state_t s;
        s.pose = pose_in(pose); s.v = v; s.w = w;
        bl_localplan_result_t r;
        check(bl_localplan_commands(h_, field.device(), &s, 1, &r), "bl_localplan_commands");
        if (result) *result = r;
        Command c;
        c.utime = pose.utime; c.trans_v = r.trans_v; c.angular_v = r.angular_v;
        return c;
    }
    // several robots, or the best few particles, in one launch sequence
    std::vector<bl_localplan_result_t> commands(const std::vector<bl_localplan_state_t>& states, const NavigationField& field) const
    {
        std::vector<bl_localplan_result_t> out(states.size());
        if (!states.empty()) check(bl_localplan_commands(h_, field.device(), states.data(), static_cast<int>(states.size()), out.data()), "bl_localplan_commands");
        return out;
    }
    // command(), with every rollout timed against the confirmed moving tracks of an ObstacleTrackerT (obstacle_tracks.hpp): a candidate
    // whose cell at step k lies in a track's box at step k is refused.  `field` is computed over the tracker's composeStatic
    // (MotionPlannerT::setMapWithStaticObstacles).
    template <class Tracker>
    Command commandMoving(const Pose& pose, float v, float w, const NavigationField& field, const Tracker& tracker, const bl_localplan_moving_t& moving,
                          bl_localplan_result_t* result = nullptr) const
    {
        bl_localplan_state_t s;
        s.pose = pose_in(pose); s.v = v; s.w = w;
        bl_localplan_result_t r;
        check(bl_localplan_commands_moving(h_, field.device(), tracker.device(), &moving, &s, 1, &r), "bl_localplan_commands_moving");
        if (result) *result = r;
        Command c;
        c.utime = pose.utime; c.trans_v = r.trans_v; c.angular_v = r.angular_v;
        return c;
    }
    template <class Tracker>
    std::vector<bl_localplan_result_t> commandsMoving(const std::vector<bl_localplan_state_t>& states, const NavigationField& field, const Tracker& tracker,
                                                      const bl_localplan_moving_t& moving) const
    {
        std::vector<bl_localplan_result_t> out(states.size());
        if (!states.empty())
            check(bl_localplan_commands_moving(h_, field.device(), tracker.device(), &moving, states.data(), static_cast<int>(states.size()), out.data()),
                  "bl_localplan_commands_moving");
        return out;
    }
    // what a GUI draws: the poses of candidate c
    std::vector<Pose> rollout(const Pose& pose, float v, float w, const NavigationField& field, int c) const
    {
        bl_localplan_state_t s;
        s.pose = pose_in(pose); s.v = v; s.w = w;
        std::vector<bl_pose_xyt_t> buf(static_cast<size_t>(params_.n_steps));
        check(bl_localplan_debug_rollout(h_, field.device(), &s, c, buf.data()), "bl_localplan_debug_rollout");
        std::vector<Pose> out;
        for (size_t k = 0; k < buf.size(); ++k) out.push_back(pose_out<Pose>(buf[k]));
        return out;
    }
    bl_localplan* device() const { return h_; }

private:
    bl_localplan* h_;
    bl_localplan_params_t params_;
};

}  // namespace botlab_hip

#endif  // BOTLAB_LOCAL_PLANNER_HPP
