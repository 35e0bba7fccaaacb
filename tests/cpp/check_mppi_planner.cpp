// Compile check of MppiPlannerT (include/botlab/mppi_planner.hpp; g++ -std=c++11 -fsyntax-only), a translation unit of its own
// beside check_headers.cpp, with the sizes and offsets botlab_hip.h states.  See tests/cpp/mppi_planner_test.cpp for the run-time
// check on a GPU.
#include <cstddef>
#include "dropin_test_types.hpp"
#include <botlab/obstacle_tracks.hpp>
#include <botlab/mppi_planner.hpp>

typedef botlab_hip::ObstacleLayerT<pose_xyt_t, lidar_t> CheckLayer;
typedef botlab_hip::ObstacleTrackerT<CheckLayer> CheckTracker;
typedef botlab_hip::MppiPlannerT<pose_xyt_t, robot_path_t> CheckMppi;

static_assert(sizeof(bl_mppi_params_t) == 72 && offsetof(bl_mppi_params_t, dt_sim) == 20 && offsetof(bl_mppi_params_t, noise_w) == 28 &&
              offsetof(bl_mppi_params_t, n_samples) == 32 && offsetof(bl_mppi_params_t, lambda) == 44 && offsetof(bl_mppi_params_t, w_field) == 48 &&
              offsetof(bl_mppi_params_t, pad) == 60 && offsetof(bl_mppi_params_t, seed) == 64, "bl_mppi_params_t is 72 bytes");
static_assert(sizeof(bl_mppi_state_t) == 40 && offsetof(bl_mppi_state_t, tick) == 32 && offsetof(bl_mppi_state_t, stream) == 36, "bl_mppi_state_t is 40 bytes");
static_assert(sizeof(bl_mppi_result_t) == 56 && offsetof(bl_mppi_result_t, index_best) == 8 && offsetof(bl_mppi_result_t, cost_best) == 16 &&
              offsetof(bl_mppi_result_t, cost_out) == 24 && offsetof(bl_mppi_result_t, weight_sum) == 32 && offsetof(bl_mppi_result_t, weight_sq_sum) == 40 &&
              offsetof(bl_mppi_result_t, flags) == 48, "bl_mppi_result_t is 56 bytes");
static_assert(BL_MPPI_FELL_BACK == 8 && (BL_MPPI_FELL_BACK & (BL_LOCALPLAN_REACHED | BL_LOCALPLAN_OFF_FIELD | BL_LOCALPLAN_BLOCKED)) == 0, "a flag of its own");

void touch_mppi(const pose_xyt_t& pose, CheckMppi& mp, const CheckMppi::NavigationField& field, CheckTracker& tracker)
{
    bl_mppi_result_t r;
    (void)mp.command(pose, 0.1f, 0.0f, field, &r).trans_v;
    (void)mp.commandMoving(pose, 0.1f, 0.0f, field, tracker, botlab_hip::local_plan_moving(2, 1, 0)).angular_v;
    mp.advance();
    (void)mp.sequence().size();
    (void)mp.rollout(pose, 0.1f, 0.0f, field).size();
    mp.setStream(3);
    (void)mp.tick();
    uint32_t table[257];
    bl_mppi_weight_table(table);
}
