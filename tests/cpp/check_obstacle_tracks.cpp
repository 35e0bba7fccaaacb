// Compile check of include/botlab/obstacle_tracks.hpp and MotionPlannerT::setMapWithTracks (g++ -std=c++11 -fsyntax-only), a
// translation unit of its own beside check_headers.cpp.  See tests/cpp/obstacle_tracks_test.cpp for the run-time check on a GPU.
#include <cstddef>
#include "dropin_test_types.hpp"
#include <botlab/obstacle_tracks.hpp>
#include <botlab/planning_dropin.hpp>

typedef botlab_hip::ObstacleLayerT<pose_xyt_t, lidar_t> CheckLayer;
typedef botlab_hip::ObstacleTrackerT<CheckLayer> CheckTracker;
typedef botlab_hip::MotionPlannerT<pose_xyt_t, robot_path_t> CheckPlanner;

static_assert(sizeof(bl_obstracks_params_t) == 32 && offsetof(bl_obstracks_params_t, min_speed) == 28, "bl_obstracks_params_t is 32 bytes");
static_assert(sizeof(bl_obstracks_compose_t) == 16 && offsetof(bl_obstracks_compose_t, keep_clear) == 12, "bl_obstracks_compose_t is 16 bytes");
static_assert(sizeof(bl_obstrack_t) == 56 && offsetof(bl_obstrack_t, hits) == 20 && offsetof(bl_obstrack_t, area) == 28 &&
              offsetof(bl_obstrack_t, flags) == 48 && offsetof(bl_obstrack_t, slot) == 52, "bl_obstrack_t is 56 bytes");
static_assert(sizeof(bl_obsblob_t) == 56 && offsetof(bl_obsblob_t, sum_y) == 8 && offsetof(bl_obsblob_t, area) == 16 &&
              offsetof(bl_obsblob_t, cx) == 36 && offsetof(bl_obsblob_t, eligible) == 44 && offsetof(bl_obsblob_t, rep) == 52, "bl_obsblob_t is 56 bytes");
static_assert(sizeof(bl_obstracks_stats_t) == 56 && offsetof(bl_obstracks_stats_t, live_cells) == 8 && offsetof(bl_obstracks_stats_t, matched) == 24 &&
              offsetof(bl_obstracks_stats_t, refused) == 48 && offsetof(bl_obstracks_stats_t, rounds) == 52, "bl_obstracks_stats_t is 56 bytes");
static_assert(sizeof(bl_obstracks_state_t) == 16 && offsetof(bl_obstracks_state_t, fresh) == 8, "bl_obstracks_state_t is 16 bytes");

void touch_obstacle_tracks(const botlab_hip::OccupancyGrid& map, const lidar_t& scan, const pose_xyt_t& pose, CheckPlanner& planner)
{
    CheckLayer layer(map.widthInCells(), map.heightInCells());
    CheckTracker tracker(layer), tracker2(layer, botlab_hip::default_obstracks_params());
    bl_obstracks_params_t p = botlab_hip::default_obstracks_params();
    p.min_cells = 2; p.max_cells = 400; p.gate_cells = 6; p.alpha = 100; p.beta = 50; p.confirm_hits = 2; p.max_missed = 5; p.min_speed = 8;
    (void)tracker.setParams(p);
    layer.update(map, scan, pose);
    tracker.update();
    (void)tracker.tryUpdate();
    botlab_hip::OccupancyGrid out;
    tracker.compose(map, out, 8, 3, 4, 2);
    tracker.compose(map, out, 0);
    const std::vector<bl_obstrack_t> t = tracker.tracks();
    if (!t.empty()) (void)botlab_hip::obstacle_track_metric(t[0], map, 0.1).vx;
    (void)tracker.blobs(); (void)tracker.labels(); (void)tracker.stats().tracks; (void)tracker.lastUpdateMs(); (void)tracker.lastComposeMs();
    std::vector<bl_obstrack_t> slots; bl_obstracks_state_t st;
    tracker.download(slots, st);
    (void)tracker.upload(slots, st);
    tracker.reset();
    (void)tracker.device(); (void)tracker.layer().widthInCells();
    planner.setMapWithTracks(map, layer, tracker, 8, pose);
    planner.setMapWithTracks(map, layer, tracker, 8, pose, -1);
    (void)planner.composedMap().widthInCells();
}
