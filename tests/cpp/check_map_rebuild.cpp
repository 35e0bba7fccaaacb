// Compile check of include/botlab/map_rebuild.hpp and OccupancyGridSLAMT::setScanHistory / rebuildMap (g++ -std=c++11 -fsyntax-only), a
// translation unit of its own beside check_headers.cpp.  See tests/cpp/map_rebuild_driver_test.cpp for the run-time check.
#include "dropin_test_types.hpp"
#include <botlab/map_rebuild.hpp>
#include <botlab/slam_driver.hpp>

typedef botlab_hip::ScanHistoryT<pose_xyt_t, lidar_t> CheckHistory;
struct check_odometry_t { int64_t utime; float x, y, theta; };
typedef botlab_hip::OccupancyGridSLAMT<pose_xyt_t, lidar_t, check_odometry_t, particle_t, particles_t, occupancy_grid_t> CheckHistorySLAM;

static_assert(sizeof(bl_scanlog_stats_t) == 64, "bl_scanlog_stats_t is 64 bytes");

void touch_map_rebuild(botlab_hip::OccupancyGrid& map, const botlab_hip::OccupancyGrid& base, const lidar_t& scan, const pose_xyt_t& pose,
                       const void* devicePose, CheckHistorySLAM& slam)
{
    CheckHistory log(8), small(4, 290);
    (void)log.append(scan, pose);
    (void)log.appendDevicePose(scan, devicePose, pose.utime);
    std::vector<pose_xyt_t> poses = log.poses();
    (void)log.poses(0, 1).size();
    log.setPoses(0, poses);
    (void)log.scan(0).times.size();
    log.rebuild(map, 5.0f, 3, 1, 0, log.size());
    log.rebuild(map, 5.0f, 3, 1, 1, 1, &pose, &base);
    log.rebuild(map, 5.0f, 3, 1, 0, poses, nullptr, &map);
    (void)log.stats().pairs; (void)log.device(); (void)small.size();
    slam.setScanHistory(64);
    slam.rebuildMap();
    slam.rebuildMap(poses);
    (void)slam.scanHistory();
}
