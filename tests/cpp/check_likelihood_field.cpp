// Compile check of include/botlab/likelihood_field.hpp and the OccupancyGridSLAMT switch built on it (g++ -std=c++11
// -fsyntax-only), a translation unit of its own beside check_headers.cpp.  See tests/cpp/likelihood_field_test.cpp for the
// run-time check on a GPU.
#include "dropin_test_types.hpp"
#include <botlab/likelihood_field.hpp>
#include <botlab/slam_driver.hpp>

struct check_odometry_t { int64_t utime = 0; float x = 0, y = 0, theta = 0; };
typedef botlab_hip::OccupancyGridSLAMT<pose_xyt_t, lidar_t, check_odometry_t, particle_t, particles_t, occupancy_grid_t> CheckFieldSLAM;
typedef botlab_hip::ParticleFilterT<pose_xyt_t, lidar_t, particle_t, particles_t> CheckFieldFilter;
typedef botlab_hip::ScanMatcherT<pose_xyt_t, lidar_t> CheckFieldMatcher;

void touch_likelihood_field(const botlab_hip::OccupancyGrid& map, const lidar_t& scan, const pose_xyt_t& pose, CheckFieldFilter& pf,
                            CheckFieldMatcher& matcher, CheckFieldSLAM& slam)
{
    botlab_hip::LikelihoodFieldT lf, lf2(botlab_hip::default_lfield_params());
    bl_lfield_params_t p = botlab_hip::default_lfield_params();
    p.sigma = 0.2f; p.max_cells = 12; p.occ_min = 10; p.peak = 100;
    (void)lf.setParams(p);
    const botlab_hip::OccupancyGrid& field = lf.compute(map);
    (void)lf.computed(); (void)lf.grid().widthInCells(); (void)lf.table(); (void)lf.lastDeviceMs(); (void)lf.device();
    (void)field.logOdds(0, 0);
    botlab_hip::OccupancyGrid own(field);                         // a copy of a view owns its buffer
    (void)own;
    (void)pf.updateFilter(pose, scan, field);
    (void)pf.updateFilterBegin(pose, scan, field);
    pf.initializeFilterAtPose(pose, 7u);
    (void)matcher.match(scan, pose, field, botlab_hip::default_scan_match_params());
    slam.setLikelihoodField(true, p);
    slam.setFilterSeed(1u);
    (void)slam.likelihoodFieldActive(); (void)slam.sensorMap().heightInCells();
}
