// Compile check of include/botlab/clearance_grid.hpp, BeamModelT::scoresLeap / reweighLeap / debugLeap and
// ParticleFilterT::reweighBeamLeap (g++ -std=c++11 -fsyntax-only), a translation unit of its own beside check_headers.cpp.
// See tests/cpp/clearance_test.cpp for the run-time check.
#include "dropin_test_types.hpp"
#include <botlab/clearance_grid.hpp>
#include <botlab/slam_driver.hpp>

typedef botlab_hip::BeamModelT<pose_xyt_t, lidar_t> CheckBeam;
typedef botlab_hip::ClearanceGridT<pose_xyt_t, lidar_t> CheckClearance;
typedef botlab_hip::ParticleFilterT<pose_xyt_t, lidar_t, particle_t, particles_t> CheckClearanceFilter;

static_assert(sizeof(bl_clearance_info_t) == 32, "bl_clearance_info_t is 32 bytes");

void touch_clearance_grid(const botlab_hip::OccupancyGrid& map, const lidar_t& scan, const pose_xyt_t& pose, CheckClearanceFilter& pf)
{
    CheckBeam beam;
    CheckClearance grid, grid2(255);
    grid.build(map);
    grid2.build(map, 2);
    grid.update(map, 1, 2, 3, 4);
    (void)grid.info().bytes; (void)grid.read(0, 0, 1, 1).size(); (void)grid.lastDeviceMs(); (void)grid2.device();
    std::vector<pose_xyt_t> poses(3, pose);
    (void)beam.scoresLeap(grid, scan, poses);
    (void)beam.units(3);
    std::vector<int32_t> rounds;
    (void)beam.debugLeap(grid, scan, pose, &rounds).p.size();
    const pose_xyt_t a = beam.reweighLeap(pf, grid, scan), b = pf.reweighBeamLeap(beam, grid, scan);
    (void)a.x; (void)b.x;
}
