// Compile check of include/botlab/range_table.hpp, BeamModelT::scoresTable / reweighTable / debugLookup, ParticleFilterT::reweighBeamTable
// and OccupancyGridSLAMT::setBeamRangeTable (g++ -std=c++11 -fsyntax-only), a translation unit of its own beside check_headers.cpp.
// See tests/cpp/range_table_test.cpp for the run-time check.
#include "dropin_test_types.hpp"
#include <botlab/range_table.hpp>
#include <botlab/slam_driver.hpp>

typedef botlab_hip::BeamModelT<pose_xyt_t, lidar_t> CheckBeam;
typedef botlab_hip::RangeTableT<pose_xyt_t, lidar_t> CheckTable;
typedef botlab_hip::ParticleFilterT<pose_xyt_t, lidar_t, particle_t, particles_t> CheckTableFilter;

static_assert(sizeof(bl_rangetable_info_t) == 32, "bl_rangetable_info_t is 32 bytes");
static_assert(BL_RANGETABLE_NONE == 0xFFFF, "the sentinel is the largest uint16");

void touch_range_table(const botlab_hip::OccupancyGrid& map, const lidar_t& scan, const pose_xyt_t& pose, CheckTableFilter& pf)
{
    CheckBeam beam;
    CheckTable table, table2(64);
    table.build(beam, map);
    table.update(map, 1, 2, 3, 4);
    (void)table.info().bytes; (void)table.read(0, 0, 1, 1).size(); (void)table.directions().size(); (void)table.lastDeviceMs(); (void)table2.device();
    std::vector<pose_xyt_t> poses(3, pose);
    (void)beam.scoresTable(table, scan, poses);
    (void)beam.units(3);
    std::vector<int32_t> h;
    (void)beam.debugLookup(table, scan, pose, &h).p.size();
    const pose_xyt_t a = beam.reweighTable(pf, table, scan), b = pf.reweighBeamTable(beam, table, scan);
    (void)a.x; (void)b.x;
}
