// Compile check of include/botlab/beam_model.hpp, ParticleFilterT::reweighBeam and OccupancyGridSLAMT::setBeamModel (g++ -std=c++11
// -fsyntax-only), a translation unit of its own beside check_headers.cpp.  See tests/cpp/beam_model_test.cpp for the run-time check.
#include "dropin_test_types.hpp"
#include <botlab/beam_model.hpp>
#include <botlab/slam_driver.hpp>

typedef botlab_hip::BeamModelT<pose_xyt_t, lidar_t> CheckBeam;
typedef botlab_hip::ParticleFilterT<pose_xyt_t, lidar_t, particle_t, particles_t> CheckBeamFilter;

static_assert(sizeof(bl_beam_params_t) == 56, "bl_beam_params_t is 56 bytes");

void touch_beam_model(const botlab_hip::OccupancyGrid& map, const lidar_t& scan, const pose_xyt_t& pose, CheckBeamFilter& pf)
{
    CheckBeam beam, beam2(botlab_hip::default_beam_params());
    bl_beam_params_t p = botlab_hip::default_beam_params();
    p.span = 1 << 20; p.ray_stride = 2;
    (void)beam.setParams(p);
    std::vector<pose_xyt_t> poses(3, pose);
    (void)beam.scores(map, scan, poses);
    (void)beam.units(3);
    (void)beam.debugCast(map, scan, pose).p.size();
    (void)beam.tables(20.0f).rand; (void)CheckBeam::unitTable(); (void)beam.debugPath(); (void)beam.lastDeviceMs(); (void)beam.device();
    const pose_xyt_t est = pf.reweighBeam(beam, map, scan);
    (void)est.x;
}
