// bl_pfmodel.h -- what the particle filter (bl_mcl.hip) and RB-SLAM (bl_rbslam.hip, bl_rbslam_match.h) share: the reference's motion
// and sensor model (action_model.cpp, sensor_model.cpp), initializeFilterAtPose and the low-variance draw (particle_filter.cpp).  Both
// must produce the reference's particles bit for bit, and each other's on the device's own noise, so each rule lives here once.
//   host             ActionModel::updateAction: the action state, its update and its reset
//   host and device  applyAction; the bounds-masked lookup, scoreRay in half-units over any "cell -> odds", the exact ray set-up; the
//                    units of a score; the resampling offset, target and comparison; the exported particle
//   device           three normals from a Philox counter (the host's libm would round them differently) and the initial draw
// What differs stays where it was: k_mcl_main's packed 16-bit and fast-trig scoring, its LDS lookups and MCL_RAY_LOOP*, the searches
// and the strict branch of resample_reaches (bl_mcl.hip); k_rb_plan's bisection (bl_rbslam.hip).
// tests/cpp/pfmodel_ref.cpp compiles the first two parts for the host (tests/test_pfmodel_header_cpu.py).
#ifndef BL_PFMODEL_H
#define BL_PFMODEL_H

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/botlab_hip.h"
#include "bl_math.h"

#if !defined(__HIPCC__)
struct float4 { float x, y, z, w; };
#endif
// ---------------------------------------------------------------------------------------------------------------- updateAction
// ActionModel's state (action_model.hpp:60-78) and ActionModel::updateAction (action_model.cpp:22-75): host scalars, the same libm
// calls as the reference.  Returns `moved`.
struct bl_action_state {
    bl_pose_xyt_t prev_odom;
    bool initialized;
    double rot1, trans, rot2, rot1Std, transStd, rot2Std;
};
inline void bl_action_reset(bl_action_state& s) { s.initialized = false; s.rot1 = s.trans = s.rot2 = 0; }
inline bool bl_action_update(bl_action_state& s, const bl_pose_xyt_t& odometry)
{
    if (!s.initialized) { s.prev_odom = odometry; s.initialized = true; }
    float deltaX = odometry.x - s.prev_odom.x;
    float deltaY = odometry.y - s.prev_odom.y;
    float deltaTheta = (float)bl_angle_diff(odometry.theta, s.prev_odom.theta);
    float dir = 1.0;
    s.rot1 = bl_angle_diff(atan2f(deltaY, deltaX), s.prev_odom.theta);
    s.trans = sqrtf(deltaX * deltaX + deltaY * deltaY);
    if (fabs(s.trans) < 0.0001) { s.rot1 = 0.0f; }
    else if (fabs(s.rot1) > BL_PI / 2.0) { s.rot1 = -bl_angle_diff(BL_PI, s.rot1); dir = -1.0; }
    // (the reference's third branch, |rot1| < -pi/2, can never be taken: action_model.cpp:44-47)
    s.trans *= dir;
    s.rot2 = bl_angle_diff(deltaTheta, s.rot1);
    s.rot1Std = 0.05; s.transStd = 0.005; s.rot2Std = 0.05;
    s.prev_odom = odometry;
    return !((fabs(s.trans) + fabs(s.rot2)) < 0.00001f);
}
// ---------------------------------------------------------------------------------------------------------------- normals, applyAction
#define BL_PF_STREAM 0x6d636c31u             // Philox counter word of the action noise and of the initial draw
#define BL_PF_INIT_STEP 0xffffffffu          // the initial draw's step (an update's step counts up from 0)

#if defined(__HIPCC__)
// three normals of counter (m, step) under key (k0, k1): (0, 1] uniforms, Box-Muller
__device__ __forceinline__ void bl_pf_normals3(uint32_t m, uint32_t step, uint32_t k0, uint32_t k1, float z[3])
{
    uint32_t o[4];
    bl_philox4x32(m, step, BL_PF_STREAM, 0, k0, k1, o);
    float u1 = ((float)(o[0] >> 8) + 1.0f) * (1.0f / 16777216.0f);
    float u2 = ((float)(o[1] >> 8) + 0.5f) * (1.0f / 16777216.0f);
    float u3 = ((float)(o[2] >> 8) + 1.0f) * (1.0f / 16777216.0f);
    float u4 = ((float)(o[3] >> 8) + 0.5f) * (1.0f / 16777216.0f);
    float ra = sqrtf(-2.0f * logf(u1)), rb = sqrtf(-2.0f * logf(u3));
    float s2, c2, c4;
    sincosf(6.2831853071795864769f * u2, &s2, &c2);
    c4 = cosf(6.2831853071795864769f * u4);
    z[0] = ra * c2; z[1] = ra * s2; z[2] = rb * c4;
}

// initializeFilterAtPose (particle_filter.cpp:16-34), particle m of M around (x0, y0, th0): pose + 0.01 z, the last particle the pose
__device__ __forceinline__ void bl_pf_init_draw(float x0, float y0, float th0, int m, int M, uint32_t k0, uint32_t k1, float& x, float& y, float& th)
{
    float z[3];
    bl_pf_normals3((uint32_t)m, BL_PF_INIT_STEP, k0, k1, z);
    x = (float)((double)x0 + 0.01 * (double)z[0]);
    y = (float)((double)y0 + 0.01 * (double)z[1]);
    th = bl_wrap_to_pi((float)((double)th0 + 0.01 * (double)z[2]));
    if (m == M - 1) { x = x0; y = y0; th = th0; }               // posterior_.back().pose = pose
}
#endif  // __HIPCC__

// ActionModel::applyAction (action_model.cpp:78-103) of output particle m from its source pose s.  a: the launch's arguments (noise,
// rot1 .. rot2Std, seed_lo, seed_hi, step).  The sampled (rot1, trans, rot2) are row noise_row of the uploaded table (parity mode)
// or drawn from Philox counter m (device only).  A float heading, then the double libm cos / sin of it (one argument reduction).
// k_rb_weigh and k_rb_match call it; k_mcl_main carries the same lines written out, for its prologue's schedule (see there).
template <class A>
BL_HD void bl_pf_apply_action(const A& a, int m, int noise_row, const float4& s, float& px, float& py, float& pth)
{
    float n1 = 0.f, n2 = 0.f, n3 = 0.f;
    if (a.noise) { n1 = a.noise[3 * noise_row]; n2 = a.noise[3 * noise_row + 1]; n3 = a.noise[3 * noise_row + 2]; }
#if defined(__HIPCC__)
    else {
        float z[3];
        bl_pf_normals3((uint32_t)m, a.step, a.seed_lo, a.seed_hi, z);
        n1 = (float)(a.rot1 + a.rot1Std * (double)z[0]); n2 = (float)(a.trans + a.transStd * (double)z[1]); n3 = (float)(a.rot2 + a.rot2Std * (double)z[2]);
    }
#endif
    const float head = s.z + n1;
    double hs, hc;
    sincos((double)head, &hs, &hc);
    px = (float)((double)s.x + (double)n2 * hc);
    py = (float)((double)s.y + (double)n2 * hs);
    pth = bl_wrap_to_pi(s.z + n1 + n3);
}
// ---------------------------------------------------------------------------------------------------------------- sensor model
// OccupancyGrid::logOdds (occupancy_grid.cpp:63-71), branch-free: an off-grid cell reads cell 0 and is masked to 0
BL_HD int bl_grid_odds(const int8_t* __restrict__ cells, const bl_frame& f, int x, int y)
{
    const bool in = (unsigned int)x < (unsigned int)f.width && (unsigned int)y < (unsigned int)f.height;
    const int v = cells[in ? (size_t)y * f.width + x : (size_t)0];
    return in ? v : 0;
}

// SensorModel::scoreRay (sensor_model.cpp:28-59) in half-units: 2 * odds, o1 or o2 (score = that / 2), for a ray of `range` metres
// along (cs, sn) from (sx, sy) in cells, (isx, isy) its start cell; odds(x, y): the log-odds of a cell.  The two neighbour cells are
// looked up unconditionally: within a 64-lane wave some ray always needs them, so the reference's early-out would only diverge.
template <class Odds>
BL_HD int bl_score_ray_half_units(float cpm, float sx, float sy, int isx, int isy, float range, float cs, float sn, Odds odds)
{
    const float tx = range * cs * cpm, ty = range * sn * cpm;
    const int ex = (int)(tx + sx), ey = (int)(ty + sy);
    // (2 * range * cos) * cpm == 2 * ((range * cos) * cpm) bit for bit: scaling by two is exact and commutes with
    // rounding for normal floats (range > 0.15 and |cos| >= 4e-8 keep every product far from the subnormal range)
    const int xx = (int)((2.0f * tx) + sx), xy = (int)((2.0f * ty) + sy);
    int ax, ay, bx, by;
    bl_bresenham_first_step(ex, ey, isx, isy, &ax, &ay);
    bl_bresenham_first_step(ex, ey, xx, xy, &bx, &by);
    const int o = odds(ex, ey), o1 = odds(ax, ay), o2 = odds(bx, by);
    return o > 0 ? 2 * o : (o1 > 0 ? o1 : (o2 > 0 ? o2 : 0));
}

// The exact set-up of ray n of MovingLaserScan(scan, pb, pe) (moving_laser_scan.cpp:22-37, sensor_model.cpp:29-38).  bl_ray_pose: the
// pose it leaves from, interpolated to its stamp (interp: the two poses' utimes differ) or pe.  bl_ray_setup: from that pose, the
// start in cells, the start cell, and the sine and cosine of the wrapped direction bl_ray_theta (k_mcl_main's rays that all leave the
// particle's own pose take the direction alone: the start is the prologue's).
BL_HD bl_pose3 bl_ray_pose(bool interp, const bl_pose3& pb, const bl_pose3& pe, const int64_t* times, int n, int64_t t_begin, double t_den)
{ return interp ? bl_interpolate_pose(pb, pe, bl_interp_ratio(times[n], t_begin, t_den)) : pe; }
BL_HD float bl_ray_theta(float pose_theta, float ray_theta) { return bl_wrap_to_pi(pose_theta - ray_theta); }
BL_HD void bl_ray_setup(const bl_frame& f, const bl_pose3& rp, float ray_theta, float* sx, float* sy, int* isx, int* isy, float* sn, float* cs)
{
    const float theta = bl_ray_theta(rp.theta, ray_theta);
    bl_global_to_grid(rp.x, rp.y, f, sx, sy);
    *isx = (int)*sx; *isy = (int)*sy;
    bl_sincosf(theta, sn, cs);
}

// computeNormalizedPosterior (particle_filter.cpp:116-141): w = max(score, 0.001) in units of 0.0005, the score in half-units
BL_HD unsigned long long bl_score_units(long long half_units) { return half_units > 0 ? (unsigned long long)half_units * 1000ull : 2ull; }
// ---------------------------------------------------------------------------------------------------------------- low-variance draw
// resamplePosteriorDistribution (particle_filter.cpp:84-103) by the integer-prefix rule: r = (rand / RAND_MAX) / M, U_m = r + m / M,
// T_m = U_m S; output particle m takes the first source i whose prefix of units reaches T_m: T_m <= (double)prefix_i.
BL_HD double bl_resample_offset(int rand_value, double M_inv) { return (((double)rand_value) / (double)RAND_MAX) * M_inv; }
BL_HD double bl_resample_u(double r, int m, double M_inv) { return r + m * M_inv; }
BL_HD double bl_resample_target(double r, int m, double M_inv, double S) { return bl_resample_u(r, m, M_inv) * S; }
BL_HD int bl_resample_reaches(double T, unsigned long long prefix) { return T <= (double)prefix; }
// ---------------------------------------------------------------------------------------------------------------- export
// A particle as particles() hands it out, but for its weight: the padding bytes zeroed, the two utimes of the set
BL_HD void bl_particle_fill(bl_particle_t* o, const float4& pose, int64_t utime, const float4& parent, int64_t parent_utime)
{
    memset(o, 0, sizeof(*o));
    o->pose.utime = utime; o->pose.x = pose.x; o->pose.y = pose.y; o->pose.theta = pose.z;
    o->parent_pose.utime = parent_utime; o->parent_pose.x = parent.x; o->parent_pose.y = parent.y; o->parent_pose.theta = parent.z;
}

#endif  // BL_PFMODEL_H
