// bl_pfmodel.h's host part, array by array, for tests/test_pfmodel_header_cpu.py (built as a shared object by the test with
// -ffp-contract=off, as the library is): updateAction, applyAction from a noise table, the plain sensor model of one particle, the
// units of a score, the low-variance draw and the exported particle.
#include "../../botlab_amd/csrc/bl_pfmodel.h"

extern "C" {

// bl_action_update over odo[0 .. n - 1] from a reset state: (rot1, trans, rot2) and moved after every call
void pm_action_seq(int n, const bl_pose_xyt_t* odo, double* rtr, int* moved)
{
    bl_action_state s;
    memset(&s, 0xff, sizeof(s));                 // the reset alone must make the state usable
    bl_action_reset(s);
    for (int i = 0; i < n; ++i) {
        moved[i] = bl_action_update(s, odo[i]) ? 1 : 0;
        rtr[3 * i] = s.rot1; rtr[3 * i + 1] = s.trans; rtr[3 * i + 2] = s.rot2;
    }
}
void pm_action_stds(double* stds)
{
    bl_action_state s;
    bl_action_reset(s);
    const bl_pose_xyt_t p = {0, 0.0f, 0.0f, 0.0f};
    (void)bl_action_update(s, p);
    stds[0] = s.rot1Std; stds[1] = s.transStd; stds[2] = s.rot2Std;
}

// bl_pf_apply_action of n source poses (x, y, theta) with the rows of a noise table
struct pm_args { const float* noise; double rot1, trans, rot2, rot1Std, transStd, rot2Std; uint32_t seed_lo, seed_hi, step; };
void pm_apply_noise(int n, const float* src, const float* noise, float* out)
{
    pm_args a;
    memset(&a, 0, sizeof(a));
    a.noise = noise;
    for (int i = 0; i < n; ++i) {
        const float4 s = {src[3 * i], src[3 * i + 1], src[3 * i + 2], 0.0f};
        bl_pf_apply_action(a, i, i, s, out[3 * i], out[3 * i + 1], out[3 * i + 2]);
    }
}

// 2 * SensorModel::likelihood of one particle (parent pose pb at utime tb, pose pe at te) over the n kept rays of a scan:
// bl_ray_pose + bl_ray_setup + bl_score_ray_half_units over bl_grid_odds, summed.  frame = (ox, oy, mpc, cpm)
long long pm_likelihood_half_units(int width, int height, const float* frame, const int8_t* cells, const float* pb, int64_t tb, const float* pe,
                                   int64_t te, int n, const float* ranges, const float* thetas, const int64_t* times)
{
    bl_frame f;
    f.width = width; f.height = height; f.ox = frame[0]; f.oy = frame[1]; f.mpc = frame[2]; f.cpm = frame[3];
    const bl_pose3 b = {pb[0], pb[1], pb[2]}, e = {pe[0], pe[1], pe[2]};
    const bool interp = tb != te;
    const double t_den = interp ? (double)(te - tb) : 1.0;
    long long acc = 0;
    for (int i = 0; i < n; ++i) {
        float sx, sy, sn, cs;
        int isx, isy;
        bl_ray_setup(f, bl_ray_pose(interp, b, e, times, i, tb, t_den), thetas[i], &sx, &sy, &isx, &isy, &sn, &cs);
        acc += bl_score_ray_half_units(f.cpm, sx, sy, isx, isy, ranges[i], cs, sn, [&](int x, int y) { return bl_grid_odds(cells, f, x, y); });
    }
    return acc;
}

unsigned long long pm_score_units(long long half_units) { return bl_score_units(half_units); }

double pm_resample_offset(int rand_value, double M_inv) { return bl_resample_offset(rand_value, M_inv); }

// the low-variance draw of n particles from n units: the first i whose prefix reaches the target, clamped to n - 1
void pm_resample(int n, const unsigned long long* units, int rand_value, int32_t* idx)
{
    unsigned long long S = 0;
    for (int i = 0; i < n; ++i) S += units[i];
    const double M_inv = 1.0 / n, r = bl_resample_offset(rand_value, M_inv);
    for (int m = 0; m < n; ++m) {
        const double T = bl_resample_target(r, m, M_inv, (double)S);
        unsigned long long prefix = 0;
        int i = 0;
        for (; i < n - 1; ++i) { prefix += units[i]; if (bl_resample_reaches(T, prefix)) break; }
        idx[m] = i;
    }
}

// bl_particle_fill into 56 bytes the caller has filled with a pattern; the weight is the caller's
void pm_particle(bl_particle_t* o, const float* pose, int64_t utime, const float* parent, int64_t parent_utime, double weight)
{
    const float4 p = {pose[0], pose[1], pose[2], 7.0f}, q = {parent[0], parent[1], parent[2], 9.0f};
    bl_particle_fill(o, p, utime, q, parent_utime);
    o->weight = weight;
}

}
