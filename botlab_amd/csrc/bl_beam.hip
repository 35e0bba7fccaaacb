// bl_beam.hip -- the ray-cast (beam) sensor model (include/botlab_hip.h, "beam model"): for many poses at once, every used ray of a scan
// cast against the static map as far as the maximum range, the measured range scored against the expected one, and the scores
// turned into weight units for the particle filter.  No reference counterpart; the definition in the header is the contract and
// tests/beam_model.py restates it.
//
//   k_beam_cast   a workgroup per BEAM_WG_POSES poses, a wave per BEAM_WAVE_POSES of them one after the other, a LANE PER RAY: the lane
//                 forms its ray's geometry (the obstacle layer's), walks the reference's Bresenham loop from the start cell towards the
//                 far cell and stops at the first occupied cell.  The loop form needs no division per cell (the closed form that lets
//                 64 lanes share one ray needs one), and a lane that stops early costs nothing further; the price is that a wave runs
//                 as long as its longest ray.  The other form -- 64 cells of one ray per round and a ballot, k_obs_rays' phase 1 -- was
//                 not built and is not measured.  The cells come from the grid through L2 (path 1, the default: measured faster at
//                 200^2 / 10^5 poses and at 2000^2 / 10^4) or, under bl_beam_debug_set, from LDS when the bounding box
//                 of the workgroup's start cells, widened by reach + 2 and clipped to the grid, fits window_bytes (path 0); a cell
//                 of the grid outside a staged window (there is none by construction) would still be read from the grid.  The
//                 three tables live in LDS.  Per pose a wave sum of the rays' integer logarithms (int64); per workgroup the largest score
//                 and the path taken.
//   k_beam_lookup the second scoring form ("range table" in the header): the same launch shape and records, but the expected range of a
//                 ray is one uint16 of a range table (bl_rangetable.hip) -- the row of the pose's start cell at the ray's quantised
//                 heading -- and the measured one the range in quarter cells: no sine, no walk.  Off unless called.
//   k_beam_leap   the third scoring form ("clearance grid" in the header): k_beam_cast's launch shape, records and per-ray values, but
//                 the lane reads a clearance grid (bl_clearance.hip) instead of the map and leaps as far as each entry allows
//                 (beam_first_hit_leap): a few dependent loads through L2 with one 32-bit division each, where the loop reads every
//                 cell.  first, K, the hit cell and everything behind them equal the cast's.  Off unless called.
//   k_beam_final  one workgroup: Smax over the workgroups' records, and how many workgroups took which path.
//   k_beam_units  a thread per pose: the units, to the handle's array and, for a filter, into the record's weight word in place.
//
// The three scoring kernels are their prologue (tables to LDS; the cast's box and window) round one frame, beam_score_poses, with the
// form's per-ray body; the rules of a ray -- start cell, walk, lengths, p, lg, heading index -- are bl_beam_dev.h's.  On the host
// a beam_form says where the expected ranges come from, and the launcher, "scores", "debug" and "reweigh" exist once for all; the
// nine entry points check their form (beam_check_map, beam_check_table, beam_check_clearance) and call them.
//
// Integers only behind the end cells; no atomics; no workgroup waits for another; no result depends on the launch shape.
#include <limits.h>
#include <math.h>
#include <string.h>

#include "bl_beam_dev.h"

#define BEAM_MIN_RANGE 0.15f              // moving_laser_scan.cpp:24, as the obstacle layer
#define BEAM_THREADS 512
#define BEAM_WAVE_POSES 4
#define BEAM_WG_POSES ((BEAM_THREADS / 64) * BEAM_WAVE_POSES)
#define BEAM_WINDOW_BYTES 40960           // a 200 x 200 grid whole; with the tables 50 176 bytes of LDS: three workgroups per CU
#define BEAM_OFF INT64_MIN

struct beam_state { long long smax; int staged_wgs, direct_wgs; };

struct beam_args {
    const int8_t* cells; bl_frame f;
    const float* ranges; const float* thetas; int R;     // the used rays
    const float4* poses; int n;                           // x, y, theta (the fourth word is not read)
    float max_range; int occ_min, hit_cut, reach;
    uint32_t rnd, max_free, max_blocked; int ln2;
    const uint32_t* tables;
    int window_bytes, stage;
    long long* scores; long long* wg_max; uint8_t* wg_path;
    int32_t* dbg;                                         // null, or [5][R] of pose 0: first, K, z, zstar, p
};

struct beam_window { int x0, y0, w, h; };

// lg(p) of one used ray of one pose (0 with p = 0 for a ray that `has` drops); dbg as in beam_args
template <bool STAGED>
__device__ __forceinline__ int beam_ray(const beam_args& a, const uint32_t* s_tab, const int8_t* s_win, const beam_window& win, float px, float py,
                                        int sx, int sy, float ptheta, int r, int32_t* dbg)
{
    const int W = a.f.width, H = a.f.height;
    const float range = a.ranges[r];
    const bool is_max = range >= a.max_range;
    const float ang = bl_wrap_to_pi(ptheta - a.thetas[r]);
    float sn, cs;
    bl_sincosf_cells(ang, &sn, &cs);
    const float fmx = a.max_range * cs * a.f.cpm + px, fmy = a.max_range * sn * a.f.cpm + py;
    const float fex = range * cs * a.f.cpm + px, fey = range * sn * a.f.cpm + py;
    bool has = __builtin_fabsf(fmx) < 0x1p30f && __builtin_fabsf(fmy) < 0x1p30f;
    if (!is_max) has = has && __builtin_fabsf(fex) < 0x1p30f && __builtin_fabsf(fey) < 0x1p30f;
    int first = -1, K = -1, z = -1, zstar = -1, lgp = 0;
    uint32_t p = 0;
    if (has) {
        // a cell outside the grid is free and the walk goes on: the far cell may lie anywhere
        const beam_hit hit = beam_first_hit(sx, sy, (int)fmx, (int)fmy, [&](int x, int y) {
            bool occ = false;
            if ((unsigned int)x < (unsigned int)W && (unsigned int)y < (unsigned int)H) {
                const int lx = x - win.x0, ly = y - win.y0;
                if (STAGED && (unsigned int)lx < (unsigned int)win.w && (unsigned int)ly < (unsigned int)win.h) occ = s_win[ly * win.w + lx] >= a.occ_min;
                else occ = a.cells[(size_t)y * W + x] >= a.occ_min;
            }
            return occ;
        });
        first = hit.first; K = hit.K;
        const bool expect = first < K;
        if (expect) zstar = beam_quarter(hit.x, hit.y, sx, sy);
        if (is_max) {
            p = expect ? a.max_blocked : a.max_free;
        } else {
            z = beam_quarter((int)fex, (int)fey, sx, sy);
            p = beam_return_p(s_tab, a.rnd, a.hit_cut, expect, z, zstar);
        }
        lgp = beam_lg(s_tab, p, a.ln2);
    }
    if (dbg) { dbg[r] = first; dbg[a.R + r] = K; dbg[2 * a.R + r] = z; dbg[3 * a.R + r] = zstar; dbg[4 * a.R + r] = (int32_t)p; }
    return lgp;
}

// The scoring frame of both forms: the workgroup's BEAM_WG_POSES poses, a wave per BEAM_WAVE_POSES of them one after the other, a lane
// per ray through ray(pose, px, py, sx, sy, r, dbg) -> lg(p); per pose the wave's int64 sum, per workgroup the largest score and
// `path` (k_beam_final counts the workgroups with path 1).  Every thread of the workgroup calls it.
template <class Args, class Ray>
__device__ __forceinline__ void beam_score_poses(const Args& a, long long* s_max, int path, Ray ray)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p0 = blockIdx.x * BEAM_WG_POSES;
    long long best = BEAM_OFF;
    for (int q = 0; q < BEAM_WAVE_POSES; ++q) {
        const int pi = p0 + wave * BEAM_WAVE_POSES + q;
        if (pi >= a.n) break;                                           // (uniform over the wave)
        const float4 pose = a.poses[pi];
        float px, py; int sx, sy;
        long long s = BEAM_OFF;
        int32_t* dbg = (a.dbg && pi == 0) ? a.dbg : nullptr;
        if (beam_start(pose, a.f, &px, &py, &sx, &sy)) {
            s = 0;
            for (int r = lane; r < a.R; r += 64) s += ray(pose, px, py, sx, sy, r, dbg);
            for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
            best = s > best ? s : best;
        }
        if (lane == 0) a.scores[pi] = s;
    }
    if (lane == 0) s_max[wave] = best;
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < BEAM_THREADS / 64; ++k) best = s_max[k] > best ? s_max[k] : best;
        a.wg_max[blockIdx.x] = best;
        a.wg_path[blockIdx.x] = (uint8_t)path;
    }
}

__global__ __launch_bounds__(BEAM_THREADS) void k_beam_cast(beam_args a)
{
    extern __shared__ uint32_t s_mem[];
    __shared__ int s_box[4];
    __shared__ long long s_max[BEAM_THREADS / 64];
    uint32_t* s_tab = s_mem;
    int8_t* s_win = (int8_t*)(s_mem + BEAM_TABLE_WORDS);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int W = a.f.width, H = a.f.height;
    const int p0 = blockIdx.x * BEAM_WG_POSES;
    for (int i = tid; i < BEAM_TABLE_WORDS; i += BEAM_THREADS) s_tab[i] = a.tables[i];
    if (wave == 0) {                                                    // the bounding box of the start cells
        int x0 = INT_MAX, y0 = INT_MAX, x1 = INT_MIN, y1 = INT_MIN;
        if (lane < BEAM_WG_POSES && p0 + lane < a.n) {
            float px, py; int sx, sy;
            if (beam_start(a.poses[p0 + lane], a.f, &px, &py, &sx, &sy)) { x0 = x1 = sx; y0 = y1 = sy; }
        }
        for (int off = 32; off > 0; off >>= 1) {
            x0 = min(x0, __shfl_xor(x0, off, 64)); y0 = min(y0, __shfl_xor(y0, off, 64));
            x1 = max(x1, __shfl_xor(x1, off, 64)); y1 = max(y1, __shfl_xor(y1, off, 64));
        }
        if (lane == 0) { s_box[0] = x0; s_box[1] = y0; s_box[2] = x1; s_box[3] = y1; }
    }
    __syncthreads();
    beam_window win = {0, 0, 0, 0};
    bool staged = false;
    if (s_box[0] <= s_box[2] && a.stage) {                      // (the same for the whole workgroup)
        const int pad = a.reach + 2;
        win.x0 = max(s_box[0] - pad, 0) & ~3;
        win.y0 = max(s_box[1] - pad, 0);
        win.w = ((min(s_box[2] + pad, W - 1) - win.x0 + 1) + 3) & ~3;
        win.h = min(s_box[3] + pad, H - 1) - win.y0 + 1;
        staged = (long long)win.w * win.h <= (long long)a.window_bytes;
    }
    if (staged) {
        if ((W & 3) == 0) {                                             // rows of whole aligned words: x0 and W are multiples of 4
            const int ww = win.w >> 2, total = ww * win.h;
            for (int i = tid; i < total; i += BEAM_THREADS) {
                const int row = i / ww, c = i - row * ww;
                ((uint32_t*)s_win)[i] = *(const uint32_t*)(a.cells + (size_t)(win.y0 + row) * W + win.x0 + 4 * c);
            }
        } else {
            const int total = win.w * win.h;
            for (int i = tid; i < total; i += BEAM_THREADS) {
                const int row = i / win.w, c = i - row * win.w;
                const int gx = win.x0 + c;
                s_win[i] = gx < W ? a.cells[(size_t)(win.y0 + row) * W + gx] : (int8_t)0;
            }
        }
    }
    __syncthreads();
    beam_score_poses(a, s_max, staged ? 0 : 1, [&](const float4& pose, float px, float py, int sx, int sy, int r, int32_t* dbg) {
        return staged ? beam_ray<true>(a, s_tab, s_win, win, px, py, sx, sy, pose.z, r, dbg)
                      : beam_ray<false>(a, s_tab, s_win, win, px, py, sx, sy, pose.z, r, dbg);
    });
}

// ---------------------------------------------------------------------------------------------------------------- scoring by table
struct beam_lookup_args {
    const uint16_t* table; bl_frame f; int Hn;            // the range table and the frame it was built on
    const float* ranges; const float* thetas; int R;
    const float4* poses; int n;
    float max_range, kf, q; int hit_cut;                  // kf = (float)(Hn / (2 pi)); q = 4.0f * cells_per_meter
    uint32_t rnd, max_free, max_blocked; int ln2;
    const uint32_t* tables;
    long long* scores; long long* wg_max; uint8_t* wg_path;
    int32_t* dbg;                                         // null, or [4][R] of pose 0: h, z, zstar, p
};

// k_beam_cast's launch shape and records; z* of a ray is one uint16 of the row of its pose's start cell
__global__ __launch_bounds__(BEAM_THREADS) void k_beam_lookup(beam_lookup_args a)
{
    __shared__ uint32_t s_tab[BEAM_TABLE_WORDS];
    __shared__ long long s_max[BEAM_THREADS / 64];
    for (int i = threadIdx.x; i < BEAM_TABLE_WORDS; i += BEAM_THREADS) s_tab[i] = a.tables[i];
    __syncthreads();
    // path 1: nothing is staged, k_beam_final counts the workgroup with the direct ones
    beam_score_poses(a, s_max, 1, [&](const float4& pose, float, float, int sx, int sy, int r, int32_t* dbg) {
        const uint16_t* row = a.table + ((size_t)sy * a.f.width + sx) * a.Hn;
        const float range = a.ranges[r];
        const float ang = bl_wrap_to_pi(pose.z - a.thetas[r]);
        int h = -1, z = -1, zstar = -1, lgp = 0;
        uint32_t p = 0;
        if (__builtin_fabsf(ang) < __builtin_inff()) {
            h = beam_heading_index(ang, a.kf, a.Hn);
            const int t = row[h];
            const bool expect = t != BL_RANGETABLE_NONE;
            if (expect) zstar = t;
            if (range >= a.max_range) {
                p = expect ? a.max_blocked : a.max_free;
            } else {
                z = (int)(range * a.q);
                p = beam_return_p(s_tab, a.rnd, a.hit_cut, expect, z, zstar);
            }
            lgp = beam_lg(s_tab, p, a.ln2);
        }
        if (dbg) { dbg[r] = h; dbg[a.R + r] = z; dbg[2 * a.R + r] = zstar; dbg[3 * a.R + r] = (int32_t)p; }
        return lgp;
    });
}

// ---------------------------------------------------------------------------------------------------------------- scoring by leaps
struct beam_leap_args {
    const uint8_t* clear; bl_frame f;                     // the clearance grid and the frame it was built on
    const float* ranges; const float* thetas; int R;
    const float4* poses; int n;
    float max_range; int hit_cut;
    uint32_t rnd, max_free, max_blocked; int ln2;
    const uint32_t* tables;
    long long* scores; long long* wg_max; uint8_t* wg_path;
    int32_t* dbg;                                         // null, or [6][R] of pose 0: first, K, z, zstar, p, rounds
};

// k_beam_cast's launch shape and records; a ray's geometry, `has`, z, z*, p and lg are beam_ray's line for line (k_beam_cast is not
// edited for this form), and only the walk differs: entries of the clearance grid through L2, one per leap
__global__ __launch_bounds__(BEAM_THREADS) void k_beam_leap(beam_leap_args a)
{
    __shared__ uint32_t s_tab[BEAM_TABLE_WORDS];
    __shared__ long long s_max[BEAM_THREADS / 64];
    for (int i = threadIdx.x; i < BEAM_TABLE_WORDS; i += BEAM_THREADS) s_tab[i] = a.tables[i];
    __syncthreads();
    const int W = a.f.width, H = a.f.height;
    // path 1: nothing is staged, k_beam_final counts the workgroup with the direct ones
    beam_score_poses(a, s_max, 1, [&](const float4& pose, float px, float py, int sx, int sy, int r, int32_t* dbg) {
        const float range = a.ranges[r];
        const bool is_max = range >= a.max_range;
        const float ang = bl_wrap_to_pi(pose.z - a.thetas[r]);
        float sn, cs;
        bl_sincosf_cells(ang, &sn, &cs);
        const float fmx = a.max_range * cs * a.f.cpm + px, fmy = a.max_range * sn * a.f.cpm + py;
        const float fex = range * cs * a.f.cpm + px, fey = range * sn * a.f.cpm + py;
        bool has = __builtin_fabsf(fmx) < 0x1p30f && __builtin_fabsf(fmy) < 0x1p30f;
        if (!is_max) has = has && __builtin_fabsf(fex) < 0x1p30f && __builtin_fabsf(fey) < 0x1p30f;
        int first = -1, K = -1, z = -1, zstar = -1, rounds = -1, lgp = 0;
        uint32_t p = 0;
        if (has) {
            const beam_leap_hit hit = beam_first_hit_leap(sx, sy, (int)fmx, (int)fmy,
                [&](int x, int y) { return (int)a.clear[(size_t)y * W + x]; },
                [&](int x, int y) { return !((unsigned int)x < (unsigned int)W && (unsigned int)y < (unsigned int)H); });
            first = hit.first; K = hit.K; rounds = hit.rounds;
            const bool expect = first < K;
            if (expect) zstar = beam_quarter(hit.x, hit.y, sx, sy);
            if (is_max) {
                p = expect ? a.max_blocked : a.max_free;
            } else {
                z = beam_quarter((int)fex, (int)fey, sx, sy);
                p = beam_return_p(s_tab, a.rnd, a.hit_cut, expect, z, zstar);
            }
            lgp = beam_lg(s_tab, p, a.ln2);
        }
        if (dbg) {
            dbg[r] = first; dbg[a.R + r] = K; dbg[2 * a.R + r] = z; dbg[3 * a.R + r] = zstar; dbg[4 * a.R + r] = (int32_t)p; dbg[5 * a.R + r] = rounds;
        }
        return lgp;
    });
}

__global__ __launch_bounds__(1024) void k_beam_final(const long long* __restrict__ wg_max, const uint8_t* __restrict__ wg_path, int blocks, beam_state* st)
{
    __shared__ long long s_best[16];
    __shared__ int s_direct[16];
    long long best = BEAM_OFF;
    int direct = 0;
    for (int i = threadIdx.x; i < blocks; i += 1024) { best = wg_max[i] > best ? wg_max[i] : best; direct += wg_path[i]; }
    for (int off = 32; off > 0; off >>= 1) {
        const long long o = __shfl_xor(best, off, 64);
        best = o > best ? o : best;
        direct += __shfl_xor(direct, off, 64);
    }
    if ((threadIdx.x & 63) == 0) { s_best[threadIdx.x >> 6] = best; s_direct[threadIdx.x >> 6] = direct; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 16; ++k) { best = s_best[k] > best ? s_best[k] : best; direct += s_direct[k]; }
        st->smax = best; st->direct_wgs = direct; st->staged_wgs = blocks - direct;
    }
}

// rec: null, or the filter's record whose weight words take the units (a float4 per particle: x, y, theta, units as bits)
__global__ __launch_bounds__(256) void k_beam_units(const long long* __restrict__ scores, int n, const beam_state* __restrict__ st, long long span,
                                                    const uint32_t* __restrict__ U, uint32_t* __restrict__ units, float4* rec)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long s = scores[i];
    uint32_t u = 1u;
    if (s != BEAM_OFF) {
        const long long j = ((st->smax - s) * 256) / span;              // >= 0: floor
        u = U[j < 256 ? (int)j : 256];
    }
    units[i] = u;
    if (rec) ((uint32_t*)&rec[i])[3] = u;
}

// ---------------------------------------------------------------------------------------------------------------- host
struct bl_beam {
    bl_ctx* ctx;
    bool have_params;
    bl_beam_params_t params;
    uint32_t* h_tab;                                       // BEAM_TABLE_WORDS, of the parameters in force
    uint32_t* d_tab; uint32_t* d_U; beam_state* d_state;
    void* h_rays; size_t h_rays_cap; void* d_rays; size_t d_rays_cap;     // ranges | thetas of the used rays
    void* h_poses; size_t h_poses_cap; void* d_poses; size_t d_poses_cap;
    void* d_scores; size_t d_scores_cap; void* d_units; size_t d_units_cap;
    void* d_wg; size_t d_wg_cap;                           // per workgroup: the largest score (8 bytes each), then the path (1 byte each)
    void* d_dbg; size_t d_dbg_cap;
    int last_n;                                            // poses of the last scores / reweigh_pf (-1: none yet)
    int last_R;                                            // used rays of the last scan staged (-1: none yet)
    int window_bytes, stage;                               // stage: windows go to LDS when they fit (off: the grid is read directly)
    bool staged, timed;
    hipEvent_t ev_stage, ev_a, ev_b;
};

static long beam_round(double v) { return lround(v); }

// the tables of a parameter set that bl_beam_set_params accepted; rnd for a map of `reach` cells
static void beam_tables(const bl_beam_params_t& p, uint32_t* tab)
{
    const double s = (double)p.sigma_cells, lam = (double)p.lambda;
    for (int d = 0; d < 1024; ++d)
        tab[BEAM_HIT + d] = (uint32_t)beam_round(1073741824.0 * (double)p.z_hit * exp(-(((double)d / 4.0) * ((double)d / 4.0)) / (2.0 * s * s)));
    for (int c = 0; c < 1024; ++c) tab[BEAM_SHORT + c] = (uint32_t)beam_round(1073741824.0 * (double)p.z_short * lam * exp(-lam * (double)c));
    for (int i = 0; i < 256; ++i) tab[BEAM_LT + i] = (uint32_t)beam_round(65536.0 * log(1.0 + (double)i / 256.0));
}
static uint32_t beam_floor1(double v) { const long r = beam_round(v); return r < 1 ? 1u : (uint32_t)r; }
static uint32_t beam_rand(const bl_beam_params_t& p, int reach) { return beam_floor1(1073741824.0 * (double)p.z_rand / (double)reach); }
static uint32_t beam_max_free(const bl_beam_params_t& p) { return beam_floor1(1073741824.0 * (double)p.z_max); }
static uint32_t beam_max_blocked(const bl_beam_params_t& p) { return beam_floor1(1073741824.0 * (double)p.z_max * (double)p.blocked_factor); }

extern "C" void bl_beam_unit_table(uint32_t out[257])
{
    for (int j = 0; j <= 256; ++j) out[j] = beam_floor1(1048576.0 * pow(2.0, -20.0 * (double)j / 256.0));
}

extern "C" int bl_beam_create(bl_ctx* ctx, bl_beam** out)
{
    BL_CHECK_ARG(ctx != nullptr && out != nullptr);
    BL_HIP(hipSetDevice(ctx->device));
    bl_beam* b = new bl_beam();
    memset((void*)b, 0, sizeof(*b));
    b->ctx = ctx; b->last_n = -1; b->last_R = -1; b->window_bytes = BEAM_WINDOW_BYTES;
    b->h_tab = new uint32_t[BEAM_TABLE_WORDS];
    uint32_t U[257];
    bl_beam_unit_table(U);
    hipError_t e = hipMalloc((void**)&b->d_tab, BEAM_TABLE_WORDS * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&b->d_U, sizeof(U));
    if (e == hipSuccess) e = hipMalloc((void**)&b->d_state, sizeof(beam_state));
    if (e == hipSuccess) e = hipEventCreateWithFlags(&b->ev_stage, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreate(&b->ev_a);
    if (e == hipSuccess) e = hipEventCreate(&b->ev_b);
    if (e == hipSuccess) e = hipMemcpyAsync(b->d_U, U, sizeof(U), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);         // U lives on this stack
    if (e != hipSuccess) {
        bl_set_error("bl_beam_create: %s", hipGetErrorString(e));
        bl_beam_destroy(b);
        return BL_ERR_HIP;
    }
    *out = b;
    return BL_OK;
}

extern "C" void bl_beam_destroy(bl_beam* b)
{
    if (!b) return;
    (void)hipSetDevice(b->ctx->device);
    (void)hipStreamSynchronize(b->ctx->stream);
    void* dev[] = {b->d_tab, b->d_U, b->d_state, b->d_rays, b->d_poses, b->d_scores, b->d_units, b->d_wg, b->d_dbg};
    for (void* q : dev) if (q) (void)hipFree(q);
    if (b->h_rays) (void)hipHostFree(b->h_rays);
    if (b->h_poses) (void)hipHostFree(b->h_poses);
    if (b->ev_stage) (void)hipEventDestroy(b->ev_stage);
    if (b->ev_a) (void)hipEventDestroy(b->ev_a);
    if (b->ev_b) (void)hipEventDestroy(b->ev_b);
    delete[] b->h_tab;
    delete b;
}

extern "C" int bl_beam_set_params(bl_beam* b, const bl_beam_params_t* p)
{
    BL_CHECK_ARG(b != nullptr && p != nullptr);
    BL_CHECK_ARG(isfinite(p->max_range) && p->max_range > BEAM_MIN_RANGE);
    BL_CHECK_ARG(isfinite(p->sigma_cells) && p->sigma_cells > 0.0f);
    BL_CHECK_ARG(isfinite(p->z_hit) && isfinite(p->z_short) && isfinite(p->z_max) && isfinite(p->z_rand) && isfinite(p->lambda) && isfinite(p->blocked_factor));
    BL_CHECK_ARG(p->z_hit >= 0.0f && p->z_short >= 0.0f && p->z_max >= 0.0f && p->z_rand >= 0.0f && p->lambda >= 0.0f && p->blocked_factor >= 0.0f);
    BL_CHECK_ARG(p->occ_min >= 1 && p->occ_min <= 127);
    BL_CHECK_ARG(p->hit_cut >= 1 && p->hit_cut <= 1023);
    BL_CHECK_ARG(p->span > 0 && p->span <= (1ll << 40));
    BL_CHECK_ARG(p->ray_stride >= 1 && p->ray_stride <= 64);
    const double t30 = 1073741824.0;
    const double zh = t30 * (double)p->z_hit, zs = t30 * (double)p->z_short * (double)p->lambda, zr = t30 * (double)p->z_rand;
    const double zm = t30 * (double)p->z_max, zb = t30 * (double)p->z_max * (double)p->blocked_factor;
    BL_CHECK_ARG(zh <= 0x1p31 && zs <= 0x1p31 && zr <= 0x1p31 && zm <= 0x1p31 && zb <= 0x1p31);
    // no p may be 0: asked of the values before their max(1, .), Rand at the largest legal reach
    BL_CHECK_ARG(beam_round(zr / (double)BL_BEAM_MAX_REACH) >= 1 && beam_round(zm) >= 1 && beam_round(zb) >= 1);
    // no p may exceed 2^31 - 1: Hit[0] + Short[0] + Rand at a reach of one cell
    BL_CHECK_ARG(beam_round(zh) + beam_round(zs) + beam_round(zr) <= 2147483647l && beam_round(zm) <= 2147483647l && beam_round(zb) <= 2147483647l);
    bl_ctx* ctx = b->ctx;
    BL_HIP(hipSetDevice(ctx->device));
    BL_HIP(hipStreamSynchronize(ctx->stream));                          // h_tab may be on its way
    beam_tables(*p, b->h_tab);
    BL_HIP(hipMemcpyAsync(b->d_tab, b->h_tab, BEAM_TABLE_WORDS * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    b->params = *p;
    b->have_params = true;
    return BL_OK;
}

static int beam_need_params(const bl_beam* b)
{
    if (!b) { bl_set_error("bad argument: no beam model handle"); return BL_ERR_ARG; }
    if (!b->have_params) { bl_set_error("beam model has no parameters (bl_beam_set_params first)"); return BL_ERR_STATE; }
    return BL_OK;
}

static int beam_ln2() { return (int)beam_round(65536.0 * log(2.0)); }

extern "C" int bl_beam_tables(const bl_beam* b, float cells_per_meter, uint32_t* hit, uint32_t* short_, uint32_t* lt, uint32_t scalars[5])
{
    int rc = beam_need_params(b);
    if (rc) return rc;
    int reach = 0;
    rc = beam_reach(b->params.max_range, cells_per_meter, &reach);
    if (rc) return rc;
    if (hit) memcpy(hit, b->h_tab + BEAM_HIT, 1024 * sizeof(uint32_t));
    if (short_) memcpy(short_, b->h_tab + BEAM_SHORT, 1024 * sizeof(uint32_t));
    if (lt) memcpy(lt, b->h_tab + BEAM_LT, 256 * sizeof(uint32_t));
    if (scalars) {
        scalars[0] = beam_rand(b->params, reach); scalars[1] = beam_max_free(b->params); scalars[2] = beam_max_blocked(b->params);
        scalars[3] = (uint32_t)beam_ln2(); scalars[4] = (uint32_t)reach;
    }
    return BL_OK;
}

extern "C" int bl_beam_debug_set(bl_beam* b, int stage_windows, int window_bytes)
{
    BL_CHECK_ARG(b != nullptr && (stage_windows == 0 || stage_windows == 1));
    BL_CHECK_ARG(window_bytes == 0 || (window_bytes >= 16 && window_bytes <= BEAM_WINDOW_BYTES));
    b->stage = stage_windows;
    b->window_bytes = window_bytes ? window_bytes : BEAM_WINDOW_BYTES;
    return BL_OK;
}

// the used rays of `scan` to the device (ranges | thetas, R each); nothing is enqueued when the scan is refused
static int beam_stage_rays(bl_beam* b, const bl_lidar_t* scan, int* R_out)
{
    BL_CHECK_ARG(scan->num_ranges >= 0 && (scan->num_ranges == 0 || (scan->ranges != nullptr && scan->thetas != nullptr)));
    const int stride = b->params.ray_stride;
    int kept = 0;
    for (int i = 0; i < scan->num_ranges; ++i) kept += (isfinite(scan->ranges[i]) && scan->ranges[i] > BEAM_MIN_RANGE) ? 1 : 0;
    const int R = (kept + stride - 1) / stride;
    BL_CHECK_ARG(R <= BL_BEAM_MAX_RAYS);
    *R_out = R;
    b->last_R = R;
    bl_ctx* ctx = b->ctx;
    const size_t bytes = 2 * (size_t)(R > 0 ? R : 1) * sizeof(float);
    if (b->staged) { BL_HIP(hipEventSynchronize(b->ev_stage)); b->staged = false; }   // the pinned blocks may still be on their way
    int rc = bl_grow(&b->h_rays, &b->h_rays_cap, bytes, true, ctx);
    if (!rc) rc = bl_grow(&b->d_rays, &b->d_rays_cap, bytes, false, ctx);
    if (rc) return rc;
    float* h = (float*)b->h_rays;
    int seen = 0, r = 0;
    for (int i = 0; i < scan->num_ranges; ++i) {
        if (!(isfinite(scan->ranges[i]) && scan->ranges[i] > BEAM_MIN_RANGE)) continue;
        if (seen++ % stride == 0) { h[r] = scan->ranges[i]; h[R + r] = scan->thetas[i]; ++r; }
    }
    if (R > 0) {
        BL_HIP(hipMemcpyAsync(b->d_rays, b->h_rays, 2 * (size_t)R * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
        BL_HIP(hipEventRecord(b->ev_stage, ctx->stream));              // (recorded again behind the poses' copy, when there is one)
        b->staged = true;
    }
    return BL_OK;
}

// where the expected ranges come from: cast against `map`, or (map null) looked up in the table `v`, or (leap) found by leaps over the
// clearance grid `c`; reach: the beam model's in cells on that map's, table's or grid's frame (a table's own is checked to equal it)
struct beam_form { const bl_grid* map; int reach; bl_rangetable_view v; bool leap; bl_clearance_view c; };

// the fields the three kernels' argument structs share, for a map or table of `reach` cells
template <class Args>
static void beam_fill_args(Args& a, const bl_beam* b, int reach, int R, const float4* poses, int n, int blocks, int32_t* dbg)
{
    const bl_beam_params_t& p = b->params;
    a.ranges = (const float*)b->d_rays; a.thetas = (const float*)b->d_rays + R; a.R = R;
    a.poses = poses; a.n = n;
    a.max_range = p.max_range; a.hit_cut = p.hit_cut;
    a.rnd = beam_rand(p, reach); a.max_free = beam_max_free(p); a.max_blocked = beam_max_blocked(p);
    a.ln2 = beam_ln2();
    a.tables = b->d_tab;
    a.scores = (long long*)b->d_scores; a.wg_max = (long long*)b->d_wg; a.wg_path = (uint8_t*)b->d_wg + (size_t)blocks * 8;
    a.dbg = dbg;
}

// The launches for n poses at `poses` (device): the form's scoring kernel, k_beam_final and -- not for a debug launch, which leaves
// the last call's units and count alone -- k_beam_units, then the closing event.  rec: the filter's record for k_beam_units, or
// null; dbg: the form's planes ([5][R] cast, [4][R] table, [6][R] leaps) of pose 0, or null
static int beam_launch(bl_beam* b, const beam_form& fm, int R, const float4* poses, int n, float4* rec, int32_t* dbg)
{
    bl_ctx* ctx = b->ctx;
    const int blocks = (n + BEAM_WG_POSES - 1) / BEAM_WG_POSES;
    int rc = bl_grow(&b->d_scores, &b->d_scores_cap, (size_t)n * 8, false, ctx);
    if (!rc) rc = bl_grow(&b->d_units, &b->d_units_cap, (size_t)n * 4, false, ctx);
    if (!rc) rc = bl_grow(&b->d_wg, &b->d_wg_cap, (size_t)blocks * 9, false, ctx);
    if (rc) return rc;
    BL_HIP(hipEventRecord(b->ev_stage, ctx->stream));                   // the pinned blocks have left once this is reached
    BL_HIP(hipEventRecord(b->ev_a, ctx->stream));
    if (fm.leap) {
        beam_leap_args a;
        beam_fill_args(a, b, fm.reach, R, poses, n, blocks, dbg);
        a.clear = fm.c.d_grid; a.f = fm.c.frame;
        hipLaunchKernelGGL(k_beam_leap, dim3((unsigned int)blocks), dim3(BEAM_THREADS), 0, ctx->stream, a);
    } else if (fm.map) {
        beam_args a;
        beam_fill_args(a, b, fm.reach, R, poses, n, blocks, dbg);
        a.cells = fm.map->cells; a.f = fm.map->frame;
        a.occ_min = b->params.occ_min; a.reach = fm.reach;
        a.window_bytes = b->window_bytes; a.stage = b->stage;
        hipLaunchKernelGGL(k_beam_cast, dim3((unsigned int)blocks), dim3(BEAM_THREADS),
                           BEAM_TABLE_WORDS * sizeof(uint32_t) + (b->stage ? (size_t)b->window_bytes : 0), ctx->stream, a);
    } else {
        beam_lookup_args a;
        beam_fill_args(a, b, fm.reach, R, poses, n, blocks, dbg);
        a.table = fm.v.d_table; a.f = fm.v.frame; a.Hn = fm.v.headings;
        a.kf = (float)((double)fm.v.headings / (2.0 * BL_PI)); a.q = 4.0f * fm.v.frame.cpm;
        hipLaunchKernelGGL(k_beam_lookup, dim3((unsigned int)blocks), dim3(BEAM_THREADS), 0, ctx->stream, a);
    }
    hipLaunchKernelGGL(k_beam_final, dim3(1), dim3(1024), 0, ctx->stream, (const long long*)b->d_wg, (const uint8_t*)b->d_wg + (size_t)blocks * 8, blocks,
                       b->d_state);
    if (!dbg)
        hipLaunchKernelGGL(k_beam_units, dim3((unsigned int)((n + 255) / 256)), dim3(256), 0, ctx->stream, (const long long*)b->d_scores, n,
                           (const beam_state*)b->d_state, (long long)b->params.span, (const uint32_t*)b->d_U, (uint32_t*)b->d_units, rec);
    BL_HIP(hipGetLastError());
    BL_HIP(hipEventRecord(b->ev_b, ctx->stream));
    b->staged = true; b->timed = true;
    if (!dbg) b->last_n = n;
    return BL_OK;
}

static int beam_check_map(const bl_beam* b, const bl_grid* map, const bl_lidar_t* scan, beam_form* fm)
{
    BL_CHECK_ARG(map != nullptr && scan != nullptr && map->ctx == b->ctx);
    fm->map = map; fm->leap = false;
    return beam_reach(b->params.max_range, map->frame.cpm, &fm->reach);
}

void bl_beam_view_host(const bl_beam* b, bl_beam_view* out)
{
    out->ctx = b->ctx; out->have_params = b->have_params; out->max_range = b->params.max_range; out->occ_min = b->params.occ_min;
}

// the table's view, once it is known to be built on this ctx with the reach and occ_min the parameters in force give
static int beam_check_table(const bl_beam* b, const bl_rangetable* rt, const bl_lidar_t* scan, beam_form* fm)
{
    BL_CHECK_ARG(rt != nullptr && scan != nullptr);
    bl_rangetable_view* v = &fm->v;
    fm->map = nullptr; fm->leap = false;
    bl_rangetable_view_host(rt, v);
    BL_CHECK_ARG(v->ctx == b->ctx);
    if (!v->built) { bl_set_error("range table not built (bl_rangetable_build first)"); return BL_ERR_STATE; }
    if (b->params.occ_min != v->occ_min) {
        bl_set_error("range table built with occ_min %d, the beam model has %d", v->occ_min, b->params.occ_min);
        return BL_ERR_STATE;
    }
    if (beam_reach(b->params.max_range, v->frame.cpm, &fm->reach) != BL_OK || fm->reach != v->reach) {
        bl_set_error("range table built with a reach of %d cells, the beam model's is another", v->reach);
        return BL_ERR_STATE;
    }
    return BL_OK;
}

// the grid's view, once it is known to be built on this ctx with the occ_min the parameters in force give
static int beam_check_clearance(const bl_beam* b, const bl_clearance* cl, const bl_lidar_t* scan, beam_form* fm)
{
    BL_CHECK_ARG(cl != nullptr && scan != nullptr);
    bl_clearance_view* c = &fm->c;
    fm->map = nullptr; fm->leap = true;
    bl_clearance_view_host(cl, c);
    BL_CHECK_ARG(c->ctx == b->ctx);
    if (!c->built) { bl_set_error("clearance grid not built (bl_clearance_build first)"); return BL_ERR_STATE; }
    if (b->params.occ_min != c->occ_min) {
        bl_set_error("clearance grid built with occ_min %d, the beam model has %d", c->occ_min, b->params.occ_min);
        return BL_ERR_STATE;
    }
    return beam_reach(b->params.max_range, c->frame.cpm, &fm->reach);
}

// n host poses staged as the kernels read them
static int beam_stage_poses(bl_beam* b, const bl_pose_xyt_t* poses, int n)
{
    bl_ctx* ctx = b->ctx;
    int rc = bl_grow(&b->h_poses, &b->h_poses_cap, (size_t)n * sizeof(float4), true, ctx);
    if (!rc) rc = bl_grow(&b->d_poses, &b->d_poses_cap, (size_t)n * sizeof(float4), false, ctx);
    if (rc) return rc;
    float4* h = (float4*)b->h_poses;
    for (int i = 0; i < n; ++i) h[i] = make_float4(poses[i].x, poses[i].y, poses[i].theta, 0.0f);
    BL_HIP(hipMemcpyAsync(b->d_poses, b->h_poses, (size_t)n * sizeof(float4), hipMemcpyHostToDevice, ctx->stream));
    return BL_OK;
}

// The three calls of either form, behind beam_need_params and the form's check.
static int beam_scores(bl_beam* b, const beam_form& fm, const bl_lidar_t* scan, const bl_pose_xyt_t* poses, int n, int64_t* out_scores)
{
    BL_CHECK_ARG(n >= 0 && (n == 0 || (poses != nullptr && out_scores != nullptr)));
    bl_ctx* ctx = b->ctx;
    BL_HIP(hipSetDevice(ctx->device));
    int R = 0;
    int rc = beam_stage_rays(b, scan, &R);
    if (rc) return rc;
    if (n == 0) { b->last_n = 0; return BL_OK; }
    rc = beam_stage_poses(b, poses, n);
    if (!rc) rc = beam_launch(b, fm, R, (const float4*)b->d_poses, n, nullptr, nullptr);
    if (rc) return rc;
    BL_HIP(hipMemcpyAsync(out_scores, b->d_scores, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));   // the one read-back
    BL_HIP(hipStreamSynchronize(ctx->stream));
    return BL_OK;
}

// outs: the form's `planes` planes of R words each (5 cast, 4 table, 6 leaps), any of them null
static int beam_debug(bl_beam* b, const beam_form& fm, const bl_lidar_t* scan, const bl_pose_xyt_t* pose, void* const* outs, int planes)
{
    BL_CHECK_ARG(pose != nullptr);
    bl_ctx* ctx = b->ctx;
    BL_HIP(hipSetDevice(ctx->device));
    int R = 0;
    int rc = beam_stage_rays(b, scan, &R);
    if (rc) return rc;
    if (R == 0) return BL_OK;
    const size_t bytes = (size_t)planes * R * 4;
    rc = bl_grow(&b->d_dbg, &b->d_dbg_cap, bytes, false, ctx);
    if (!rc) rc = beam_stage_poses(b, pose, 1);
    if (rc) return rc;
    BL_HIP(hipMemsetAsync(b->d_dbg, 0, bytes, ctx->stream));            // (an off-grid pose writes nothing)
    rc = beam_launch(b, fm, R, (const float4*)b->d_poses, 1, nullptr, (int32_t*)b->d_dbg);
    if (rc) return rc;
    for (int k = 0; k < planes; ++k)
        if (outs[k]) BL_HIP(hipMemcpyAsync(outs[k], (const int32_t*)b->d_dbg + (size_t)k * R, (size_t)R * 4, hipMemcpyDeviceToHost, ctx->stream));
    BL_HIP(hipStreamSynchronize(ctx->stream));
    return BL_OK;
}

struct beam_install { bl_beam* b; beam_form fm; int R; };
static int beam_write_units(void* user, float4* rec, int n)
{
    const beam_install* q = (const beam_install*)user;
    return beam_launch(q->b, q->fm, q->R, rec, n, rec, nullptr);
}

// q: b and the checked form
static int beam_reweigh(beam_install& q, bl_pf* pf, const bl_lidar_t* scan, bl_pose_xyt_t* out_pose)
{
    bl_beam* b = q.b;
    BL_CHECK_ARG(pf != nullptr);
    int rc = bl_pf_install_units(pf, b->ctx, nullptr, nullptr, nullptr);   // the filter's state and ctx, before anything is enqueued
    if (rc) return rc;
    BL_HIP(hipSetDevice(b->ctx->device));
    rc = beam_stage_rays(b, scan, &q.R);
    if (rc) return rc;
    return bl_pf_install_units(pf, b->ctx, beam_write_units, &q, out_pose);
}

extern "C" int bl_beam_scores(bl_beam* b, const bl_grid* map, const bl_lidar_t* scan, const bl_pose_xyt_t* poses, int n, int64_t* out_scores)
{
    int rc = beam_need_params(b);
    if (rc) return rc;
    beam_form fm;
    rc = beam_check_map(b, map, scan, &fm);
    return rc ? rc : beam_scores(b, fm, scan, poses, n, out_scores);
}

extern "C" int bl_rangetable_scores(bl_beam* b, const bl_rangetable* rt, const bl_lidar_t* scan, const bl_pose_xyt_t* poses, int n, int64_t* out_scores)
{
    int rc = beam_need_params(b);
    if (rc) return rc;
    beam_form fm;
    rc = beam_check_table(b, rt, scan, &fm);
    return rc ? rc : beam_scores(b, fm, scan, poses, n, out_scores);
}

extern "C" int bl_beam_debug_cast(bl_beam* b, const bl_grid* map, const bl_lidar_t* scan, const bl_pose_xyt_t* pose, int32_t* out_first,
                                  int32_t* out_K, int32_t* out_z, int32_t* out_zstar, uint32_t* out_p)
{
    int rc = beam_need_params(b);
    if (rc) return rc;
    beam_form fm;
    rc = beam_check_map(b, map, scan, &fm);
    void* const outs[5] = {out_first, out_K, out_z, out_zstar, out_p};
    return rc ? rc : beam_debug(b, fm, scan, pose, outs, 5);
}

extern "C" int bl_rangetable_debug_lookup(bl_beam* b, const bl_rangetable* rt, const bl_lidar_t* scan, const bl_pose_xyt_t* pose, int32_t* out_h,
                                    int32_t* out_z, int32_t* out_zstar, uint32_t* out_p)
{
    int rc = beam_need_params(b);
    if (rc) return rc;
    beam_form fm;
    rc = beam_check_table(b, rt, scan, &fm);
    void* const outs[4] = {out_h, out_z, out_zstar, out_p};
    return rc ? rc : beam_debug(b, fm, scan, pose, outs, 4);
}

extern "C" int bl_beam_reweigh_pf(bl_beam* b, bl_pf* pf, const bl_grid* map, const bl_lidar_t* scan, bl_pose_xyt_t* out_pose)
{
    int rc = beam_need_params(b);
    if (rc) return rc;
    beam_install q;
    q.b = b;
    rc = beam_check_map(b, map, scan, &q.fm);
    return rc ? rc : beam_reweigh(q, pf, scan, out_pose);
}

extern "C" int bl_rangetable_reweigh_pf(bl_beam* b, bl_pf* pf, const bl_rangetable* rt, const bl_lidar_t* scan, bl_pose_xyt_t* out_pose)
{
    int rc = beam_need_params(b);
    if (rc) return rc;
    beam_install q;
    q.b = b;
    rc = beam_check_table(b, rt, scan, &q.fm);
    return rc ? rc : beam_reweigh(q, pf, scan, out_pose);
}

extern "C" int bl_clearance_scores(bl_beam* b, const bl_clearance* cl, const bl_lidar_t* scan, const bl_pose_xyt_t* poses, int n, int64_t* out_scores)
{
    int rc = beam_need_params(b);
    if (rc) return rc;
    beam_form fm;
    rc = beam_check_clearance(b, cl, scan, &fm);
    return rc ? rc : beam_scores(b, fm, scan, poses, n, out_scores);
}

extern "C" int bl_clearance_debug_cast(bl_beam* b, const bl_clearance* cl, const bl_lidar_t* scan, const bl_pose_xyt_t* pose, int32_t* out_first,
                                       int32_t* out_K, int32_t* out_z, int32_t* out_zstar, uint32_t* out_p, int32_t* out_rounds)
{
    int rc = beam_need_params(b);
    if (rc) return rc;
    beam_form fm;
    rc = beam_check_clearance(b, cl, scan, &fm);
    void* const outs[6] = {out_first, out_K, out_z, out_zstar, out_p, out_rounds};
    return rc ? rc : beam_debug(b, fm, scan, pose, outs, 6);
}

extern "C" int bl_clearance_reweigh_pf(bl_beam* b, bl_pf* pf, const bl_clearance* cl, const bl_lidar_t* scan, bl_pose_xyt_t* out_pose)
{
    int rc = beam_need_params(b);
    if (rc) return rc;
    beam_install q;
    q.b = b;
    rc = beam_check_clearance(b, cl, scan, &q.fm);
    return rc ? rc : beam_reweigh(q, pf, scan, out_pose);
}

extern "C" int bl_beam_units(bl_beam* b, uint32_t* out_units, int n)
{
    BL_CHECK_ARG(b != nullptr && n >= 0 && (n == 0 || out_units != nullptr));
    if (b->last_n < 0) { bl_set_error("bl_beam_units: no bl_beam_scores or bl_beam_reweigh_pf yet"); return BL_ERR_STATE; }
    BL_CHECK_ARG(n == b->last_n);
    if (n == 0) return BL_OK;
    BL_HIP(hipSetDevice(b->ctx->device));
    BL_HIP(hipMemcpyAsync(out_units, b->d_units, (size_t)n * 4, hipMemcpyDeviceToHost, b->ctx->stream));
    BL_HIP(hipStreamSynchronize(b->ctx->stream));
    return BL_OK;
}

extern "C" int bl_beam_last_rays(const bl_beam* b) { return b ? b->last_R : -1; }

extern "C" int bl_beam_debug_path(bl_beam* b)
{
    if (!b || !b->timed) return -1;
    beam_state st;
    if (hipSetDevice(b->ctx->device) != hipSuccess) return -1;
    if (hipMemcpyAsync(&st, b->d_state, sizeof(st), hipMemcpyDeviceToHost, b->ctx->stream) != hipSuccess) return -1;
    if (hipStreamSynchronize(b->ctx->stream) != hipSuccess) return -1;
    return st.direct_wgs == 0 ? 0 : st.staged_wgs == 0 ? 1 : 2;
}

extern "C" int bl_beam_last_device_ms(const bl_beam* b, float* ms)
{
    BL_CHECK_ARG(b != nullptr && ms != nullptr);
    if (!b->timed) { bl_set_error("bl_beam_last_device_ms: no kernels launched yet"); return BL_ERR_STATE; }
    BL_HIP(hipEventSynchronize(b->ev_b));
    BL_HIP(hipEventElapsedTime(ms, b->ev_a, b->ev_b));
    return BL_OK;
}
