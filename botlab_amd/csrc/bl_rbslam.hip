// bl_rbslam.hip -- Rao-Blackwellized grid SLAM (FastSLAM on grids): P particles, each with a pose, a parent pose, a cumulative
// score and its OWN W x H int8 map.  The definition is in include/botlab_hip.h ("bl_rbslam"); tests/rb_slam_model.py is the same
// definition over the reference's per-particle entry points, and the two agree bit for bit.
//
// One moved update is five stream-ordered launches, no host loop over particles and no host round trip in between:
//   k_rb_plan    one workgroup: S and Q of the units the last weighing left, the exact "resampling is due" test, and -- when due --
//                the integer prefix, the low-variance search, the particle -> slot table and the list of map copies
//   k_rb_copy    every map copy of the resampling in ONE launch, 16-byte vector loads and stores
//   k_rb_weigh   ActionModel::applyAction and SensorModel::likelihood of every particle against its own map: a wave per particle,
//                the rays across its lanes, the <= 3 cells of scoreRay gathered from the particle's map through L2
//   k_rb_reduce  one workgroup: units, S, Q and the best particle
//   (k_rb_match  only with scan matching on, and then k_rb_weigh in its form without the action: bl_rbslam_match.h)
//   k_rb_map     Mapping::updateMap of all P maps: a workgroup per (particle, window tile), hit and miss counts of the tile in an
//                LDS window of uint16 counters, one owner thread per cell
// The motion and sensor model, the initial draw and the low-variance draw are bl_pfmodel.h's, which the filter (bl_mcl.hip) shares; the
// mapper's ray cells and walk are bl_mapray_dev.h's.
#include <stdio.h>
#include <string.h>

#include "bl_internal.h"
#include "bl_mapray_dev.h"
#include "bl_pfmodel.h"

#define RB_MAX_PARTICLES 4096
#define RB_PLAN_THREADS 1024
#define RB_PLAN_ITEMS (RB_MAX_PARTICLES / RB_PLAN_THREADS)
#define RB_WEIGH_THREADS 256
#define RB_MAP_THREADS 512
#define RB_MAP_COUNTERS (20 * 1024)          // uint16 counters of one window tile: 40 KB of LDS, so that three to four workgroups share a CU
#define RB_MAP_TILE_W 256                    // widest tile; a window up to this wide is cut into horizontal strips only
#define RB_MAP_SEG 16                        // cells per walk segment
#define RB_MAP_SEG_RAYS 512                  // rays whose cells and segment table are kept in LDS (longer scans: a serial walk per ray)
#define RB_MAP_MAX_RAYS 8192
#define RB_COPY_THREADS 256
#define RB_COPY_VEC 4                        // int4 per thread and item: 16 KB per workgroup item
#define RB_SCORE_SAT (1ll << 33)             // BL_RBSLAM_SCORE_MAX (botlab_hip.h)

struct rb_state {
    unsigned long long S, Q_lo, Q_hi;        // over the units of the last weighing
    int weighed, resampled, ncopy, best;
    bl_pose_xyt_t best_pose;
};

struct bl_rbslam {
    bl_ctx* ctx;
    int P;
    bl_frame frame;
    size_t stride;                           // bytes between two maps (W * H rounded up to 16)
    float max_laser; int hit, miss;
    uint32_t num, den;
    int8_t* maps;                            // P slots
    int8_t* staging;                         // one map: upload / download
    float4* pose[2]; int cur;                // (x, y, theta, -)
    float4* parent;
    long long* cum;
    unsigned long long* units;
    int32_t* like; int32_t* idx; int32_t* slot; int2* copies;
    float* d_noise;
    rb_state* state;
    rb_state* h_state;                       // pinned
    bl_particle_t* d_export;
    int64_t pose_utime, parent_utime;
    bl_action_state action;                  // ActionModel::updateAction (bl_pfmodel.h)
    uint64_t noise_seed; uint32_t step;
    bool initialized, map_latched;
    // scan matching (step 3b, bl_rbslam_match.h); the buffers exist once it has been switched on
    bool match_on, match_done;
    bl_rbslam_match_params_t match;
    float* match_rays;                       // ranges[RBM_MAX_RAYS] | thetas[RBM_MAX_RAYS]: the valid rays of the scan
    float* h_match_rays;                     // pinned, the same layout
    int32_t* match_out;                      // 7 x P
    int match_path;
};

// ---------------------------------------------------------------- device helpers
template <class T>
__device__ __forceinline__ T rb_wave_incl_scan(T v, int lane)
{
    for (int off = 1; off < 64; off <<= 1) {
        T t = __shfl_up(v, off, 64);
        if (lane >= off) v += t;
    }
    return v;
}

// exclusive scan over the workgroup's threads in thread order; *total: the sum.  s_w: one slot per wave.  Ends with a barrier.
template <class T>
__device__ __forceinline__ T rb_block_excl_scan(T v, T* s_w, T* total)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    const T incl = rb_wave_incl_scan(v, lane);
    __syncthreads();                                            // s_w may still be read from the previous use
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    T base = 0, tot = 0;
    for (int w = 0; w < nw; ++w) { const T x = s_w[w]; if (w < wave) base += x; tot += x; }
    *total = tot;
    return base + incl - v;
}

// S and Q = sum u^2 of the workgroup's units.  u < 2^43 (RB_SCORE_SAT): with u = a 2^22 + b, a < 2^21, the three sums of a^2, a b and
// b^2 over <= 4096 particles stay below 2^56 and are plain 64-bit reductions; one thread assembles the 128-bit Q.
struct rb_sums { unsigned long long S, A2, AB, B2; };
__device__ __forceinline__ void rb_sums_add(rb_sums& s, unsigned long long u)
{
    const unsigned long long a = u >> 22, b = u & ((1ull << 22) - 1ull);
    s.S += u; s.A2 += a * a; s.AB += a * b; s.B2 += b * b;
}
__device__ __forceinline__ unsigned __int128 rb_q_of(const rb_sums& s)
{
    return ((unsigned __int128)s.A2 << 44) + ((unsigned __int128)s.AB << 23) + (unsigned __int128)s.B2;
}
__device__ __forceinline__ unsigned long long rb_wave_sum_u64(unsigned long long v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
// every thread gets the workgroup's sums.  s_r: 4 slots per wave.
__device__ __forceinline__ rb_sums rb_block_sums(rb_sums s, unsigned long long* s_r)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    s.S = rb_wave_sum_u64(s.S); s.A2 = rb_wave_sum_u64(s.A2); s.AB = rb_wave_sum_u64(s.AB); s.B2 = rb_wave_sum_u64(s.B2);
    __syncthreads();
    if (lane == 0) { s_r[4 * wave] = s.S; s_r[4 * wave + 1] = s.A2; s_r[4 * wave + 2] = s.AB; s_r[4 * wave + 3] = s.B2; }
    __syncthreads();
    rb_sums t = {0, 0, 0, 0};
    for (int w = 0; w < nw; ++w) { t.S += s_r[4 * w]; t.A2 += s_r[4 * w + 1]; t.AB += s_r[4 * w + 2]; t.B2 += s_r[4 * w + 3]; }
    return t;
}

// ---------------------------------------------------------------- plan: due?, prefix, search, slot table, copy list
struct rb_plan_args {
    int P;
    const unsigned long long* units;
    rb_state* state;
    int32_t* idx; int32_t* slot; int2* copies; long long* cum;
    double r, M_inv;                         // particle_filter.cpp:89-92 with M = P
    uint32_t num, den;
};

__global__ __launch_bounds__(RB_PLAN_THREADS) void k_rb_plan(rb_plan_args a)
{
    __shared__ unsigned long long s_pre[RB_MAX_PARTICLES];      // inclusive prefix; afterwards: has[] and dead[] (int each)
    __shared__ unsigned short s_idx[RB_MAX_PARTICLES];
    __shared__ unsigned long long s_w64[RB_PLAN_THREADS / 64 * 4];
    __shared__ int s_w32[RB_PLAN_THREADS / 64];
    __shared__ int s_due;
    const int tid = threadIdx.x, P = a.P;
    const int i0 = tid * RB_PLAN_ITEMS;                          // this thread's particles: i0 .. i0 + 3
    unsigned long long u[RB_PLAN_ITEMS];
    rb_sums sums = {0, 0, 0, 0};
    unsigned long long mine = 0;
#pragma unroll
    for (int k = 0; k < RB_PLAN_ITEMS; ++k) {
        u[k] = i0 + k < P ? a.units[i0 + k] : 0ull;
        rb_sums_add(sums, u[k]);
        mine += u[k];
    }
    unsigned long long S;
    unsigned long long run = rb_block_excl_scan(mine, s_w64, &S);
#pragma unroll
    for (int k = 0; k < RB_PLAN_ITEMS; ++k) { run += u[k]; if (i0 + k < P) s_pre[i0 + k] = run; }
    const rb_sums tot = rb_block_sums(sums, s_w64);
    if (tid == 0) {
        // due iff den S^2 <= num P Q, exactly: S < 2^55 and Q < 2^98, num, den < 2^16 (botlab_hip.h)
        const unsigned __int128 lhs = (unsigned __int128)S * S * a.den;
        const unsigned __int128 rhs = rb_q_of(tot) * ((unsigned long long)a.num * (unsigned long long)P);
        const int due = a.state->weighed && lhs <= rhs;
        s_due = due;
        a.state->resampled = due;
        if (!due) a.state->ncopy = 0;
    }
    __syncthreads();
    if (!s_due) {
#pragma unroll
        for (int k = 0; k < RB_PLAN_ITEMS; ++k) if (i0 + k < P) a.idx[i0 + k] = i0 + k;
        return;
    }
    // ---- low-variance search by the integer-prefix rule (bl_pfmodel.h): the first i whose prefix reaches T_m, clamped to P - 1
    const double Sd = (double)S;
    int src[RB_PLAN_ITEMS];
#pragma unroll
    for (int k = 0; k < RB_PLAN_ITEMS; ++k) {
        const int m = i0 + k;
        src[k] = 0;
        if (m < P) {
            const double T = bl_resample_target(a.r, m, a.M_inv, Sd);
            int lo = 0, hi = P - 1;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (bl_resample_reaches(T, s_pre[mid])) hi = mid; else lo = mid + 1; }
            src[k] = lo;
            s_idx[m] = (unsigned short)lo;
        }
    }
    __syncthreads();                                            // the prefix is dead from here on
    int* s_has = (int*)s_pre;
    int* s_dead = s_has + RB_MAX_PARTICLES;
#pragma unroll
    for (int k = 0; k < RB_PLAN_ITEMS; ++k) if (i0 + k < P) s_has[i0 + k] = 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < RB_PLAN_ITEMS; ++k) if (i0 + k < P) s_has[src[k]] = 1;
    __syncthreads();
    // the sources ascend with m: the first child of a source is the one whose predecessor has another source.  It keeps the slot;
    // the k-th other child (in order of m) takes the slot of the k-th particle that died (in order of index).
    bool extra[RB_PLAN_ITEMS];
    int n_extra = 0, n_dead = 0;
#pragma unroll
    for (int k = 0; k < RB_PLAN_ITEMS; ++k) {
        const int m = i0 + k;
        extra[k] = m < P && m > 0 && s_idx[m - 1] == src[k];
        n_extra += extra[k] ? 1 : 0;
        n_dead += (m < P && !s_has[m]) ? 1 : 0;
    }
    int total_extra, total_dead;
    int rank_extra = rb_block_excl_scan(n_extra, s_w32, &total_extra);
    int rank_dead = rb_block_excl_scan(n_dead, s_w32, &total_dead);
#pragma unroll
    for (int k = 0; k < RB_PLAN_ITEMS; ++k) if (i0 + k < P && !s_has[i0 + k]) s_dead[rank_dead++] = i0 + k;
    __syncthreads();
    int new_slot[RB_PLAN_ITEMS];
#pragma unroll
    for (int k = 0; k < RB_PLAN_ITEMS; ++k) {
        const int m = i0 + k;
        new_slot[k] = 0;
        if (m < P) {
            const int from = a.slot[src[k]];
            new_slot[k] = from;
            if (extra[k] && rank_extra < total_dead) {           // (total_extra == total_dead: P children, one first child per live source)
                const int to = a.slot[s_dead[rank_extra]];
                a.copies[rank_extra] = make_int2(from, to);
                new_slot[k] = to;
                ++rank_extra;
            }
        }
    }
    __syncthreads();                                            // every read of the old slot table is done
#pragma unroll
    for (int k = 0; k < RB_PLAN_ITEMS; ++k) {
        const int m = i0 + k;
        if (m < P) { a.slot[m] = new_slot[k]; a.idx[m] = src[k]; a.cum[m] = 0; }
    }
    if (tid == 0) a.state->ncopy = total_extra < total_dead ? total_extra : total_dead;
}

// ---------------------------------------------------------------- the map copies of a resampling, one launch
__global__ __launch_bounds__(RB_COPY_THREADS) void k_rb_copy(int8_t* maps, size_t stride, const int2* __restrict__ copies,
                                                             const rb_state* __restrict__ state, int chunks)
{
    const int ncopy = state->ncopy;
    const size_t n16 = stride / 16;
    const long long items = (long long)ncopy * chunks;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const int c = (int)(it / chunks), ch = (int)(it - (long long)c * chunks);
        const int2 sd = copies[c];
        const int4* s4 = (const int4*)(maps + (size_t)sd.x * stride);
        int4* d4 = (int4*)(maps + (size_t)sd.y * stride);
        const size_t base = (size_t)ch * RB_COPY_THREADS * RB_COPY_VEC + threadIdx.x;
        int4 v[RB_COPY_VEC];
#pragma unroll
        for (int q = 0; q < RB_COPY_VEC; ++q) { const size_t i = base + (size_t)q * RB_COPY_THREADS; if (i < n16) v[q] = s4[i]; }
#pragma unroll
        for (int q = 0; q < RB_COPY_VEC; ++q) { const size_t i = base + (size_t)q * RB_COPY_THREADS; if (i < n16) d4[i] = v[q]; }
    }
}

// one map <-> a flat buffer, by slot; which < 0: the best particle's
__global__ __launch_bounds__(RB_COPY_THREADS) void k_rb_map_io(int8_t* maps, size_t stride, const int32_t* __restrict__ slot,
                                                               const rb_state* __restrict__ state, int which, int8_t* flat, size_t n, int to_maps)
{
    const int p = which < 0 ? state->best : which;
    int8_t* m = maps + (size_t)slot[p] * stride;
    const size_t n16 = ((((size_t)flat) & 15) == 0) ? n / 16 : 0;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nt = (size_t)gridDim.x * blockDim.x;
    if (to_maps) {
        for (size_t i = t; i < n16; i += nt) ((int4*)m)[i] = ((const int4*)flat)[i];
        for (size_t i = n16 * 16 + t; i < n; i += nt) m[i] = flat[i];
    } else {
        for (size_t i = t; i < n16; i += nt) ((int4*)flat)[i] = ((const int4*)m)[i];
        for (size_t i = n16 * 16 + t; i < n; i += nt) flat[i] = m[i];
    }
}

// ---------------------------------------------------------------- action + weigh
struct rb_weigh_args {
    int P, R;
    const float4* src; float4* dst; float4* parent;
    const int32_t* idx; const int32_t* slot;
    const int8_t* maps; size_t stride; bl_frame frame;
    const float* ranges; const float* thetas; const int64_t* times;
    int64_t t_begin; double t_den; int interp;
    const float* noise;
    double rot1, trans, rot2, rot1Std, transStd, rot2Std;
    uint32_t seed_lo, seed_hi, step;
    long long* cum; unsigned long long* units; int32_t* like;
};

// ACTION: step 3 and step 4 of particle m in one wave (the form every update without scan matching launches).  !ACTION: step 4
// alone, on the pose and parent pose that k_rb_match (bl_rbslam_match.h) has left in dst and parent.
template <bool ACTION>
__device__ __forceinline__ void rb_weigh_wave(const rb_weigh_args& a)
{
    const int lane = threadIdx.x & 63;
    const int m = blockIdx.x * (RB_WEIGH_THREADS / 64) + (threadIdx.x >> 6);
    if (m >= a.P) return;                                       // whole waves; no barrier below
    float4 s;
    float px, py, pth;
    if (ACTION) {
        s = a.src[a.idx[m]];
        bl_pf_apply_action(a, m, m, s, px, py, pth);            // the same in every lane of the wave
        if (lane == 0) { a.dst[m] = make_float4(px, py, pth, 0.0f); a.parent[m] = make_float4(s.x, s.y, s.z, 0.0f); }
    } else {
        s = a.parent[m];
        const float4 d = a.dst[m];
        px = d.x; py = d.y; pth = d.z;
    }
    // ---- SensorModel::likelihood (sensor_model.cpp:14-25) over MovingLaserScan(scan, parent_pose, pose), against the particle's own map
    const int8_t* cells = a.maps + (size_t)a.slot[m] * a.stride;
    const bl_pose3 pb = {s.x, s.y, s.z}, pe = {px, py, pth};
    int acc = 0;
    for (int n = lane; n < a.R; n += 64) {                      // the host keeps only rays with range > 0.15f (moving_laser_scan.cpp:24)
        float sx, sy, sn, cs; int isx, isy;
        const bl_pose3 rp = bl_ray_pose(a.interp != 0, pb, pe, a.times, n, a.t_begin, a.t_den);
        bl_ray_setup(a.frame, rp, a.thetas[n], &sx, &sy, &isx, &isy, &sn, &cs);
        acc += bl_score_ray_half_units(a.frame.cpm, sx, sy, isx, isy, a.ranges[n], cs, sn,
                                       [&](int x, int y) { return bl_grid_odds(cells, a.frame, x, y); });
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (lane == 0) {
        long long c = a.cum[m] + (long long)acc;                // k_rb_plan has zeroed it when it resampled
        if (c > RB_SCORE_SAT) c = RB_SCORE_SAT;
        a.cum[m] = c;
        a.like[m] = acc;
        a.units[m] = bl_score_units(c);
    }
}

__global__ __launch_bounds__(RB_WEIGH_THREADS) void k_rb_weigh(rb_weigh_args a) { rb_weigh_wave<true>(a); }
__global__ __launch_bounds__(RB_WEIGH_THREADS) void k_rb_weigh_matched(rb_weigh_args a) { rb_weigh_wave<false>(a); }

#include "bl_rbslam_match.h"

// ---------------------------------------------------------------- units -> S, Q, best
__global__ __launch_bounds__(RB_PLAN_THREADS) void k_rb_reduce(int P, const unsigned long long* __restrict__ units, const float4* __restrict__ pose,
                                                               int64_t utime, int weighed, rb_state* state)
{
    __shared__ unsigned long long s_w64[RB_PLAN_THREADS / 64 * 4];
    __shared__ unsigned long long s_key[RB_PLAN_THREADS / 64];
    const int tid = threadIdx.x;
    rb_sums sums = {0, 0, 0, 0};
    unsigned long long key = 0;                                 // (u, 4095 - index): the largest u, ties to the lowest index; u < 2^43
    for (int i = tid; i < P; i += RB_PLAN_THREADS) {
        const unsigned long long u = units[i];
        rb_sums_add(sums, u);
        const unsigned long long k = (u << 12) | (unsigned long long)(RB_MAX_PARTICLES - 1 - i);
        key = k > key ? k : key;
    }
    const rb_sums tot = rb_block_sums(sums, s_w64);
    for (int off = 32; off > 0; off >>= 1) { const unsigned long long o = __shfl_xor(key, off, 64); key = o > key ? o : key; }
    if ((tid & 63) == 0) s_key[tid >> 6] = key;
    __syncthreads();
    if (tid == 0) {
        for (int w = 0; w < RB_PLAN_THREADS / 64; ++w) key = s_key[w] > key ? s_key[w] : key;
        const int best = RB_MAX_PARTICLES - 1 - (int)(key & (RB_MAX_PARTICLES - 1));
        const unsigned __int128 Q = rb_q_of(tot);
        state->S = tot.S; state->Q_lo = (unsigned long long)Q; state->Q_hi = (unsigned long long)(Q >> 64);
        state->best = best;
        state->weighed = weighed;
        const float4 p = pose[best];
        bl_pose_xyt_t bp; bp.utime = utime; bp.x = p.x; bp.y = p.y; bp.theta = p.z;
        state->best_pose = bp;
    }
}

// ---------------------------------------------------------------- map update of all P maps
struct rb_map_args {
    int P, R;
    int8_t* maps; size_t stride; bl_frame frame;
    const int32_t* slot;
    const float4* begin; const float4* end;  // parent poses and poses (a moved update), or the poses twice
    const float* ranges; const float* thetas; const int64_t* times;
    int64_t t_begin; double t_den; int interp;
    float max_laser; int hit, miss;
};

// start cell and end cell of ray r (bl_mapray_dev.h)
__device__ __forceinline__ int4 rb_ray_of(const rb_map_args& a, const bl_pose3& pb, const bl_pose3& pe, int r)
{
    return bl_ray_cells(a.frame, a.max_laser, a.interp != 0, a.t_begin, a.t_den, pb, pe, a.ranges[r], a.thetas[r], a.interp ? a.times[r] : 0);
}

// One owner thread per cell of the tile: v' = HIT ? min(127, v + k c) : max(-128, v - k c) where the count c is not zero.
template <bool HIT>
__device__ __forceinline__ void rb_apply(int8_t* cells, int W, const unsigned int* s_cnt, int tx0, int ty0, int tw, int th, int k, bool dwords)
{
    const int tid = threadIdx.x;
    if (dwords) {                                               // grid rows and tile columns are whole dwords: four cells per access
        const int wq = tw >> 2, nitems = th * wq;
        for (int it = tid; it < nitems; it += RB_MAP_THREADS) {
            const int ry = it / wq, dq = it - ry * wq;
            const unsigned long long c = *(const unsigned long long*)&s_cnt[(ry * tw + 4 * dq) >> 1];
            if (!c) continue;
            int* g = (int*)(cells + (size_t)(ty0 + ry) * W + tx0 + 4 * dq);
            *g = (int)bl_apply4<HIT>(c, *g, k);
        }
    } else {
        for (int it = tid; it < tw * th; it += RB_MAP_THREADS) {
            const int cnt = bl_cnt_of(s_cnt, it);
            if (!cnt) continue;
            const int ry = it / tw, cx = it - ry * tw;
            int8_t* g = cells + (size_t)(ty0 + ry) * W + tx0 + cx;
            const int val = *g;
            *g = (int8_t)(HIT ? min(127, val + k * cnt) : max(-128, val - k * cnt));
        }
    }
}

// Mapping::updateMap (mapping.cpp:17-127) of particle blockIdx.x's map.  All hits are applied before any miss, as the reference's two
// passes do, so a cell ends at max(-128, min(127, v + hit H) - miss M).  The window -- the bounding box of all ray cells clipped to the
// grid -- is cut into tiles of at most RB_MAP_COUNTERS cells; the workgroups of a particle (gridDim.y of them) take its tiles in turn,
// each forming the ray geometry itself.  Tiles are disjoint, so the workgroups of a particle never store to the same cell.
__global__ __launch_bounds__(RB_MAP_THREADS) void k_rb_map(rb_map_args a)
{
    __shared__ unsigned int s_cnt[RB_MAP_COUNTERS / 2];
    __shared__ int4 s_rays[RB_MAP_SEG_RAYS];
    __shared__ int s_segp[RB_MAP_SEG_RAYS + 1];
    __shared__ int s_wsum[RB_MAP_THREADS / 64];
    __shared__ int s_box[4];
    const int tid = threadIdx.x, p = blockIdx.x;
    const bool seg_walk = a.R <= RB_MAP_SEG_RAYS;
    int8_t* cells = a.maps + (size_t)a.slot[p] * a.stride;
    const float4 b4 = a.begin[p], e4 = a.end[p];
    const bl_pose3 pb = {b4.x, b4.y, b4.z}, pe = {e4.x, e4.y, e4.z};
    if (tid == 0) { s_box[0] = BL_NO_RAY; s_box[1] = BL_NO_RAY; s_box[2] = -BL_NO_RAY; s_box[3] = -BL_NO_RAY; }
    __syncthreads();
    // ---- ray geometry, bounding box, segment table
    bl_box box = bl_box_none();
    int segs = 0;
    for (int r = tid; r < a.R; r += RB_MAP_THREADS) {
        const int4 ray = rb_ray_of(a, pb, pe, r);
        bl_box_add(box, ray);
        if (seg_walk) {
            s_rays[r] = ray;
            segs = bl_ray_segs(ray, RB_MAP_SEG);
        }
    }
    bl_box_to_lds(box, s_box);
    if (seg_walk) {                                             // thread r holds ray r's segment count (R <= 512 threads)
        int total;
        const int excl = rb_block_excl_scan(segs, s_wsum, &total);
        if (tid < a.R) s_segp[tid] = excl;
        if (tid == 0) s_segp[a.R] = total;
    }
    __syncthreads();
    const int W = a.frame.width, H = a.frame.height;
    int bx0 = max(s_box[0], 0), by0 = max(s_box[1], 0);
    int bx1 = min(s_box[2], W - 1), by1 = min(s_box[3], H - 1);
    if (bx1 < bx0 || by1 < by0) return;                         // nothing inside the grid (uniform over the workgroup)
    const bool dwords = (W & 3) == 0;                           // rows of whole dwords (the slots are 16-byte aligned)
    if (dwords) { bx0 &= ~3; bx1 |= 3; }
    const int ww = bx1 - bx0 + 1, wh = by1 - by0 + 1;
    const int tw_max = ww < RB_MAP_TILE_W ? ww : RB_MAP_TILE_W; // a multiple of 4 when dwords
    const int th_max = min(wh, RB_MAP_COUNTERS / tw_max);       // >= 80 rows
    const int ntx = (ww + tw_max - 1) / tw_max, nty = (wh + th_max - 1) / th_max;
    for (int tile = blockIdx.y; tile < ntx * nty; tile += gridDim.y) {
        const int tyi = tile / ntx, txi = tile - tyi * ntx;
        const int tx0 = bx0 + txi * tw_max, ty0 = by0 + tyi * th_max;
        const int tx1 = min(tx0 + tw_max - 1, bx1), ty1 = min(ty0 + th_max - 1, by1);
        const int tw = tx1 - tx0 + 1, th = ty1 - ty0 + 1;
        const int nwords = (tw * th + 1) / 2;
        __syncthreads();
        for (int i = tid; i < nwords; i += RB_MAP_THREADS) s_cnt[i] = 0;
        __syncthreads();
        auto count = [&](int x, int y) {                        // a cell of a ray, counted where it falls into the tile
            if (x >= tx0 && x <= tx1 && y >= ty0 && y <= ty1) bl_cnt_add(s_cnt, (y - ty0) * tw + (x - tx0));
        };
        // ---- endpoint pass (mapping.cpp:42-57): H = rays ending in a cell
        for (int r = tid; r < a.R; r += RB_MAP_THREADS) {
            const int4 ray = seg_walk ? s_rays[r] : rb_ray_of(a, pb, pe, r);
            if (ray.x != BL_NO_RAY) count(ray.z, ray.w);
        }
        __syncthreads();
        rb_apply<true>(cells, W, s_cnt, tx0, ty0, tw, th, a.hit, dwords);
        __syncthreads();                                        // this workgroup's stores are visible to its own loads below
        for (int i = tid; i < nwords; i += RB_MAP_THREADS) s_cnt[i] = 0;
        __syncthreads();
        // ---- free-space pass (mapping.cpp:59-71, 101-127): M = rays crossing a cell
        if (seg_walk) {
            const int nseg = s_segp[a.R];
            for (int sg = tid; sg < nseg; sg += RB_MAP_THREADS) {
                const int r = bl_seg_ray(s_segp, a.R, sg);
                const int k0 = (sg - s_segp[r]) * RB_MAP_SEG;
                bl_walk_range(s_rays[r], k0, k0 + RB_MAP_SEG, count);
            }
        } else {
            for (int r = tid; r < a.R; r += RB_MAP_THREADS) {
                const int4 ray = rb_ray_of(a, pb, pe, r);
                if (ray.x != BL_NO_RAY) bl_walk_range(ray, 0, bl_ray_steps(ray), count);
            }
        }
        __syncthreads();
        rb_apply<false>(cells, W, s_cnt, tx0, ty0, tw, th, a.miss, dwords);
    }
}

// ---------------------------------------------------------------- init / export
__global__ void k_rb_init(int P, bl_pose_xyt_t pose, uint32_t k0, uint32_t k1, float4* rec, float4* parent, long long* cum,
                          unsigned long long* units, int32_t* like, int32_t* idx, int32_t* slot)
{
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= P) return;
    float th, y, x;                                             // (in k_pf_init's order: the compiler's selects follow it)
    bl_pf_init_draw(pose.x, pose.y, pose.theta, m, P, k0, k1, x, y, th);     // the filter's own draw (bl_pfmodel.h)
    rec[m] = make_float4(x, y, th, 0.0f);
    parent[m] = make_float4(x, y, th, 0.0f);
    cum[m] = 0; units[m] = 2ull; like[m] = 0; idx[m] = m; slot[m] = m;
}

__global__ void k_rb_export(int P, const float4* rec, const float4* parent, const unsigned long long* units, const rb_state* state,
                            int64_t pose_utime, int64_t parent_utime, bl_particle_t* out)
{
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= P) return;
    const float4 r = rec[m], q = parent[m];
    bl_particle_t o; bl_particle_fill(&o, r, pose_utime, q, parent_utime);
    o.weight = (double)units[m] / (double)state->S;
    out[m] = o;
}

// ---------------------------------------------------------------- host side
static int rb_launch_reduce(bl_rbslam* rb, int weighed)
{
    hipLaunchKernelGGL(k_rb_reduce, dim3(1), dim3(RB_PLAN_THREADS), 0, rb->ctx->stream, rb->P, rb->units, rb->pose[rb->cur], rb->pose_utime,
                       weighed, rb->state);
    BL_HIP(hipGetLastError());
    return BL_OK;
}

static void rb_free(bl_rbslam* rb)
{
    void* d[] = {rb->maps, rb->staging, rb->pose[0], rb->pose[1], rb->parent, rb->cum, rb->units, rb->like, rb->idx, rb->slot, rb->copies,
                 rb->d_noise, rb->state, rb->d_export, rb->match_rays, rb->match_out};
    for (void* q : d) if (q) (void)hipFree(q);
    if (rb->h_state) (void)hipHostFree(rb->h_state);
    if (rb->h_match_rays) (void)hipHostFree(rb->h_match_rays);
    delete rb;
}

extern "C" int bl_rbslam_create(bl_ctx* ctx, int num_particles, int width, int height, float meters_per_cell, float cells_per_meter,
                                float origin_x, float origin_y, float max_laser_distance, int8_t hit_odds, int8_t miss_odds, bl_rbslam** out)
{
    BL_CHECK_ARG(ctx != nullptr && out != nullptr);
    BL_CHECK_ARG(num_particles >= 1 && num_particles <= BL_RBSLAM_MAX_PARTICLES);
    BL_CHECK_ARG(width > 0 && height > 0 && width <= 65535 && height <= 65535);
    BL_CHECK_ARG(hit_odds >= 0 && miss_odds >= 0);
    static_assert(BL_RBSLAM_MAX_PARTICLES == RB_MAX_PARTICLES && BL_RBSLAM_SCORE_MAX == RB_SCORE_SAT, "botlab_hip.h and bl_rbslam.hip disagree");
    const size_t stride = ((size_t)width * height + 15) & ~(size_t)15;
    if ((unsigned long long)stride * (unsigned long long)num_particles > BL_RBSLAM_MAX_MAP_BYTES) {
        bl_set_error("bl_rbslam_create: %d maps of %d x %d cells exceed the cap of %llu bytes", num_particles, width, height,
                     (unsigned long long)BL_RBSLAM_MAX_MAP_BYTES);
        return BL_ERR_ARG;
    }
    BL_HIP(hipSetDevice(ctx->device));
    bl_rbslam* rb = new bl_rbslam();
    memset(rb, 0, sizeof(*rb));
    rb->ctx = ctx; rb->P = num_particles;
    rb->frame.width = width; rb->frame.height = height; rb->frame.mpc = meters_per_cell; rb->frame.cpm = cells_per_meter;
    rb->frame.ox = origin_x; rb->frame.oy = origin_y;
    rb->stride = stride;
    rb->max_laser = max_laser_distance; rb->hit = hit_odds; rb->miss = miss_odds;
    rb->num = 1; rb->den = 2;
    rb->match_path = -1;
    const size_t P = (size_t)num_particles;
    hipError_t e = hipMalloc((void**)&rb->maps, stride * P);
    if (e == hipSuccess) e = hipMalloc((void**)&rb->staging, stride);
    if (e == hipSuccess) e = hipMalloc((void**)&rb->pose[0], P * sizeof(float4));
    if (e == hipSuccess) e = hipMalloc((void**)&rb->pose[1], P * sizeof(float4));
    if (e == hipSuccess) e = hipMalloc((void**)&rb->parent, P * sizeof(float4));
    if (e == hipSuccess) e = hipMalloc((void**)&rb->cum, P * sizeof(long long));
    if (e == hipSuccess) e = hipMalloc((void**)&rb->units, P * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMalloc((void**)&rb->like, P * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&rb->idx, P * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&rb->slot, P * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&rb->copies, P * sizeof(int2));
    if (e == hipSuccess) e = hipMalloc((void**)&rb->d_noise, P * 3 * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&rb->state, sizeof(rb_state));
    if (e == hipSuccess) e = hipMalloc((void**)&rb->d_export, P * sizeof(bl_particle_t));
    if (e == hipSuccess) e = hipHostMalloc((void**)&rb->h_state, sizeof(rb_state), hipHostMallocDefault);
    if (e != hipSuccess) { bl_set_error("bl_rbslam_create: allocation failed: %s", hipGetErrorString(e)); rb_free(rb); return BL_ERR_HIP; }
    *out = rb;
    return BL_OK;
}

extern "C" void bl_rbslam_destroy(bl_rbslam* rb)
{
    if (!rb) return;
    (void)hipSetDevice(rb->ctx->device);
    (void)hipStreamSynchronize(rb->ctx->stream);
    rb_free(rb);
}

extern "C" int bl_rbslam_set_resampling(bl_rbslam* rb, uint32_t num, uint32_t den)
{
    BL_CHECK_ARG(rb != nullptr);
    BL_CHECK_ARG(num >= 1 && num <= 65535 && den >= 1 && den <= 65535);
    rb->num = num; rb->den = den;
    return BL_OK;
}

extern "C" int bl_rbslam_set_noise_seed(bl_rbslam* rb, uint64_t seed)
{
    BL_CHECK_ARG(rb != nullptr);
    rb->noise_seed = seed;
    return BL_OK;
}

extern "C" int bl_rbslam_set_scan_matching(bl_rbslam* rb, const bl_rbslam_match_params_t* params)
{
    BL_CHECK_ARG(rb != nullptr);
    if (!params) { rb->match_on = false; return BL_OK; }
    BL_CHECK_ARG(params->nx >= 0 && params->nx <= BL_RBSLAM_MATCH_MAX_N && params->ny >= 0 && params->ny <= BL_RBSLAM_MATCH_MAX_N);
    BL_CHECK_ARG(params->ntheta >= 0 && params->ntheta <= BL_RBSLAM_MATCH_MAX_NTHETA);
    BL_CHECK_ARG(params->dtheta > 0.0f);                         // false for NaN
    if (!rb->match_rays) {
        BL_HIP(hipSetDevice(rb->ctx->device));
        BL_HIP(hipMalloc((void**)&rb->match_rays, 2 * RBM_MAX_RAYS * sizeof(float)));
        BL_HIP(hipHostMalloc((void**)&rb->h_match_rays, 2 * RBM_MAX_RAYS * sizeof(float), hipHostMallocDefault));
        BL_HIP(hipMalloc((void**)&rb->match_out, 7 * (size_t)rb->P * sizeof(int32_t)));
    }
    rb->match = *params;
    rb->match_on = true;
    return BL_OK;
}

extern "C" int bl_rbslam_debug_match(bl_rbslam* rb, int32_t* di, int32_t* dj, int32_t* dk, int32_t* score, int32_t* score_centre,
                                     int32_t* ties, int32_t* accepted)
{
    BL_CHECK_ARG(rb != nullptr);
    if (!rb->match_done) { bl_set_error("bl_rbslam_debug_match: no moved update with scan matching on so far"); return BL_ERR_STATE; }
    BL_HIP(hipSetDevice(rb->ctx->device));
    int32_t* dst[7] = {di, dj, dk, score, score_centre, ties, accepted};
    const size_t P = (size_t)rb->P;
    for (int k = 0; k < 7; ++k)
        if (dst[k]) BL_HIP(hipMemcpyAsync(dst[k], rb->match_out + k * P, P * sizeof(int32_t), hipMemcpyDeviceToHost, rb->ctx->stream));
    BL_HIP(hipStreamSynchronize(rb->ctx->stream));
    return BL_OK;
}

extern "C" int bl_rbslam_debug_match_path(const bl_rbslam* rb)
{
    return rb ? rb->match_path : -1;
}

static void rb_reset_run(bl_rbslam* rb, int64_t pose_utime, int64_t parent_utime)
{
    rb->cur = 0;
    rb->pose_utime = pose_utime; rb->parent_utime = parent_utime;
    bl_action_reset(rb->action);
    rb->step = 0;
    rb->map_latched = false;
    rb->match_done = false; rb->match_path = -1;
    rb->initialized = true;
}

extern "C" int bl_rbslam_init_at_pose(bl_rbslam* rb, const bl_pose_xyt_t* pose, uint64_t seed)
{
    BL_CHECK_ARG(rb != nullptr && pose != nullptr);
    BL_HIP(hipSetDevice(rb->ctx->device));
    hipStream_t st = rb->ctx->stream;
    BL_HIP(hipMemsetAsync(rb->maps, 0, rb->stride * (size_t)rb->P, st));
    BL_HIP(hipMemsetAsync(rb->state, 0, sizeof(rb_state), st));
    hipLaunchKernelGGL(k_rb_init, dim3((rb->P + 255) / 256), dim3(256), 0, st, rb->P, *pose, (uint32_t)seed, (uint32_t)(seed >> 32), rb->pose[0],
                       rb->parent, rb->cum, rb->units, rb->like, rb->idx, rb->slot);
    BL_HIP(hipGetLastError());
    rb_reset_run(rb, pose->utime, pose->utime);
    return rb_launch_reduce(rb, 0);
}

extern "C" int bl_rbslam_set_particles(bl_rbslam* rb, const bl_particle_t* particles, const int64_t* cum_scores)
{
    BL_CHECK_ARG(rb != nullptr && particles != nullptr);
    if (!rb->initialized) { bl_set_error("bl_rbslam_set_particles before bl_rbslam_init_at_pose"); return BL_ERR_STATE; }
    const int P = rb->P;
    if (cum_scores) for (int m = 0; m < P; ++m) BL_CHECK_ARG(cum_scores[m] >= 0 && cum_scores[m] <= BL_RBSLAM_SCORE_MAX);
    BL_HIP(hipSetDevice(rb->ctx->device));
    hipStream_t st = rb->ctx->stream;
    std::vector<float4> rec(P), par(P);
    std::vector<long long> cum(P);
    std::vector<unsigned long long> units(P);
    for (int m = 0; m < P; ++m) {
        rec[m] = make_float4(particles[m].pose.x, particles[m].pose.y, particles[m].pose.theta, 0.0f);
        par[m] = make_float4(particles[m].parent_pose.x, particles[m].parent_pose.y, particles[m].parent_pose.theta, 0.0f);
        cum[m] = cum_scores ? cum_scores[m] : 0;
        units[m] = bl_score_units(cum[m]);
    }
    rb->cur = 0;
    rb->pose_utime = particles[0].pose.utime; rb->parent_utime = particles[0].parent_pose.utime;
    BL_HIP(hipMemcpyAsync(rb->pose[0], rec.data(), P * sizeof(float4), hipMemcpyHostToDevice, st));
    BL_HIP(hipMemcpyAsync(rb->parent, par.data(), P * sizeof(float4), hipMemcpyHostToDevice, st));
    BL_HIP(hipMemcpyAsync(rb->cum, cum.data(), P * sizeof(long long), hipMemcpyHostToDevice, st));
    BL_HIP(hipMemcpyAsync(rb->units, units.data(), P * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
    int rc = rb_launch_reduce(rb, cum_scores ? 1 : 0);
    if (rc) return rc;
    BL_HIP(hipStreamSynchronize(st));                           // caller-owned pageable buffers
    return BL_OK;
}

extern "C" int bl_rbslam_get_particles(bl_rbslam* rb, bl_particle_t* out, int64_t* cum_scores, uint64_t* units)
{
    BL_CHECK_ARG(rb != nullptr);
    if (!rb->initialized) { bl_set_error("bl_rbslam_get_particles before bl_rbslam_init_at_pose"); return BL_ERR_STATE; }
    BL_HIP(hipSetDevice(rb->ctx->device));
    hipStream_t st = rb->ctx->stream;
    const size_t P = (size_t)rb->P;
    if (out) {
        hipLaunchKernelGGL(k_rb_export, dim3((rb->P + 255) / 256), dim3(256), 0, st, rb->P, rb->pose[rb->cur], rb->parent, rb->units, rb->state,
                           rb->pose_utime, rb->parent_utime, rb->d_export);
        BL_HIP(hipGetLastError());
        BL_HIP(hipMemcpyAsync(out, rb->d_export, P * sizeof(bl_particle_t), hipMemcpyDeviceToHost, st));
    }
    if (cum_scores) BL_HIP(hipMemcpyAsync(cum_scores, rb->cum, P * sizeof(long long), hipMemcpyDeviceToHost, st));
    if (units) BL_HIP(hipMemcpyAsync(units, rb->units, P * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    BL_HIP(hipStreamSynchronize(st));
    return BL_OK;
}

// step 3b: the action and the match of every particle against its own map, one launch (bl_rbslam_match.h)
static int rb_launch_match(bl_rbslam* rb, const rb_weigh_args& wa, int rays, float reach_m)
{
    hipStream_t st = rb->ctx->stream;
    const bl_rbslam_match_params_t& mp = rb->match;
    if (rays > 0) {                                              // the pinned block is free: the previous update has synchronised
        BL_HIP(hipMemcpyAsync(rb->match_rays, rb->h_match_rays, (size_t)rays * sizeof(float), hipMemcpyHostToDevice, st));
        BL_HIP(hipMemcpyAsync(rb->match_rays + RBM_MAX_RAYS, rb->h_match_rays + RBM_MAX_RAYS, (size_t)rays * sizeof(float), hipMemcpyHostToDevice, st));
    }
    rb_match_args q;
    q.rays = rays; q.ranges = rb->match_rays; q.thetas = rb->match_rays + RBM_MAX_RAYS;
    q.nx = mp.nx; q.ny = mp.ny; q.ntheta = mp.ntheta; q.dtheta = mp.dtheta; q.min_score = mp.min_score;
    // half window: reach + n + 1 cells (botlab_hip.h); the bound of the window decides the path for the whole launch
    const float reach_c = ceilf(reach_m * rb->frame.cpm);
    const bool whole = !(reach_c < (float)(RBM_WHOLE - 64));      // also NaN
    q.hx = whole ? RBM_WHOLE : (int)reach_c + mp.nx + 1;
    q.hy = whole ? RBM_WHOLE : (int)reach_c + mp.ny + 1;
    long long bw = 2ll * q.hx + 1 + 3, bh = 2ll * q.hy + 1;       // + 3: the first column steps down to a multiple of four
    if (bw > rb->frame.width) bw = rb->frame.width;
    if (bh > rb->frame.height) bh = rb->frame.height;
    const long long win_bytes = ((bw + 3) & ~3ll) * bh;
    const bool staged = win_bytes <= (long long)RBM_WINDOW_BYTES;
    q.ends_bytes = (int)(((size_t)(rays > 0 ? rays : 1) * sizeof(int2) + 15) & ~(size_t)15);
    q.out = rb->match_out;
    const size_t lds = (size_t)q.ends_bytes + (staged ? (size_t)(win_bytes > 16 ? win_bytes : 16) : (size_t)16);   // never empty: a masked-out lookup reads byte 0
    if (staged) {
        BL_DYN_LDS_ONCE_PER_DEVICE(k_rb_match<true>, RBM_WINDOW_BYTES + RBM_MAX_RAYS * sizeof(int2), rb->ctx);
        hipLaunchKernelGGL(k_rb_match<true>, dim3(rb->P), dim3(RBM_THREADS), lds, st, wa, q);
    } else {
        hipLaunchKernelGGL(k_rb_match<false>, dim3(rb->P), dim3(RBM_THREADS), lds, st, wa, q);
    }
    BL_HIP(hipGetLastError());
    rb->match_path = staged ? 0 : 1;
    rb->match_done = true;
    return BL_OK;
}

extern "C" int bl_rbslam_update(bl_rbslam* rb, const bl_pose_xyt_t* odometry, const bl_lidar_t* scan, int rand_value, const float* noise,
                                bl_rbslam_result_t* result)
{
    BL_CHECK_ARG(rb != nullptr && odometry != nullptr && scan != nullptr);
    if (!rb->initialized) { bl_set_error("bl_rbslam_update before bl_rbslam_init_at_pose"); return BL_ERR_STATE; }
    BL_CHECK_ARG(scan->num_ranges >= 0 && scan->num_ranges <= RB_MAP_MAX_RAYS);
    bl_ctx* ctx = rb->ctx;
    BL_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    int R = 0;
    int rc = bl_scan_upload(ctx, scan, &R);
    if (rc) return rc;
    // scan matching: the valid rays, packed for the copy; too many are refused before the ActionModel latches the odometry
    int match_rays = 0; float match_reach = 0;
    if (rb->match_on) {
        const int valid = sm_valid_rays(scan, rb->match.max_range, nullptr, nullptr, nullptr);
        BL_CHECK_ARG(valid <= RBM_MAX_RAYS);
        match_rays = sm_valid_rays(scan, rb->match.max_range, rb->h_match_rays, rb->h_match_rays + RBM_MAX_RAYS, &match_reach);
    }
    const bool moved = bl_action_update(rb->action, *odometry);
    const int P = rb->P;
    if (moved) {
        if (noise) {
            BL_HIP(hipMemcpyAsync(rb->d_noise, noise, (size_t)P * 3 * sizeof(float), hipMemcpyHostToDevice, st));
            BL_HIP(hipStreamSynchronize(st));                   // caller-owned pageable buffer
        }
        rb_plan_args pa;
        pa.P = P; pa.units = rb->units; pa.state = rb->state; pa.idx = rb->idx; pa.slot = rb->slot; pa.copies = rb->copies; pa.cum = rb->cum;
        pa.M_inv = 1.0 / P;
        pa.r = bl_resample_offset(rand_value, pa.M_inv);
        pa.num = rb->num; pa.den = rb->den;
        hipLaunchKernelGGL(k_rb_plan, dim3(1), dim3(RB_PLAN_THREADS), 0, st, pa);
        const int chunks = (int)((rb->stride / 16 + RB_COPY_THREADS * RB_COPY_VEC - 1) / (RB_COPY_THREADS * RB_COPY_VEC));
        if (P > 1) {
            long long blocks = (long long)(P - 1) * chunks;
            if (blocks > 2048) blocks = 2048;
            hipLaunchKernelGGL(k_rb_copy, dim3((unsigned)blocks), dim3(RB_COPY_THREADS), 0, st, rb->maps, rb->stride, rb->copies, rb->state, chunks);
        }
        rb_weigh_args wa;
        wa.P = P; wa.R = R;
        wa.src = rb->pose[rb->cur]; wa.dst = rb->pose[rb->cur ^ 1]; wa.parent = rb->parent;
        wa.idx = rb->idx; wa.slot = rb->slot; wa.maps = rb->maps; wa.stride = rb->stride; wa.frame = rb->frame;
        wa.ranges = ctx->scan.ranges; wa.thetas = ctx->scan.thetas; wa.times = ctx->scan.times;
        // the parent pose carries the utime the pose had, the pose takes the odometry's
        wa.t_begin = rb->pose_utime;
        wa.interp = rb->pose_utime != odometry->utime ? 1 : 0;
        wa.t_den = wa.interp ? (double)(odometry->utime - rb->pose_utime) : 1.0;
        wa.noise = noise ? rb->d_noise : nullptr;
        wa.rot1 = rb->action.rot1; wa.trans = rb->action.trans; wa.rot2 = rb->action.rot2; wa.rot1Std = rb->action.rot1Std; wa.transStd = rb->action.transStd; wa.rot2Std = rb->action.rot2Std;
        wa.seed_lo = (uint32_t)rb->noise_seed; wa.seed_hi = (uint32_t)(rb->noise_seed >> 32); wa.step = rb->step;
        wa.cum = rb->cum; wa.units = rb->units; wa.like = rb->like;
        if (!rb->match_on) {
            hipLaunchKernelGGL(k_rb_weigh, dim3((P + RB_WEIGH_THREADS / 64 - 1) / (RB_WEIGH_THREADS / 64)), dim3(RB_WEIGH_THREADS), 0, st, wa);
        } else {
            rc = rb_launch_match(rb, wa, match_rays, match_reach);
            if (rc) return rc;
            hipLaunchKernelGGL(k_rb_weigh_matched, dim3((P + RB_WEIGH_THREADS / 64 - 1) / (RB_WEIGH_THREADS / 64)), dim3(RB_WEIGH_THREADS), 0, st, wa);
        }
        BL_HIP(hipGetLastError());
        rb->cur ^= 1;
        rb->parent_utime = rb->pose_utime;
        rb->pose_utime = odometry->utime;
        rb->step += 1;
        rc = rb_launch_reduce(rb, 1);
        if (rc) return rc;
    }
    if (rb->map_latched && R > 0) {
        rb_map_args ma;
        ma.P = P; ma.R = R; ma.maps = rb->maps; ma.stride = rb->stride; ma.frame = rb->frame; ma.slot = rb->slot;
        ma.end = rb->pose[rb->cur];
        ma.begin = moved ? rb->parent : rb->pose[rb->cur];
        ma.ranges = ctx->scan.ranges; ma.thetas = ctx->scan.thetas; ma.times = ctx->scan.times;
        ma.interp = (moved && rb->parent_utime != rb->pose_utime) ? 1 : 0;
        ma.t_begin = rb->parent_utime;
        ma.t_den = ma.interp ? (double)(rb->pose_utime - rb->parent_utime) : 1.0;
        ma.max_laser = rb->max_laser; ma.hit = rb->hit; ma.miss = rb->miss;
        // tiles of the largest window the kept rays can span when the pose does not move inside the scan; a wider window (a jump
        // between parent pose and pose) only makes the workgroups of a particle take several tiles each
        const float reach_m = ctx->scan.max_range < rb->max_laser ? ctx->scan.max_range : rb->max_laser;
        long long side = 2ll * (long long)ceilf(reach_m * rb->frame.cpm) + 8;
        const int ww = (int)(side < rb->frame.width ? side : rb->frame.width), wh = (int)(side < rb->frame.height ? side : rb->frame.height);
        const int tw = ww < RB_MAP_TILE_W ? ww : RB_MAP_TILE_W;
        int th = RB_MAP_COUNTERS / (tw < 1 ? 1 : tw); if (th > wh) th = wh; if (th < 1) th = 1;
        long long tiles = (long long)((ww + tw - 1) / tw) * ((wh + th - 1) / th);
        if (tiles < 1) tiles = 1;
        if (tiles > 64) tiles = 64;
        hipLaunchKernelGGL(k_rb_map, dim3(P, (unsigned)tiles), dim3(RB_MAP_THREADS), 0, st, ma);
        BL_HIP(hipGetLastError());
    }
    rb->map_latched = true;                                     // the very first update latches (mapping.cpp:19-21, 74, 88)
    BL_HIP(hipMemcpyAsync(rb->h_state, rb->state, sizeof(rb_state), hipMemcpyDeviceToHost, st));
    BL_HIP(hipStreamSynchronize(st));
    if (result) {
        memset(result, 0, sizeof(*result));
        result->moved = moved ? 1 : 0;
        result->resampled = moved ? rb->h_state->resampled : 0;
        result->best = rb->h_state->best;
        result->best_pose = rb->h_state->best_pose;
        result->S = rb->h_state->S; result->Q_lo = rb->h_state->Q_lo; result->Q_hi = rb->h_state->Q_hi;
    }
    return BL_OK;
}

static int rb_map_io(bl_rbslam* rb, int which, int8_t* flat, int to_maps)
{
    const size_t n = (size_t)rb->frame.width * rb->frame.height;
    size_t blocks = (n / 16 + RB_COPY_THREADS - 1) / RB_COPY_THREADS;
    if (blocks < 1) blocks = 1;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(k_rb_map_io, dim3((unsigned)blocks), dim3(RB_COPY_THREADS), 0, rb->ctx->stream, rb->maps, rb->stride, rb->slot, rb->state,
                       which, flat, n, to_maps);
    BL_HIP(hipGetLastError());
    return BL_OK;
}

extern "C" int bl_rbslam_map_download(bl_rbslam* rb, int p, int8_t* cells)
{
    BL_CHECK_ARG(rb != nullptr && cells != nullptr && p >= 0 && p < rb->P);
    if (!rb->initialized) { bl_set_error("bl_rbslam_map_download before bl_rbslam_init_at_pose"); return BL_ERR_STATE; }
    BL_HIP(hipSetDevice(rb->ctx->device));
    int rc = rb_map_io(rb, p, rb->staging, 0);
    if (rc) return rc;
    BL_HIP(hipMemcpyAsync(cells, rb->staging, (size_t)rb->frame.width * rb->frame.height, hipMemcpyDeviceToHost, rb->ctx->stream));
    BL_HIP(hipStreamSynchronize(rb->ctx->stream));
    return BL_OK;
}

extern "C" int bl_rbslam_map_upload(bl_rbslam* rb, int p, const int8_t* cells)
{
    BL_CHECK_ARG(rb != nullptr && cells != nullptr && p >= 0 && p < rb->P);
    if (!rb->initialized) { bl_set_error("bl_rbslam_map_upload before bl_rbslam_init_at_pose"); return BL_ERR_STATE; }
    BL_HIP(hipSetDevice(rb->ctx->device));
    BL_HIP(hipMemcpyAsync(rb->staging, cells, (size_t)rb->frame.width * rb->frame.height, hipMemcpyHostToDevice, rb->ctx->stream));
    int rc = rb_map_io(rb, p, rb->staging, 1);
    if (rc) return rc;
    BL_HIP(hipStreamSynchronize(rb->ctx->stream));              // caller-owned buffer
    return BL_OK;
}

extern "C" int bl_rbslam_best_map(bl_rbslam* rb, bl_grid* dst)
{
    BL_CHECK_ARG(rb != nullptr && dst != nullptr);
    if (!rb->initialized) { bl_set_error("bl_rbslam_best_map before bl_rbslam_init_at_pose"); return BL_ERR_STATE; }
    BL_CHECK_ARG(dst->frame.width == rb->frame.width && dst->frame.height == rb->frame.height);
    BL_CHECK_ARG(dst->ctx == rb->ctx);                          // one stream orders the copy behind the updates
    BL_HIP(hipSetDevice(rb->ctx->device));
    dst->frame = rb->frame;
    dst->mirror_valid = false;
    (void)bl_grid_new_lineage(dst);
    return rb_map_io(rb, -1, dst->cells, 0);
}

extern "C" int bl_rbslam_debug_last(bl_rbslam* rb, int32_t* resample_idx, int32_t* likelihood_half_units)
{
    BL_CHECK_ARG(rb != nullptr);
    if (!rb->initialized) { bl_set_error("bl_rbslam_debug_last before bl_rbslam_init_at_pose"); return BL_ERR_STATE; }
    BL_HIP(hipSetDevice(rb->ctx->device));
    const size_t P = (size_t)rb->P;
    if (resample_idx) BL_HIP(hipMemcpyAsync(resample_idx, rb->idx, P * sizeof(int32_t), hipMemcpyDeviceToHost, rb->ctx->stream));
    if (likelihood_half_units) BL_HIP(hipMemcpyAsync(likelihood_half_units, rb->like, P * sizeof(int32_t), hipMemcpyDeviceToHost, rb->ctx->stream));
    BL_HIP(hipStreamSynchronize(rb->ctx->stream));
    return BL_OK;
}
