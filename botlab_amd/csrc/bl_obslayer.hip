// bl_obslayer.hip -- the obstacle layer (include/botlab_hip.h, "obstacle layer"): what the scan sees and the map does not, as a
// per-cell hit / clear / expire state beside the static map and an int8 grid composed of both.  No reference counterpart; the
// definition in the header is the contract and tests/obstacle_layer_model.py restates it.
//
//   k_obs_rays     a wave per ray of the scan.  The ray's geometry is the scan matcher's (k_sm_raster at heading step 0), formed by
//                  every lane alike.  Phase 1: the lanes take the cells of the walk 64 at a time (closed form of the reference's
//                  Bresenham variant, bl_mapray_dev.h) and a ballot finds `first`, the least occupied one; the tol box around the end
//                  cell, clipped to the grid, is spread over the lanes the same way.  Phase 2, once the class is known: the cells
//                  k < first get the update's number n stored into the clear stamps, the end cell of a NOVEL ray into the hit
//                  stamps.  Plain stores of one value from any number of waves: a set without atomics and without a memset.
//   k_obs_apply    a thread per cell of a box that holds every walk of the update (formed on the host from the pose and the reach,
//                  clipped to the grid): the transition of the cells whose stamps equal n.
//   k_obs_compose  16 cells per thread: the map's cells with 127 where the layer is live.  `last` is read only for the cells whose
//                  count reaches min_hits.  The grid is treated as one flat array, so the width plays no part; the cells behind the
//                  last whole 16 are taken one per thread.
//   k_obs_rowcount, k_obs_rowscan, k_obs_livewrite   the readers (stats, live cells): counts per row, their exclusive prefix, and a
//                  write pass in which every row's workgroup places its live cells in x order behind the row's offset.
//
// Integers only behind the end cells; no atomics; no result depends on the launch shape or on the order of the rays.
#include <math.h>
#include <string.h>

#include "bl_internal.h"
#include "bl_mapray_dev.h"
#include "bl_obslayer_dev.h"

#define OBS_MIN_RANGE 0.15f               // moving_laser_scan.cpp:24, as the scan matcher
#define OBS_RAY_WAVES 4                   // rays (waves) per workgroup of k_obs_rays
#define OBS_OFF 0
#define OBS_EXPLAINED 1
#define OBS_NOVEL 2
#define OBS_THROUGH 3
#define OBS_OUTSIDE 4

__global__ __launch_bounds__(64 * OBS_RAY_WAVES) void k_obs_rays(const int8_t* __restrict__ cells, bl_frame f, const float* __restrict__ ranges,
                                                                 const float* __restrict__ thetas, int R, float px, float py, float ptheta,
                                                                 float max_range, int occ_min, int tol, uint32_t n,
                                                                 uint32_t* __restrict__ hit, uint32_t* __restrict__ clr,
                                                                 uint8_t* __restrict__ classes)
{
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * OBS_RAY_WAVES + (threadIdx.x >> 6);
    if (r >= R) return;                                                 // (every branch below is uniform over the wave)
    const float range = ranges[r];
    int cls = OBS_OFF;
    if (range > OBS_MIN_RANGE && range < max_range) {
        const float a = bl_wrap_to_pi(ptheta - thetas[r]);
        float sn, cs, fsx, fsy;
        bl_sincosf_cells(a, &sn, &cs);
        bl_global_to_grid(px, py, f, &fsx, &fsy);
        const float fx = range * cs * f.cpm + fsx;
        const float fy = range * sn * f.cpm + fsy;
        // has: beyond +-2^30 (or NaN) the ray takes no part.  Within it the start cell fits an int too: it lies within the reach
        // (at most 4096 cells and a rounding) of the end point.
        if (__builtin_fabsf(fx) < 0x1p30f && __builtin_fabsf(fy) < 0x1p30f) {
            const int W = f.width, H = f.height;
            const int ex = (int)fx, ey = (int)fy;
            const int4 ray = make_int4((int)fsx, (int)fsy, ex, ey);
            const int K = bl_ray_steps(ray);
            // ---- phase 1: first, the least k whose cell is inside the grid and occupied
            int first = K;
            for (int base = 0; base < K; base += 64) {
                const int k = base + lane;
                bool occ = false;
                if (k < K) {
                    int x, y;
                    bl_walk_cell(ray, k, &x, &y);
                    if (x >= 0 && x < W && y >= 0 && y < H) occ = cells[(size_t)y * W + x] >= occ_min;
                }
                const unsigned long long m = __ballot(occ);
                if (m) { first = base + __ffsll((long long)m) - 1; break; }
            }
            // ---- explained: an occupied cell of the grid within tol of the end cell (the box clipped: nothing outside is read)
            const int x0 = max(ex - tol, 0), x1 = min(ex + tol, W - 1), y0 = max(ey - tol, 0), y1 = min(ey + tol, H - 1);
            bool explained = false;
            if (x0 <= x1 && y0 <= y1) {
                const int bw = x1 - x0 + 1, total = bw * (y1 - y0 + 1);   // at most 33 * 33
                for (int base = 0; base < total && !explained; base += 64) {
                    const int i = base + lane;
                    bool occ = false;
                    if (i < total) {
                        const int by = i / bw, bx = i - by * bw;
                        occ = cells[(size_t)(y0 + by) * W + (x0 + bx)] >= occ_min;
                    }
                    explained = __ballot(occ) != 0ull;
                }
            }
            const bool e_in = ex >= 0 && ex < W && ey >= 0 && ey < H;
            cls = explained ? OBS_EXPLAINED : first < K ? OBS_THROUGH : e_in ? OBS_NOVEL : OBS_OUTSIDE;
            // ---- phase 2: the marks
            if (cls != OBS_THROUGH) {
                for (int k = lane; k < first; k += 64) {
                    int x, y;
                    bl_walk_cell(ray, k, &x, &y);
                    if (x >= 0 && x < W && y >= 0 && y < H) clr[(size_t)y * W + x] = n;
                }
            }
            if (cls == OBS_NOVEL && lane == 0) hit[(size_t)ey * W + ex] = n;
        }
    }
    if (lane == 0) classes[r] = (uint8_t)cls;
}

// box: x0, y0, x1, y1 inclusive, inside the grid
__global__ __launch_bounds__(256) void k_obs_apply(const uint32_t* __restrict__ hit, const uint32_t* __restrict__ clr, uint8_t* __restrict__ count,
                                                   uint32_t* __restrict__ last, int W, int4 box, uint32_t n, uint32_t ttl)
{
    const int x = box.x + (int)blockIdx.x * 64 + (int)(threadIdx.x & 63);
    const int y = box.y + (int)blockIdx.y * 4 + (int)(threadIdx.x >> 6);
    if (x > box.z || y > box.w) return;
    const size_t i = (size_t)y * W + x;
    if (hit[i] == n) {                                                  // a hit beats a clear
        const uint32_t l = last[i];
        const uint32_t c = count[i];
        count[i] = (uint8_t)((l != 0u && n - l < ttl) ? (c < 255u ? c + 1u : 255u) : 1u);
        last[i] = n;
    } else if (clr[i] == n) {
        count[i] = 0;
        last[i] = 0u;
    }
}

__device__ __forceinline__ uint32_t obs_compose_word(uint32_t m, uint32_t c, const uint32_t* __restrict__ last4, const obs_live_rule& q)
{
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const uint32_t cnt = (c >> (8 * b)) & 0xffu;
        if (cnt >= q.min_hits && obs_live(q, cnt, last4[b])) m = (m & ~(0xffu << (8 * b))) | (127u << (8 * b));
    }
    return m;
}

__global__ __launch_bounds__(256) void k_obs_compose(const int8_t* __restrict__ map, const uint8_t* __restrict__ count, const uint32_t* __restrict__ last,
                                                     int8_t* __restrict__ out, size_t cells, obs_live_rule q)
{
    const size_t n16 = cells / 16;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n16) {
        uint4 m = ((const uint4*)map)[i];
        const uint4 c = ((const uint4*)count)[i];
        const uint32_t* l = last + i * 16;
        m.x = obs_compose_word(m.x, c.x, l, q);
        m.y = obs_compose_word(m.y, c.y, l + 4, q);
        m.z = obs_compose_word(m.z, c.z, l + 8, q);
        m.w = obs_compose_word(m.w, c.w, l + 12, q);
        ((uint4*)out)[i] = m;
    } else {
        const size_t j = n16 * 16 + (i - n16);                          // the cells behind the last whole 16, one per thread
        if (j < cells) out[j] = obs_live(q, count[j], last[j]) ? (int8_t)127 : map[j];
    }
}

// ---------------------------------------------------------------------------------------------------------------- readers
// per row: (live cells, cells hit in update n, cells cleared and not hit in update n)
__global__ __launch_bounds__(256) void k_obs_rowcount(const uint8_t* __restrict__ count, const uint32_t* __restrict__ last, const uint32_t* __restrict__ hit,
                                                      const uint32_t* __restrict__ clr, int W, obs_live_rule q, int sets, int4* __restrict__ rows)
{
    __shared__ int s_sum[4][3];
    const int y = blockIdx.x;
    int live = 0, hs = 0, cl = 0;
    for (int x = threadIdx.x; x < W; x += 256) {
        const size_t i = (size_t)y * W + x;
        const uint32_t c = count[i];
        if (c >= q.min_hits && obs_live(q, c, last[i])) ++live;
        if (sets) {
            const bool h = hit[i] == q.n;
            hs += h ? 1 : 0;
            cl += (!h && clr[i] == q.n) ? 1 : 0;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        live += __shfl_xor(live, off, 64); hs += __shfl_xor(hs, off, 64); cl += __shfl_xor(cl, off, 64);
    }
    if ((threadIdx.x & 63) == 0) { s_sum[threadIdx.x >> 6][0] = live; s_sum[threadIdx.x >> 6][1] = hs; s_sum[threadIdx.x >> 6][2] = cl; }
    __syncthreads();
    if (threadIdx.x == 0)
        rows[y] = make_int4(s_sum[0][0] + s_sum[1][0] + s_sum[2][0] + s_sum[3][0], s_sum[0][1] + s_sum[1][1] + s_sum[2][1] + s_sum[3][1],
                            s_sum[0][2] + s_sum[1][2] + s_sum[2][2] + s_sum[3][2], 0);
}

// one workgroup: rows[y].w = the number of live cells in the rows before y; totals = the three sums
__global__ __launch_bounds__(1024) void k_obs_rowscan(int4* __restrict__ rows, int H, int* __restrict__ totals)
{
    __shared__ int s_live[1024], s_hs[1024], s_cl[1024];
    const int t = threadIdx.x;
    const int per = (H + 1023) / 1024;
    const int y0 = min(t * per, H), y1 = min(y0 + per, H);
    int live = 0, hs = 0, cl = 0;
    for (int y = y0; y < y1; ++y) { const int4 v = rows[y]; live += v.x; hs += v.y; cl += v.z; }
    s_live[t] = live; s_hs[t] = hs; s_cl[t] = cl;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {                          // inclusive scan of the live counts, plain sums of the others
        const int a = t >= off ? s_live[t - off] : 0;
        __syncthreads();
        s_live[t] += a;
        __syncthreads();
    }
    int base = s_live[t] - live;
    for (int y = y0; y < y1; ++y) { int4 v = rows[y]; v.w = base; base += v.x; rows[y] = v; }
    if (t == 0) {
        int a = 0, b = 0;
        for (int k = 0; k < 1024; ++k) { a += s_hs[k]; b += s_cl[k]; }
        totals[0] = s_live[1023]; totals[1] = a; totals[2] = b;
    }
}

__global__ __launch_bounds__(256) void k_obs_livewrite(const uint8_t* __restrict__ count, const uint32_t* __restrict__ last, int W, obs_live_rule q,
                                                       const int4* __restrict__ rows, int32_t* __restrict__ xy, int cap)
{
    __shared__ int s_wave[4];
    const int y = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int base = rows[y].w;
    if (rows[y].x == 0) return;
    for (int xb = 0; xb < W; xb += 256) {
        const int x = xb + (int)threadIdx.x;
        bool on = false;
        if (x < W) {
            const size_t i = (size_t)y * W + x;
            const uint32_t c = count[i];
            on = c >= q.min_hits && obs_live(q, c, last[i]);
        }
        const unsigned long long m = __ballot(on);
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int before = 0, all = 0;
        for (int k = 0; k < 4; ++k) { before += k < wave ? s_wave[k] : 0; all += s_wave[k]; }
        if (on) {
            const int pos = base + before + __popcll(m & ((1ull << lane) - 1ull));
            if (pos < cap) { xy[2 * (size_t)pos] = x; xy[2 * (size_t)pos + 1] = y; }
        }
        base += all;
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------- host
extern "C" int bl_obslayer_create(bl_ctx* ctx, int width, int height, bl_obslayer** out)
{
    BL_CHECK_ARG(ctx != nullptr && out != nullptr);
    BL_CHECK_ARG(width >= 1 && height >= 1 && (long long)width * height < (1ll << 31));
    BL_HIP(hipSetDevice(ctx->device));
    bl_obslayer* ol = new bl_obslayer();
    memset((void*)ol, 0, sizeof(*ol));
    ol->ctx = ctx; ol->W = width; ol->H = height;
    const size_t cells = (size_t)width * height;
    const size_t padded = (cells + 15) & ~(size_t)15;
    hipError_t e = hipMalloc((void**)&ol->d_count, padded);
    if (e == hipSuccess) e = hipMalloc((void**)&ol->d_last, padded * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&ol->d_hit, cells * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&ol->d_clr, cells * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&ol->d_rows, (size_t)height * sizeof(int4));
    if (e == hipSuccess) e = hipMalloc((void**)&ol->d_totals, 3 * sizeof(int));
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ol->ev_stage, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreate(&ol->ev_ua);
    if (e == hipSuccess) e = hipEventCreate(&ol->ev_ub);
    if (e == hipSuccess) e = hipEventCreate(&ol->ev_ca);
    if (e == hipSuccess) e = hipEventCreate(&ol->ev_cb);
    if (e == hipSuccess) e = hipMemsetAsync(ol->d_count, 0, padded, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(ol->d_last, 0, padded * sizeof(uint32_t), ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(ol->d_hit, 0, cells * sizeof(uint32_t), ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(ol->d_clr, 0, cells * sizeof(uint32_t), ctx->stream);
    if (e != hipSuccess) {
        bl_set_error("bl_obslayer_create: %s", hipGetErrorString(e));
        bl_obslayer_destroy(ol);
        return BL_ERR_HIP;
    }
    *out = ol;
    return BL_OK;
}

extern "C" void bl_obslayer_destroy(bl_obslayer* ol)
{
    if (!ol) return;
    (void)hipSetDevice(ol->ctx->device);
    (void)hipStreamSynchronize(ol->ctx->stream);
    if (ol->d_count) (void)hipFree(ol->d_count);
    if (ol->d_last) (void)hipFree(ol->d_last);
    if (ol->d_hit) (void)hipFree(ol->d_hit);
    if (ol->d_clr) (void)hipFree(ol->d_clr);
    if (ol->d_rays) (void)hipFree(ol->d_rays);
    if (ol->d_classes) (void)hipFree(ol->d_classes);
    if (ol->h_rays) (void)hipHostFree(ol->h_rays);
    if (ol->d_rows) (void)hipFree(ol->d_rows);
    if (ol->d_totals) (void)hipFree(ol->d_totals);
    if (ol->d_xy) (void)hipFree(ol->d_xy);
    if (ol->ev_stage) (void)hipEventDestroy(ol->ev_stage);
    if (ol->ev_ua) (void)hipEventDestroy(ol->ev_ua);
    if (ol->ev_ub) (void)hipEventDestroy(ol->ev_ub);
    if (ol->ev_ca) (void)hipEventDestroy(ol->ev_ca);
    if (ol->ev_cb) (void)hipEventDestroy(ol->ev_cb);
    delete ol;
}

extern "C" int bl_obslayer_set_params(bl_obslayer* ol, const bl_obslayer_params_t* p)
{
    BL_CHECK_ARG(ol != nullptr && p != nullptr);
    BL_CHECK_ARG(isfinite(p->max_range) && p->max_range > OBS_MIN_RANGE);
    BL_CHECK_ARG(p->occ_min >= 1 && p->occ_min <= 127);
    BL_CHECK_ARG(p->tol_cells >= 0 && p->tol_cells <= BL_OBSLAYER_MAX_TOL);
    BL_CHECK_ARG(p->ttl_scans >= 1 && p->ttl_scans <= 65535);
    BL_CHECK_ARG(p->min_hits >= 1 && p->min_hits <= 255);
    ol->params = *p;
    ol->have_params = true;
    return BL_OK;
}

static obs_live_rule obs_rule(const bl_obslayer* ol)
{
    obs_live_rule q;
    q.n = ol->n; q.ttl = (uint32_t)ol->params.ttl_scans; q.min_hits = (uint32_t)ol->params.min_hits;
    return q;
}

static int obs_need_params(const bl_obslayer* ol)
{
    if (ol->have_params) return BL_OK;
    bl_set_error("obstacle layer has no parameters (bl_obslayer_set_params first)");
    return BL_ERR_STATE;
}

extern "C" int bl_obslayer_reset(bl_obslayer* ol)
{
    BL_CHECK_ARG(ol != nullptr);
    bl_ctx* ctx = ol->ctx;
    BL_HIP(hipSetDevice(ctx->device));
    const size_t cells = (size_t)ol->W * ol->H;
    BL_HIP(hipMemsetAsync(ol->d_count, 0, cells, ctx->stream));
    BL_HIP(hipMemsetAsync(ol->d_last, 0, cells * sizeof(uint32_t), ctx->stream));
    BL_HIP(hipMemsetAsync(ol->d_hit, 0, cells * sizeof(uint32_t), ctx->stream));
    BL_HIP(hipMemsetAsync(ol->d_clr, 0, cells * sizeof(uint32_t), ctx->stream));
    ol->n = 0;
    ol->last_rays = 0; ol->last_valid = 0; ol->sets_valid = false;
    return BL_OK;
}

extern "C" int bl_obslayer_update(bl_obslayer* ol, const bl_grid* map, const bl_lidar_t* scan, const bl_pose_xyt_t* pose)
{
    BL_CHECK_ARG(ol != nullptr && map != nullptr && scan != nullptr && pose != nullptr);
    int rc = obs_need_params(ol);
    if (rc) return rc;
    bl_ctx* ctx = ol->ctx;
    BL_CHECK_ARG(map->ctx == ctx);
    BL_CHECK_ARG(map->frame.width == ol->W && map->frame.height == ol->H);
    BL_CHECK_ARG(scan->num_ranges >= 0 && (scan->num_ranges == 0 || (scan->ranges != nullptr && scan->thetas != nullptr)));
    const bl_frame& f = map->frame;
    const bl_obslayer_params_t& p = ol->params;
    const double reach = ceil((double)p.max_range * (double)f.cpm);
    BL_CHECK_ARG(reach <= (double)BL_OBSLAYER_MAX_REACH);               // (false for NaN too)
    int valid = 0;
    for (int i = 0; i < scan->num_ranges; ++i) valid += (scan->ranges[i] > OBS_MIN_RANGE && scan->ranges[i] < p.max_range) ? 1 : 0;
    BL_CHECK_ARG(valid <= BL_OBSLAYER_MAX_RAYS);
    BL_CHECK_ARG(isfinite(pose->x) && isfinite(pose->y) && isfinite(pose->theta));
    if (ol->n == 0xffffffffu) { bl_set_error("bl_obslayer_update: the update counter is at its end (bl_obslayer_reset)"); return BL_ERR_STATE; }
    BL_HIP(hipSetDevice(ctx->device));
    const int R = scan->num_ranges;
    if (R > ol->ray_cap) {
        BL_HIP(hipStreamSynchronize(ctx->stream));
        if (ol->d_rays) { BL_HIP(hipFree(ol->d_rays)); ol->d_rays = nullptr; }
        if (ol->d_classes) { BL_HIP(hipFree(ol->d_classes)); ol->d_classes = nullptr; }
        if (ol->h_rays) { BL_HIP(hipHostFree(ol->h_rays)); ol->h_rays = nullptr; }
        ol->ray_cap = 0; ol->staged = false;
        const size_t c = ((size_t)R + 255) & ~(size_t)255;
        BL_HIP(hipMalloc((void**)&ol->d_rays, 2 * c * sizeof(float)));
        BL_HIP(hipMalloc((void**)&ol->d_classes, c));
        BL_HIP(hipHostMalloc((void**)&ol->h_rays, 2 * c * sizeof(float), hipHostMallocDefault));
        ol->ray_cap = (int)c;
    }
    // a box that holds every cell of every walk: a ray's end point lies within `reach` cells of the start position, each of its two
    // roundings is below 2^-23 of the larger operand, and the start cell itself is a rounding of the position formed here in double
    int4 box = make_int4(1, 1, 0, 0);
    {
        const double sx = ((double)pose->x - (double)f.ox) * (double)f.cpm, sy = ((double)pose->y - (double)f.oy) * (double)f.cpm;
        const double padx = reach + 2.0 + fabs(sx) * 1e-6, pady = reach + 2.0 + fabs(sy) * 1e-6;
        double x0 = floor(sx - padx), x1 = ceil(sx + padx), y0 = floor(sy - pady), y1 = ceil(sy + pady);
        if (x0 < 0.0) x0 = 0.0;
        if (y0 < 0.0) y0 = 0.0;
        if (x1 > (double)(ol->W - 1)) x1 = (double)(ol->W - 1);
        if (y1 > (double)(ol->H - 1)) y1 = (double)(ol->H - 1);
        if (x0 <= x1 && y0 <= y1) box = make_int4((int)x0, (int)y0, (int)x1, (int)y1);
    }
    ol->n += 1;                                                         // from here on the update is accepted
    ol->last_rays = R; ol->last_valid = valid; ol->sets_valid = true; ol->updated = true;
    if (R > 0) {
        if (ol->staged) BL_HIP(hipEventSynchronize(ol->ev_stage));      // the pinned block may still be on its way
        memcpy(ol->h_rays, scan->ranges, (size_t)R * sizeof(float));
        memcpy(ol->h_rays + ol->ray_cap, scan->thetas, (size_t)R * sizeof(float));
    }
    BL_HIP(hipEventRecord(ol->ev_ua, ctx->stream));
    if (R > 0) {
        BL_HIP(hipMemcpyAsync(ol->d_rays, ol->h_rays, ((size_t)ol->ray_cap + (size_t)R) * sizeof(float), hipMemcpyHostToDevice, ctx->stream));   // one copy
        BL_HIP(hipEventRecord(ol->ev_stage, ctx->stream));
        ol->staged = true;
        hipLaunchKernelGGL(k_obs_rays, dim3((unsigned int)((R + OBS_RAY_WAVES - 1) / OBS_RAY_WAVES)), dim3(64 * OBS_RAY_WAVES), 0, ctx->stream,
                           (const int8_t*)map->cells, f, (const float*)ol->d_rays, (const float*)(ol->d_rays + ol->ray_cap), R, pose->x, pose->y,
                           pose->theta, p.max_range, (int)p.occ_min, (int)p.tol_cells, ol->n, ol->d_hit, ol->d_clr, ol->d_classes);
        BL_HIP(hipGetLastError());
        if (box.x <= box.z) {
            hipLaunchKernelGGL(k_obs_apply, dim3((unsigned int)((box.z - box.x) / 64 + 1), (unsigned int)((box.w - box.y) / 4 + 1)), dim3(256), 0,
                               ctx->stream, (const uint32_t*)ol->d_hit, (const uint32_t*)ol->d_clr, ol->d_count, ol->d_last, ol->W, box, ol->n,
                               (uint32_t)p.ttl_scans);
            BL_HIP(hipGetLastError());
        }
    }
    BL_HIP(hipEventRecord(ol->ev_ub, ctx->stream));
    return BL_OK;
}

extern "C" int bl_obslayer_compose(bl_obslayer* ol, const bl_grid* map, bl_grid* out)
{
    BL_CHECK_ARG(ol != nullptr && map != nullptr && out != nullptr);
    int rc = obs_need_params(ol);
    if (rc) return rc;
    bl_ctx* ctx = ol->ctx;
    BL_CHECK_ARG(map->ctx == ctx && out->ctx == ctx);
    BL_CHECK_ARG((const bl_grid*)out != map && out->cells != map->cells);
    BL_CHECK_ARG(map->frame.width == ol->W && map->frame.height == ol->H);
    BL_CHECK_ARG(out->frame.width == ol->W && out->frame.height == ol->H);
    BL_HIP(hipSetDevice(ctx->device));
    // the cells are rewritten wholesale: what an upload, a reset and a copy do (bl_internal.h, struct bl_grid)
    out->frame = map->frame;
    out->mirror_valid = false;
    (void)bl_grid_new_lineage(out);
    const size_t cells = (size_t)ol->W * ol->H;
    const size_t threads = cells / 16 + (cells & 15);
    BL_HIP(hipEventRecord(ol->ev_ca, ctx->stream));
    hipLaunchKernelGGL(k_obs_compose, dim3((unsigned int)((threads + 255) / 256)), dim3(256), 0, ctx->stream, (const int8_t*)map->cells,
                       (const uint8_t*)ol->d_count, (const uint32_t*)ol->d_last, out->cells, cells, obs_rule(ol));
    BL_HIP(hipGetLastError());
    BL_HIP(hipEventRecord(ol->ev_cb, ctx->stream));
    ol->composed = true;
    return BL_OK;
}

extern "C" int bl_obslayer_classes(bl_obslayer* ol, uint8_t* out, int* n_rays)
{
    BL_CHECK_ARG(ol != nullptr && n_rays != nullptr);
    BL_HIP(hipSetDevice(ol->ctx->device));
    *n_rays = ol->last_rays;
    if (out && ol->last_rays > 0)
        BL_HIP(hipMemcpyAsync(out, ol->d_classes, (size_t)ol->last_rays, hipMemcpyDeviceToHost, ol->ctx->stream));
    BL_HIP(hipStreamSynchronize(ol->ctx->stream));
    return BL_OK;
}

// the row counts and their prefix on the stream; the totals to the host (synchronises)
static int obs_count(bl_obslayer* ol, int totals[3])
{
    bl_ctx* ctx = ol->ctx;
    BL_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_obs_rowcount, dim3((unsigned int)ol->H), dim3(256), 0, ctx->stream, (const uint8_t*)ol->d_count, (const uint32_t*)ol->d_last,
                       (const uint32_t*)ol->d_hit, (const uint32_t*)ol->d_clr, ol->W, obs_rule(ol), ol->sets_valid ? 1 : 0, ol->d_rows);
    hipLaunchKernelGGL(k_obs_rowscan, dim3(1), dim3(1024), 0, ctx->stream, ol->d_rows, ol->H, ol->d_totals);
    BL_HIP(hipGetLastError());
    BL_HIP(hipMemcpyAsync(totals, ol->d_totals, 3 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    BL_HIP(hipStreamSynchronize(ctx->stream));
    return BL_OK;
}

// the same two launches and the write pass, for a list that stays on the device (bl_obslayer_dev.h)
int obs_live_list_enqueue(bl_obslayer* ol, int32_t* d_xy, int cap)
{
    bl_ctx* ctx = ol->ctx;
    BL_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_obs_rowcount, dim3((unsigned int)ol->H), dim3(256), 0, ctx->stream, (const uint8_t*)ol->d_count, (const uint32_t*)ol->d_last,
                       (const uint32_t*)ol->d_hit, (const uint32_t*)ol->d_clr, ol->W, obs_rule(ol), 0, ol->d_rows);   // the stamps are not read
    hipLaunchKernelGGL(k_obs_rowscan, dim3(1), dim3(1024), 0, ctx->stream, ol->d_rows, ol->H, ol->d_totals);
    hipLaunchKernelGGL(k_obs_livewrite, dim3((unsigned int)ol->H), dim3(256), 0, ctx->stream, (const uint8_t*)ol->d_count, (const uint32_t*)ol->d_last,
                       ol->W, obs_rule(ol), (const int4*)ol->d_rows, d_xy, cap);
    BL_HIP(hipGetLastError());
    return BL_OK;
}

extern "C" int bl_obslayer_stats(bl_obslayer* ol, bl_obslayer_stats_t* out)
{
    BL_CHECK_ARG(ol != nullptr && out != nullptr);
    int rc = obs_need_params(ol);
    if (rc) return rc;
    int totals[3] = {0, 0, 0};
    rc = obs_count(ol, totals);
    if (rc) return rc;
    std::vector<uint8_t> cls((size_t)(ol->last_rays > 0 ? ol->last_rays : 1));
    int rays = 0;
    rc = bl_obslayer_classes(ol, cls.data(), &rays);
    if (rc) return rc;
    memset(out, 0, sizeof(*out));
    out->n = ol->n;
    out->valid_rays = ol->last_valid;
    for (int i = 0; i < rays; ++i) if (cls[(size_t)i] < 5) out->rays_by_class[cls[(size_t)i]] += 1;
    out->hit_cells = totals[1]; out->cleared_cells = totals[2]; out->live_cells = totals[0];
    return BL_OK;
}

extern "C" int bl_obslayer_live_cells(bl_obslayer* ol, int32_t* xy, int cap, int* count)
{
    BL_CHECK_ARG(ol != nullptr && count != nullptr && cap >= 0 && (cap == 0 || xy != nullptr));
    int rc = obs_need_params(ol);
    if (rc) return rc;
    bl_ctx* ctx = ol->ctx;
    int totals[3] = {0, 0, 0};
    rc = obs_count(ol, totals);
    if (rc) return rc;
    *count = totals[0];
    const int m = totals[0] < cap ? totals[0] : cap;
    if (m <= 0) return BL_OK;
    if (m > ol->xy_cap) {
        if (ol->d_xy) { BL_HIP(hipFree(ol->d_xy)); ol->d_xy = nullptr; ol->xy_cap = 0; }
        const size_t c = ((size_t)m + 1023) & ~(size_t)1023;
        BL_HIP(hipMalloc((void**)&ol->d_xy, 2 * c * sizeof(int32_t)));
        ol->xy_cap = (int)c;
    }
    hipLaunchKernelGGL(k_obs_livewrite, dim3((unsigned int)ol->H), dim3(256), 0, ctx->stream, (const uint8_t*)ol->d_count, (const uint32_t*)ol->d_last,
                       ol->W, obs_rule(ol), (const int4*)ol->d_rows, ol->d_xy, m);
    BL_HIP(hipGetLastError());
    BL_HIP(hipMemcpyAsync(xy, ol->d_xy, 2 * (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    BL_HIP(hipStreamSynchronize(ctx->stream));
    return BL_OK;
}

extern "C" int bl_obslayer_download(bl_obslayer* ol, uint8_t* count, uint32_t* last, uint32_t* n)
{
    BL_CHECK_ARG(ol != nullptr);
    bl_ctx* ctx = ol->ctx;
    BL_HIP(hipSetDevice(ctx->device));
    const size_t cells = (size_t)ol->W * ol->H;
    if (count) BL_HIP(hipMemcpyAsync(count, ol->d_count, cells, hipMemcpyDeviceToHost, ctx->stream));
    if (last) BL_HIP(hipMemcpyAsync(last, ol->d_last, cells * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    BL_HIP(hipStreamSynchronize(ctx->stream));
    if (n) *n = ol->n;
    return BL_OK;
}

extern "C" int bl_obslayer_upload(bl_obslayer* ol, const uint8_t* count, const uint32_t* last, uint32_t n)
{
    BL_CHECK_ARG(ol != nullptr && count != nullptr && last != nullptr);
    bl_ctx* ctx = ol->ctx;
    BL_HIP(hipSetDevice(ctx->device));
    const size_t cells = (size_t)ol->W * ol->H;
    BL_HIP(hipMemcpyAsync(ol->d_count, count, cells, hipMemcpyHostToDevice, ctx->stream));
    BL_HIP(hipMemcpyAsync(ol->d_last, last, cells * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    // the stamps speak of updates of the state that is being replaced: any value of theirs could meet the new counter again
    BL_HIP(hipMemsetAsync(ol->d_hit, 0, cells * sizeof(uint32_t), ctx->stream));
    BL_HIP(hipMemsetAsync(ol->d_clr, 0, cells * sizeof(uint32_t), ctx->stream));
    BL_HIP(hipStreamSynchronize(ctx->stream));                          // the caller's arrays are free again
    ol->n = n;
    ol->sets_valid = false;
    return BL_OK;
}

extern "C" int bl_obslayer_last_device_ms(const bl_obslayer* ol, float* update_ms, float* compose_ms)
{
    BL_CHECK_ARG(ol != nullptr);
    if ((update_ms && !ol->updated) || (compose_ms && !ol->composed)) {
        bl_set_error("bl_obslayer_last_device_ms: no %s yet", (update_ms && !ol->updated) ? "bl_obslayer_update" : "bl_obslayer_compose");
        return BL_ERR_STATE;
    }
    if (update_ms) {
        BL_HIP(hipEventSynchronize(ol->ev_ub));
        BL_HIP(hipEventElapsedTime(update_ms, ol->ev_ua, ol->ev_ub));
    }
    if (compose_ms) {
        BL_HIP(hipEventSynchronize(ol->ev_cb));
        BL_HIP(hipEventElapsedTime(compose_ms, ol->ev_ca, ol->ev_cb));
    }
    return BL_OK;
}
