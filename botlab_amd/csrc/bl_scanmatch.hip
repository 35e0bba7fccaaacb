// bl_scanmatch.hip -- correlative scan matching (Olson 2009, exhaustive form): the pose of a scan against the map from a bounded
// window of (dx, dy, dtheta) around a centre pose, without odometry.  The definition is in include/botlab_hip.h; the numpy
// restatement the tests compare with, bit for bit, is "the model" (tests/scan_match_model.py).
//
// One stream-ordered sequence per match on the ctx stream: header + rays H2D, k_sm_raster, k_sm_score, k_sm_final, result D2H.
//   k_sm_raster  one thread per (heading, ray): the ray's endpoint cell at that heading, scoreRay's float arithmetic; endpoints that
//                no shift of the window can bring onto the grid become a sentinel; the bounding box of the others is kept (one
//                vector atomic min / max per wave and bound).
//   k_sm_score   a workgroup owns one heading and a slice of its (dj, di) candidates, lanes along di (row-major over the window), so
//                the lanes of a wave read consecutive bytes of a map row for one ray.  The heading's endpoints are wave-uniform:
//                64 at a time sit one per lane and are broadcast through scalar registers.  When the bounding box widened by the window and
//                clipped to the grid fits in the LDS, the positive part of those cells is staged there (path 0); otherwise the grid is read directly (path 1).
//                Every workgroup leaves its best 64-bit key and how many of its candidates share that key's score.
//   k_sm_final   one workgroup: maximum of the keys (order-independent), sum of the tie counts, the result struct.
#include <string.h>

#include "bl_internal.h"

#define SM_MAX_N 64
#define SM_MAX_NTHETA 180
#define SM_MAX_RAYS 4096
#define SM_LDS_MAX (152 * 1024)        // dynamic LDS a workgroup of k_sm_score may ask for (a CU has 160 KiB)
// x and y of an endpoint that no candidate can bring onto the grid.  2^31 + shift - origin, taken as unsigned, lies below a window's
// or the grid's extent only for an origin within 64 + extent of 2^31 -- in both coordinates at once that would take a grid of 2^60
// cells (bl_grid_create allows 2^31) -- so the scoring loops need no test for it.
#define SM_NONE INT32_MIN
#define SM_MIN_RANGE 0.15f             // moving_laser_scan.cpp:24

// device header of a match: parameters in, bounding box and result out
struct sm_head {
    float cx, cy, ctheta, dtheta;
    int64_t utime;
    int32_t nx, ny, ntheta, rays;
    int32_t min_score, pad;
    int32_t bbox[4];                   // x0, y0 (atomic min), x1, y1 (atomic max) of the endpoints that count
    int32_t score_centre, path;
    bl_scan_match_result_t result;
};

struct sm_block_best { unsigned long long key; uint32_t ties; uint32_t pad; };

struct bl_scanmatch {
    bl_ctx* ctx = nullptr;
    sm_head* d_head = nullptr;
    float* d_rays = nullptr;           // ranges[cap] | thetas[cap]
    int ray_cap = 0;
    int2* d_ends = nullptr; size_t ends_cap = 0;           // [heading][ray]
    sm_block_best* d_best = nullptr; int best_cap = 0;     // one per workgroup of k_sm_score
    int32_t* d_volume = nullptr; size_t volume_cap = 0;
    void* staging = nullptr;           // pinned: sm_head | ranges | thetas
    size_t staging_bytes = 0;
    bool volume_kept = false;
    int vol_nx = 0, vol_ny = 0, vol_nt = 0;
    int last_path = -1;
};

// The candidate order as one unsigned key: score, then small di*di + dj*dj, small |dk|, small dk, small dj, small di.  Given
// d2 and dj, di is known up to its sign, and given |dk|, dk likewise: one bit each (set for the negative, i.e. smaller, value).
__device__ __forceinline__ unsigned long long sm_key(int score, int di, int dj, int dk)
{
    const uint32_t d2 = (uint32_t)(di * di + dj * dj);                 // <= 8192
    const uint32_t adk = (uint32_t)(dk < 0 ? -dk : dk);                // <= 180
    const uint32_t lo = ((16383u - d2) << 18) | ((255u - adk) << 10) | ((dk <= 0 ? 1u : 0u) << 9) | ((uint32_t)(SM_MAX_N - dj) << 1) |
                        (di <= 0 ? 1u : 0u);
    return ((unsigned long long)(uint32_t)score << 32) | lo;
}
__device__ __forceinline__ void sm_key_decode(unsigned long long key, int* score, int* di, int* dj, int* dk)
{
    const uint32_t lo = (uint32_t)key;
    const int d2 = 16383 - (int)(lo >> 18);
    const int adk = 255 - (int)((lo >> 10) & 255u);
    *dk = (lo & 512u) ? -adk : adk;
    *dj = SM_MAX_N - (int)((lo >> 1) & 255u);
    int a = 0;
    while ((a + 1) * (a + 1) <= d2 - *dj * *dj) ++a;                    // at most 64 steps, once per match
    *di = (lo & 1u) ? -a : a;
    *score = (int)(uint32_t)(key >> 32);
}

__device__ __forceinline__ unsigned long long sm_wave_max(unsigned long long v)
{
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}

// ---------------------------------------------------------------------------------------------------------------- rasteriser
__global__ __launch_bounds__(256) void k_sm_raster(sm_head* __restrict__ head, const float* __restrict__ ranges,
                                                   const float* __restrict__ thetas, bl_frame f, int2* __restrict__ ends)
{
    const int rays = head->rays, nt = head->ntheta, nx = head->nx, ny = head->ny;
    const int rp = (rays + 63) & ~63;                                   // rows padded to whole waves of k_sm_score, sentinels in the pad
    const int total = (2 * nt + 1) * rp;
    const int t = blockIdx.x * 256 + threadIdx.x;
    int ex = SM_NONE, ey = SM_NONE;
    const int k = t / rp, r = t - k * rp;
    if (t < total && r < rays) {
        const float theta_k = head->ctheta + (float)(k - nt) * head->dtheta;
        const float a = bl_wrap_to_pi(theta_k - thetas[r]);             // moving_laser_scan.cpp:33
        float sn, cs, sx, sy;
        bl_sincosf_cells(a, &sn, &cs);
        bl_global_to_grid(head->cx, head->cy, f, &sx, &sy);
        const float range = ranges[r];
        const float fx = range * cs * f.cpm + sx;                       // sensor_model.cpp:34-35
        const float fy = range * sn * f.cpm + sy;
        // beyond +-2^30 (or NaN) the endpoint is nowhere near a grid: it counts nothing, and the conversion is never asked for it
        if (__builtin_fabsf(fx) < 0x1p30f && __builtin_fabsf(fy) < 0x1p30f) {
            const int ix = (int)fx, iy = (int)fy;
            if (ix >= -nx && ix < f.width + nx && iy >= -ny && iy < f.height + ny) { ex = ix; ey = iy; }
        }
    }
    if (t < total) ends[t] = make_int2(ex, ey);
    const bool on = ex != SM_NONE;
    int x0 = on ? ex : INT32_MAX, y0 = on ? ey : INT32_MAX, x1 = on ? ex : INT32_MIN, y1 = on ? ey : INT32_MIN;
    for (int off = 32; off > 0; off >>= 1) {
        x0 = min(x0, __shfl_xor(x0, off, 64)); y0 = min(y0, __shfl_xor(y0, off, 64));
        x1 = max(x1, __shfl_xor(x1, off, 64)); y1 = max(y1, __shfl_xor(y1, off, 64));
    }
    if ((threadIdx.x & 63) == 0 && x1 >= x0) {
        atomicMin(&head->bbox[0], x0); atomicMin(&head->bbox[1], y0);
        atomicMax(&head->bbox[2], x1); atomicMax(&head->bbox[3], y1);
    }
}

// ---------------------------------------------------------------------------------------------------------------- scoring
// the map window of a match: the endpoints' bounding box widened by the shifts, clipped to the grid; x0 a multiple of four when the
// rows can be copied a dword at a time
struct sm_window { int x0, y0, w, h, pitch; bool any, dwords; };

__device__ __forceinline__ sm_window sm_make_window(const sm_head* head, const bl_frame& f)
{
    sm_window win;
    const int bx0 = head->bbox[0], by0 = head->bbox[1], bx1 = head->bbox[2], by1 = head->bbox[3];
    win.any = bx1 >= bx0;
    win.dwords = (f.width & 3) == 0;
    int x0 = max(bx0 - head->nx, 0), x1 = min(bx1 + head->nx, f.width - 1);
    int y0 = max(by0 - head->ny, 0), y1 = min(by1 + head->ny, f.height - 1);
    if (win.dwords) x0 &= ~3;
    win.any = win.any && x1 >= x0 && y1 >= y0;
    win.x0 = x0; win.y0 = y0;
    win.w = win.any ? x1 - x0 + 1 : 0; win.h = win.any ? y1 - y0 + 1 : 0;
    win.pitch = (win.w + 3) & ~3;
    return win;
}

__device__ __forceinline__ uint32_t sm_positive_bytes(uint32_t v)       // max(0, b) of four signed bytes
{
    const uint32_t neg = (v >> 7) & 0x01010101u;
    return v & ~(neg * 0xffu);
}

// grid: (slices, headings).  Dynamic LDS: uint8 window[lds_window_bytes].
__global__ __launch_bounds__(1024) void k_sm_score(sm_head* __restrict__ head, const int8_t* __restrict__ cells, bl_frame f,
                                                    const int2* __restrict__ ends, int lds_window_bytes,
                                                    sm_block_best* __restrict__ best, int32_t* __restrict__ volume)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    __shared__ unsigned long long s_key[16];
    __shared__ uint32_t s_ties[16];
    const int rays = head->rays, nt = head->ntheta, nx = head->nx, ny = head->ny;
    const int k = blockIdx.y, dk = k - nt;
    const int tid = threadIdx.x, nthreads = blockDim.x;
    unsigned char* s_win = s_raw;
    const int rp = (rays + 63) & ~63;                                   // a heading's row of endpoints, padded with sentinels
    const int2* __restrict__ k_ends = ends + (size_t)k * rp;
    const int wave = tid >> 6, lane = tid & 63;

    const sm_window win = sm_make_window(head, f);
    const bool staged = (long long)win.pitch * win.h <= (long long)lds_window_bytes;          // uniform over the whole launch
    if (staged && win.any) {
        if (win.dwords) {
            const int qw = win.pitch >> 2;                              // x0 and the grid width are multiples of four: whole dwords lie inside the row
            for (int i = tid; i < qw * win.h; i += nthreads) {
                const int row = i / qw, q = i - row * qw;
                const uint32_t v = *(const uint32_t*)(cells + (size_t)(win.y0 + row) * f.width + win.x0 + 4 * q);
                *(uint32_t*)(s_win + row * win.pitch + 4 * q) = sm_positive_bytes(v);
            }
        } else {
            for (int i = tid; i < win.pitch * win.h; i += nthreads) {
                const int row = i / win.pitch, col = i - row * win.pitch;
                int v = 0;
                if (col < win.w) v = cells[(size_t)(win.y0 + row) * f.width + win.x0 + col];
                s_win[i] = (unsigned char)(v > 0 ? v : 0);
            }
        }
    }
    __syncthreads();

    const int cw = 2 * nx + 1, ncand = cw * (2 * ny + 1);
    const int per = (ncand + gridDim.x - 1) / gridDim.x;                // candidates of this slice
    const int c_begin = blockIdx.x * per, c_end = min(ncand, c_begin + per);
    unsigned long long key = 0;
    int top = -1; uint32_t ties = 0;
    for (int cb = c_begin + (tid & ~63); cb < c_end; cb += nthreads) {       // wave-uniform trip count: the broadcasts need every lane
        const int c = cb + lane;
        const int jrow = c / cw;
        const int di = c - jrow * cw - nx, dj = jrow - ny;
        int acc = 0;
        // 64 endpoints at a time, one per lane, the next 64 on their way; each is then broadcast through a scalar register pair
        int2 mine = rp > 0 ? k_ends[lane] : make_int2(SM_NONE, SM_NONE);
        for (int r0 = 0; r0 < rp; r0 += 64) {
            int2 next = mine;
            if (r0 + 64 < rp) next = k_ends[r0 + 64 + lane];
            if (staged) {
                const unsigned ox = (unsigned)(di - win.x0), oy = (unsigned)(dj - win.y0);
#pragma unroll
                for (int i = 0; i < 64; ++i) {
                    const int ex = __builtin_amdgcn_readlane(mine.x, i), ey = __builtin_amdgcn_readlane(mine.y, i);
                    const unsigned ux = (unsigned)ex + ox, uy = (unsigned)ey + oy;
                    const bool in = ux < (unsigned)win.w && uy < (unsigned)win.h;      // never true for a sentinel (see SM_NONE)
                    const int v = s_win[in ? uy * (unsigned)win.pitch + ux : 0u];      // no branch: the reads of a batch overlap
                    acc += in ? v : 0;
                }
            } else {
#pragma unroll
                for (int i = 0; i < 64; ++i) {
                    const int ex = __builtin_amdgcn_readlane(mine.x, i), ey = __builtin_amdgcn_readlane(mine.y, i);
                    const unsigned x = (unsigned)ex + (unsigned)di, y = (unsigned)ey + (unsigned)dj;
                    const bool in = x < (unsigned)f.width && y < (unsigned)f.height;
                    const int v = cells[in ? (size_t)y * f.width + x : (size_t)0];
                    acc += (in && v > 0) ? v : 0;
                }
            }
            mine = next;
        }
        if (c >= c_end) continue;
        if (volume) volume[(size_t)k * ncand + c] = acc;
        if (dk == 0 && di == 0 && dj == 0) head->score_centre = acc;
        const unsigned long long kc = sm_key(acc, di, dj, dk);
        key = kc > key ? kc : key;
        if (acc > top) { top = acc; ties = 1; } else if (acc == top) ++ties;
    }
    // the workgroup's best key, and how many of its candidates share that score
    const unsigned long long wkey = sm_wave_max(key);
    if (lane == 0) s_key[wave] = wkey;
    __syncthreads();
    unsigned long long bkey = 0;
    for (int w = 0; w < (nthreads >> 6); ++w) bkey = s_key[w] > bkey ? s_key[w] : bkey;
    uint32_t n = (top >= 0 && (uint32_t)top == (uint32_t)(bkey >> 32)) ? ties : 0;
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, 64);
    if (lane == 0) s_ties[wave] = n;
    __syncthreads();
    if (tid == 0) {
        uint32_t total = 0;
        for (int w = 0; w < (nthreads >> 6); ++w) total += s_ties[w];
        sm_block_best b; b.key = bkey; b.ties = (c_end > c_begin) ? total : 0; b.pad = 0;
        best[blockIdx.y * gridDim.x + blockIdx.x] = b;
        if (blockIdx.x == 0 && blockIdx.y == 0) head->path = staged ? 0 : 1;
    }
}

// ---------------------------------------------------------------------------------------------------------------- result
__global__ __launch_bounds__(256) void k_sm_final(sm_head* __restrict__ head, const sm_block_best* __restrict__ best, int nblocks,
                                                  bl_frame f)
{
    __shared__ unsigned long long s_key[4];
    __shared__ uint32_t s_ties[4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    unsigned long long key = 0;
    for (int i = tid; i < nblocks; i += 256) { const unsigned long long b = best[i].key; key = b > key ? b : key; }
    key = sm_wave_max(key);
    if (lane == 0) s_key[wave] = key;
    __syncthreads();
    key = 0;
    for (int w = 0; w < 4; ++w) key = s_key[w] > key ? s_key[w] : key;
    uint32_t n = 0;
    for (int i = tid; i < nblocks; i += 256) {
        const sm_block_best b = best[i];
        if (b.ties && (uint32_t)(b.key >> 32) == (uint32_t)(key >> 32)) n += b.ties;
    }
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, 64);
    if (lane == 0) s_ties[wave] = n;
    __syncthreads();
    if (tid == 0) {
        int score, di, dj, dk;
        sm_key_decode(key, &score, &di, &dj, &dk);
        bl_scan_match_result_t r;
        r.di = di; r.dj = dj; r.dk = dk;
        r.score = score;
        r.score_centre = head->score_centre;
        r.ties = (int32_t)(s_ties[0] + s_ties[1] + s_ties[2] + s_ties[3]);
        r.rays_used = head->rays;
        r.accepted = score >= head->min_score ? 1 : 0;
        r.pose.utime = head->utime;
        if (r.accepted) {
            r.pose.x = (float)((double)head->cx + (double)di * (double)f.mpc);
            r.pose.y = (float)((double)head->cy + (double)dj * (double)f.mpc);
            r.pose.theta = bl_wrap_to_pi(head->ctheta + (float)dk * head->dtheta);
        } else {
            r.pose.x = head->cx; r.pose.y = head->cy; r.pose.theta = head->ctheta;
        }
        head->result = r;
    }
}

// ---------------------------------------------------------------------------------------------------------------- host
extern "C" int bl_scanmatch_create(bl_ctx* ctx, bl_scanmatch** out)
{
    BL_CHECK_ARG(ctx != nullptr && out != nullptr);
    BL_HIP(hipSetDevice(ctx->device));
    // per create: the attribute belongs to the current device, and contexts of several devices and threads make matchers
    BL_HIP(hipFuncSetAttribute((const void*)k_sm_score, hipFuncAttributeMaxDynamicSharedMemorySize, SM_LDS_MAX));
    bl_scanmatch* sm = new bl_scanmatch();
    sm->ctx = ctx;
    hipError_t e = hipMalloc((void**)&sm->d_head, sizeof(sm_head));
    if (e != hipSuccess) { bl_set_error("hipMalloc failed: %s", hipGetErrorString(e)); delete sm; return BL_ERR_HIP; }
    *out = sm;
    return BL_OK;
}

extern "C" void bl_scanmatch_destroy(bl_scanmatch* sm)
{
    if (!sm) return;
    (void)hipStreamSynchronize(sm->ctx->stream);
    (void)hipFree(sm->d_head); (void)hipFree(sm->d_rays); (void)hipFree(sm->d_ends); (void)hipFree(sm->d_best); (void)hipFree(sm->d_volume);
    if (sm->staging) (void)hipHostFree(sm->staging);
    delete sm;
}

template <typename T>
static int sm_grow(T** p, size_t* cap, size_t need)
{
    if (need <= *cap) return BL_OK;
    if (*p) { BL_HIP(hipFree(*p)); *p = nullptr; *cap = 0; }
    BL_HIP(hipMalloc((void**)p, need * sizeof(T)));
    *cap = need;
    return BL_OK;
}

extern "C" int bl_scanmatch_match(bl_scanmatch* sm, const bl_grid* map, const bl_lidar_t* scan, const bl_pose_xyt_t* centre,
                                  const bl_scan_match_params_t* params, bl_scan_match_result_t* result)
{
    BL_CHECK_ARG(sm != nullptr);
    sm->volume_kept = false;           // "the last match" includes a refused one: bl_scanmatch_volume then answers BL_ERR_STATE
    BL_CHECK_ARG(map != nullptr && scan != nullptr && centre != nullptr && params != nullptr && result != nullptr);
    BL_CHECK_ARG(map->ctx == sm->ctx);
    BL_CHECK_ARG(params->nx >= 0 && params->nx <= SM_MAX_N && params->ny >= 0 && params->ny <= SM_MAX_N);
    BL_CHECK_ARG(params->ntheta >= 0 && params->ntheta <= SM_MAX_NTHETA);
    BL_CHECK_ARG(params->dtheta > 0.0f);
    BL_CHECK_ARG(scan->num_ranges >= 0 && (scan->num_ranges == 0 || (scan->ranges != nullptr && scan->thetas != nullptr)));
    int rays = 0;
    for (int i = 0; i < scan->num_ranges; ++i) rays += (scan->ranges[i] > SM_MIN_RANGE && scan->ranges[i] < params->max_range) ? 1 : 0;
    BL_CHECK_ARG(rays <= SM_MAX_RAYS);
    bl_ctx* ctx = sm->ctx;
    BL_HIP(hipSetDevice(ctx->device));

    // ---- buffers
    const int nk = 2 * params->ntheta + 1, cw = 2 * params->nx + 1, ch = 2 * params->ny + 1, ncand = cw * ch;
    const int cap = rays > 0 ? rays : 1;
    if (cap > sm->ray_cap) {
        size_t c = 0;
        BL_HIP(hipStreamSynchronize(ctx->stream));
        if (sm->d_rays) { BL_HIP(hipFree(sm->d_rays)); sm->d_rays = nullptr; sm->ray_cap = 0; }
        if (sm->staging) { BL_HIP(hipHostFree(sm->staging)); sm->staging = nullptr; }
        c = (size_t)((cap + 255) & ~255);
        BL_HIP(hipMalloc((void**)&sm->d_rays, 2 * c * sizeof(float)));
        sm->staging_bytes = sizeof(sm_head) + 2 * c * sizeof(float);
        BL_HIP(hipHostMalloc(&sm->staging, sm->staging_bytes, hipHostMallocDefault));
        sm->ray_cap = (int)c;
    }
    const int rp = (rays + 63) & ~63;
    int rc = sm_grow(&sm->d_ends, &sm->ends_cap, (size_t)nk * (rp > 0 ? rp : 64));
    if (rc) return rc;
    // slices of a heading's candidates: enough workgroups to fill the device, none with less than a wave of candidates
    const int threads = ncand >= 4096 ? 1024 : 256;
    int slices = (1024 + nk - 1) / nk;
    const int max_slices = (ncand + threads - 1) / threads;
    if (slices > max_slices) slices = max_slices;
    if (slices < 1) slices = 1;
    const int nblocks = slices * nk;
    { size_t bc = (size_t)sm->best_cap; rc = sm_grow(&sm->d_best, &bc, (size_t)nblocks); sm->best_cap = (int)bc; if (rc) return rc; }
    if (params->keep_volume) { rc = sm_grow(&sm->d_volume, &sm->volume_cap, (size_t)nk * ncand); if (rc) return rc; }

    // ---- header and the valid rays, one copy
    sm_head* h = (sm_head*)sm->staging;
    float* h_ranges = (float*)((char*)sm->staging + sizeof(sm_head));
    float* h_thetas = h_ranges + sm->ray_cap;
    memset(h, 0, sizeof(sm_head));
    h->cx = centre->x; h->cy = centre->y; h->ctheta = centre->theta; h->dtheta = params->dtheta;
    h->utime = scan->utime;
    h->nx = params->nx; h->ny = params->ny; h->ntheta = params->ntheta; h->rays = rays;
    h->min_score = params->min_score;
    h->bbox[0] = INT32_MAX; h->bbox[1] = INT32_MAX; h->bbox[2] = INT32_MIN; h->bbox[3] = INT32_MIN;
    float rmax = 0;
    for (int i = 0, j = 0; i < scan->num_ranges; ++i) {
        const float r = scan->ranges[i];
        if (r > SM_MIN_RANGE && r < params->max_range) { h_ranges[j] = r; h_thetas[j] = scan->thetas[i]; ++j; if (r > rmax) rmax = r; }
    }
    BL_HIP(hipMemcpyAsync(sm->d_head, h, sizeof(sm_head), hipMemcpyHostToDevice, ctx->stream));
    if (rays > 0)
        BL_HIP(hipMemcpyAsync(sm->d_rays, h_ranges, 2 * (size_t)sm->ray_cap * sizeof(float), hipMemcpyHostToDevice, ctx->stream));

    // ---- LDS for the window: an upper bound of what the device will find (every endpoint lies within the longest range, a cell of
    // slack for each rounding, of the centre; the window is that box widened by the shifts, clipped to the grid).  The device
    // compares the window it really needs with what it was given, so an optimistic bound could only cost the staging.
    const bl_frame& f = map->frame;
    const double reach = (double)rmax * (double)f.cpm + 3.0;
    double bw = 2.0 * reach + 1.0 + 2.0 * params->nx + 4.0, bh = 2.0 * reach + 1.0 + 2.0 * params->ny;
    if (!(bw < (double)f.width)) bw = (double)f.width;                  // also catches NaN
    if (!(bh < (double)f.height)) bh = (double)f.height;
    const size_t win_bytes = (size_t)(((int)bw + 3) & ~3) * (size_t)(int)bh;
    int lds_window = 0;
    if (win_bytes <= (size_t)SM_LDS_MAX) lds_window = (int)win_bytes;
    const size_t lds_bytes = (size_t)(lds_window > 16 ? lds_window : 16);   // never empty: a masked-out lookup reads byte 0

    const int total = nk * rp;
    if (total > 0)
        hipLaunchKernelGGL(k_sm_raster, dim3((total + 255) / 256), dim3(256), 0, ctx->stream, sm->d_head, sm->d_rays,
                           sm->d_rays + sm->ray_cap, f, sm->d_ends);
    hipLaunchKernelGGL(k_sm_score, dim3(slices, nk), dim3(threads), lds_bytes, ctx->stream, sm->d_head, map->cells, f, sm->d_ends,
                       lds_window, sm->d_best, params->keep_volume ? sm->d_volume : (int32_t*)nullptr);
    hipLaunchKernelGGL(k_sm_final, dim3(1), dim3(256), 0, ctx->stream, sm->d_head, sm->d_best, nblocks, f);
    BL_HIP(hipGetLastError());
    BL_HIP(hipMemcpyAsync(h, sm->d_head, sizeof(sm_head), hipMemcpyDeviceToHost, ctx->stream));
    BL_HIP(hipStreamSynchronize(ctx->stream));
    *result = h->result;
    sm->last_path = h->path;
    if (params->keep_volume) { sm->volume_kept = true; sm->vol_nx = params->nx; sm->vol_ny = params->ny; sm->vol_nt = params->ntheta; }
    return BL_OK;
}

extern "C" int bl_scanmatch_volume(bl_scanmatch* sm, int32_t* scores)
{
    BL_CHECK_ARG(sm != nullptr && scores != nullptr);
    if (!sm->volume_kept) { bl_set_error("bl_scanmatch_volume: the last match did not keep its score volume"); return BL_ERR_STATE; }
    BL_HIP(hipSetDevice(sm->ctx->device));
    const size_t n = (size_t)(2 * sm->vol_nt + 1) * (2 * sm->vol_ny + 1) * (2 * sm->vol_nx + 1);
    BL_HIP(hipMemcpyAsync(scores, sm->d_volume, n * sizeof(int32_t), hipMemcpyDeviceToHost, sm->ctx->stream));
    BL_HIP(hipStreamSynchronize(sm->ctx->stream));
    return BL_OK;
}

extern "C" int bl_scanmatch_debug_path(const bl_scanmatch* sm)
{
    return sm ? sm->last_path : -1;
}
