// bl_scanmatch_dev.h -- what the correlative matchers share: bl_scanmatch.hip (the plain and prior match, the wide match) and
// bl_rbslam_match.h (a match per particle against its own map) score the same definition (include/botlab_hip.h, "correlative scan
// matching"; tests/scan_match_model.py); each rule lives here once.
//   device  the candidate order as one key; the positive part of map bytes; the map window (clip, staging into LDS); the endpoint cell
//           of a ray at a heading; the sum of a heading's endpoints over a byte image; a workgroup's best key and tie count; the pose
//           of the winner
//   host    which rays of a scan count, counted and packed
// What differs stays where it was: where a window's box comes from, each kernel's LDS layout and barriers, the wide match's two-word
// key and its reduction, the sentinels and on-grid tests of the endpoints.
#ifndef BL_SCANMATCH_DEV_H
#define BL_SCANMATCH_DEV_H

#include "bl_internal.h"

#define SM_MAX_N 64
// x and y of an endpoint that no candidate can bring onto the grid.  2^31 + shift - origin, taken as unsigned, lies below a window's
// or the grid's extent only for an origin within 64 + extent of 2^31 -- in both coordinates at once that would take a grid of 2^60
// cells (bl_grid_create allows 2^31) -- so the scoring loops need no test for it.
#define SM_NONE INT32_MIN
#define SM_MIN_RANGE 0.15f             // moving_laser_scan.cpp:24

// ---------------------------------------------------------------------------------------------------------------- the key
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

// A workgroup's best key and how many of its candidates share that key's score.  Every thread comes with the best key of its own
// candidates, their top score as a key's high word holds it, and how many of them have it (0 for a thread without candidates).
// Two barriers; s_key and s_ties have a slot per wave.  The key is returned to every thread, the count to thread 0 only.
struct sm_best { unsigned long long key; uint32_t ties; };
__device__ __forceinline__ sm_best sm_block_best_key(unsigned long long key, uint32_t top_word, uint32_t ties, int nwaves,
                                                     unsigned long long* s_key, uint32_t* s_ties)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned long long wkey = sm_wave_max(key);
    if (lane == 0) s_key[wave] = wkey;
    __syncthreads();
    sm_best b; b.key = 0; b.ties = 0;
    for (int w = 0; w < nwaves; ++w) b.key = s_key[w] > b.key ? s_key[w] : b.key;
    uint32_t n = top_word == (uint32_t)(b.key >> 32) ? ties : 0;
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, 64);
    if (lane == 0) s_ties[wave] = n;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 0; w < nwaves; ++w) b.ties += s_ties[w];
    return b;
}

// ---------------------------------------------------------------------------------------------------------------- the map window
__device__ __forceinline__ uint32_t sm_positive_bytes(uint32_t v)       // max(0, b) of four signed bytes
{
    const uint32_t neg = (v >> 7) & 0x01010101u;
    return v & ~(neg * 0xffu);
}

// the map cells a match can read: an inclusive box clipped to the grid; x0 a multiple of four when the rows can be copied a dword
// at a time
struct sm_window { int x0, y0, w, h, pitch; bool any, dwords; };

__device__ __forceinline__ sm_window sm_clip_window(int bx0, int by0, int bx1, int by1, bool any, const bl_frame& f)
{
    sm_window win;
    win.dwords = (f.width & 3) == 0;
    int x0 = max(bx0, 0), x1 = min(bx1, f.width - 1);
    int y0 = max(by0, 0), y1 = min(by1, f.height - 1);
    if (win.dwords) x0 &= ~3;
    win.any = any && x1 >= x0 && y1 >= y0;
    win.x0 = x0; win.y0 = y0;
    win.w = win.any ? x1 - x0 + 1 : 0; win.h = win.any ? y1 - y0 + 1 : 0;
    win.pitch = (win.w + 3) & ~3;
    return win;
}

// The positive part of the window's cells to LDS, rows at win.pitch, by every thread of the workgroup (the caller has the barrier).
// Dwords: x0 and the grid width are multiples of four, so whole dwords lie inside the row; a window as wide as the grid is one
// run of them and needs no row arithmetic.  Otherwise bytes, the pad of a row zero.
__device__ __forceinline__ void sm_stage_window(const int8_t* __restrict__ cells, int width, const sm_window& win, unsigned char* s_win,
                                                int tid, int nthreads)
{
    if (win.dwords) {
        const int qw = win.pitch >> 2;
        if (win.pitch == width) {
            const uint32_t* __restrict__ src = (const uint32_t*)(cells + (size_t)win.y0 * width);
            for (int i = tid; i < qw * win.h; i += nthreads) ((uint32_t*)s_win)[i] = sm_positive_bytes(src[i]);
            return;
        }
        for (int i = tid; i < qw * win.h; i += nthreads) {
            const int row = i / qw, q = i - row * qw;
            const uint32_t v = *(const uint32_t*)(cells + (size_t)(win.y0 + row) * width + win.x0 + 4 * q);
            *(uint32_t*)(s_win + row * win.pitch + 4 * q) = sm_positive_bytes(v);
        }
    } else {
        for (int i = tid; i < win.pitch * win.h; i += nthreads) {
            const int row = i / win.pitch, col = i - row * win.pitch;
            int v = 0;
            if (col < win.w) v = cells[(size_t)(win.y0 + row) * width + win.x0 + col];
            s_win[i] = (unsigned char)(v > 0 ? v : 0);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- endpoints
// The cell of a ray's endpoint at heading theta_k, seen from (sx, sy) in cells: scoreRay's float arithmetic.  false: beyond +-2^30
// (or NaN) the endpoint is nowhere near a grid; it counts nothing, and the conversion is never asked for it.
__device__ __forceinline__ bool sm_endpoint(float range, float ray_theta, float theta_k, float sx, float sy, const bl_frame& f, int* ix,
                                            int* iy)
{
    const float a = bl_wrap_to_pi(theta_k - ray_theta);                 // moving_laser_scan.cpp:33
    float sn, cs;
    bl_sincosf_cells(a, &sn, &cs);
    const float fx = range * cs * f.cpm + sx;                           // sensor_model.cpp:34-35
    const float fy = range * sn * f.cpm + sy;
    if (!(__builtin_fabsf(fx) < 0x1p30f && __builtin_fabsf(fy) < 0x1p30f)) return false;
    *ix = (int)fx; *iy = (int)fy;
    return true;
}

// sum over a heading's endpoints of bytes[(ey + oy) * pitch + ex + ox] where that lies inside w x h; all 64 lanes of the wave must
// be here: 64 endpoints at a time sit one per lane, the next 64 on their way, and each is broadcast through a scalar register pair.
// SIGNED: the bytes are int8 log-odds and only the positive count.
template <bool SIGNED>
__device__ __forceinline__ int sm_lookup_sum(const int2* __restrict__ k_ends, int rp, int lane, unsigned ox, unsigned oy,
                                             const unsigned char* __restrict__ bytes, unsigned w, unsigned h, unsigned pitch)
{
    int acc = 0;
    int2 mine = rp > 0 ? k_ends[lane] : make_int2(SM_NONE, SM_NONE);
    for (int r0 = 0; r0 < rp; r0 += 64) {
        int2 next = mine;
        if (r0 + 64 < rp) next = k_ends[r0 + 64 + lane];
#pragma unroll
        for (int i = 0; i < 64; ++i) {
            const int ex = __builtin_amdgcn_readlane(mine.x, i), ey = __builtin_amdgcn_readlane(mine.y, i);
            const unsigned ux = (unsigned)ex + ox, uy = (unsigned)ey + oy;
            const bool in = ux < w && uy < h;                               // never true for a sentinel (see SM_NONE; shifts <= 4096 + 63)
            const unsigned char b = bytes[in ? (size_t)uy * pitch + ux : (size_t)0];     // no branch: the reads of a batch overlap
            const int v = SIGNED ? (int)(signed char)b : (int)b;
            acc += (in && (!SIGNED || v > 0)) ? v : 0;
        }
        mine = next;
    }
    return acc;
}

// ---------------------------------------------------------------------------------------------------------------- the result
// the pose of candidate (di, dj, dk) around the centre when the match moves there, the centre as it is otherwise
__device__ __forceinline__ void sm_result_pose(bool moved, float cx, float cy, float ctheta, int di, int dj, int dk, float mpc, float dtheta,
                                               float* x, float* y, float* theta)
{
    *x = cx; *y = cy; *theta = ctheta;
    if (moved) {
        *x = (float)((double)cx + (double)di * (double)mpc);
        *y = (float)((double)cy + (double)dj * (double)mpc);
        *theta = bl_wrap_to_pi(ctheta + (float)dk * dtheta);
    }
}

// ---------------------------------------------------------------------------------------------------------------- host
// The rays of a scan that count (min range < range < max_range), in scan order: how many, and the largest.  With `ranges` they are
// packed there and their thetas into `thetas`; without, only counted.
BL_HD bool sm_ray_valid(float range, float max_range) { return range > SM_MIN_RANGE && range < max_range; }
static inline int sm_valid_rays(const bl_lidar_t* scan, float max_range, float* ranges, float* thetas, float* reach)
{
    int n = 0;
    float longest = 0;
    for (int i = 0; i < scan->num_ranges; ++i) {
        const float r = scan->ranges[i];
        if (!sm_ray_valid(r, max_range)) continue;
        if (ranges) { ranges[n] = r; thetas[n] = scan->thetas[i]; }
        if (r > longest) longest = r;
        ++n;
    }
    if (reach) *reach = longest;
    return n;
}

#endif  // BL_SCANMATCH_DEV_H
