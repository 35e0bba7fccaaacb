// bl_mapray_dev.h -- what the map updates share.  Mapping::updateMap (src/slam/mapping.cpp:17-127, the reference's inverse sensor
// model) runs as k_map_update (bl_mapping.hip: one map at the filter's pose), k_rb_map (bl_rbslam.hip: a map per particle) and
// k_rl_rays / k_rl_fold (bl_scanlog.hip: a map from K recorded scans); k_obs_rays (bl_obslayer.hip) takes cells of the same walk.
// All of them must produce the reference's cells bit for bit, so each rule that decides a cell lives here once.
//   host and device  the start and end cell of a ray; the closed-form Bresenham walk from any step k0
//   device           a workgroup's bounding box; the packed uint16 counter pairs; the segment table's count and search; four
//                    counters applied to four cells of a grid dword
// What differs stays where it was: each kernel's constants (segment length, tile sizes, thread counts), its LDS layout and
// barriers, mapping's look-ahead, leaders and strips, RB-SLAM's tiling, the scan log's fold.
// tests/cpp/mapray_ref.cpp compiles the first part for the host (tests/test_mapray_header_cpu.py).
#ifndef BL_MAPRAY_DEV_H
#define BL_MAPRAY_DEV_H

#include "bl_math.h"

#if !defined(__HIPCC__)
struct int4 { int x, y, z, w; };
inline int4 make_int4(int x, int y, int z, int w) { int4 v = {x, y, z, w}; return v; }
#endif

// ---------------------------------------------------------------------------------------------------------------- ray geometry
#define BL_NO_RAY 0x7fffffff                 // x of a ray that takes no part
#define BL_RAY_CELL_LIMIT (1 << 24)          // |cell coordinate| bound for a ray to be traced (rejects NaN / inf geometry)

// Start cell and end cell of one ray (moving_laser_scan.cpp:22-37, mapping.cpp:45-49) as (x0, y0, x1, y1); x == BL_NO_RAY: the
// ray takes no part.  It comes in two parts.  What depends on the poses' THETA alone -- the interpolated theta does not depend on
// x or y --: the ray's reach in cells along both axes (wrap, sine and cosine, two products each).  And what depends on their
// POSITION.  A map update that ran ahead of the filter's exact x, y checks its cells with the second part alone.
// The scan is traced from pose pb to pose pe; interp: their utimes differ, and a ray stamped ray_time leaves from the pose at
// ratio (ray_time - t_begin) / t_den between them, otherwise from pe.  Rays with range <= 0.15f were dropped on the host.
struct bl_ray_reach { float ex, ey; double ratio; bool on; };
BL_HD bl_ray_reach bl_ray_angle(const bl_frame& f, float max_laser, bool interp, int64_t t_begin, double t_den, const bl_pose3& pb,
                                const bl_pose3& pe, float range, float ray_theta, int64_t ray_time)
{
    bl_ray_reach d = {0.0f, 0.0f, 0.0, range <= max_laser};
    if (d.on) {
        if (interp) d.ratio = bl_interp_ratio(ray_time, t_begin, t_den);
        const float rp_theta = interp ? bl_interpolate_pose(pb, pe, d.ratio).theta : pe.theta;
        float theta = bl_wrap_to_pi(rp_theta - ray_theta);
        float sn, cs;
        bl_sincosf(theta, &sn, &cs);
        d.ex = range * cs * f.cpm;
        d.ey = range * sn * f.cpm;
    }
    return d;
}
BL_HD int4 bl_ray_place(const bl_frame& f, bool interp, const bl_pose3& pb, const bl_pose3& pe, const bl_ray_reach& d)
{
    int4 ray = make_int4(BL_NO_RAY, 0, 0, 0);
    if (d.on) {
        const bl_pose3 rp = interp ? bl_interpolate_pose(pb, pe, d.ratio) : pe;
        float sx, sy;
        bl_global_to_grid(rp.x, rp.y, f, &sx, &sy);
        float fx = d.ex + sx;
        float fy = d.ey + sy;
        const float lim = (float)BL_RAY_CELL_LIMIT;
        if (fx > -lim && fx < lim && fy > -lim && fy < lim && sx > -lim && sx < lim && sy > -lim && sy < lim)
            ray = make_int4((int)sx, (int)sy, (int)fx, (int)fy);        // float -> int truncation at the bresenham() call
    }
    return ray;
}
BL_HD int4 bl_ray_cells(const bl_frame& f, float max_laser, bool interp, int64_t t_begin, double t_den, const bl_pose3& pb, const bl_pose3& pe,
                        float range, float ray_theta, int64_t ray_time)
{
    return bl_ray_place(f, interp, pb, pe, bl_ray_angle(f, max_laser, interp, t_begin, t_den, pb, pe, range, ray_theta, ray_time));
}

// ---------------------------------------------------------------------------------------------------------------- the walk
// Cell k (k = 0 .. K - 1, K = max(dx, dy); start cell included, end cell excluded) of the reference's Bresenham walk
// (mapping.cpp:101-127: e2 = 2*err; if (e2 >= -dy) {err -= dy; x += sx;} if (e2 <= dx) {err += dx; y += sy;}) has a closed
// form: the major axis advances k, the minor axis n = floor((2 k dmin + dmaj) / (2 dmaj)).  So the walk of one ray can start at
// any k0 with one division and go on with the remainder: rem += 2 dmin, carrying into n at 2 dmaj.
// Widths.  BL_RAY_CELL_LIMIT bounds dmin <= dmaj < 2^25, so rem < 2 dmaj, 2 dmin and their sum (< 2^27) are carried as int.
// Only the start's numerator 2 k0 dmin + dmaj outgrows 32 bits: below dmaj = 32768 it stays under 2^31 + 2^15 and is divided as
// unsigned int, from there on as long long (a 64-bit division costs a few hundred instructions on the device).
BL_HD int bl_ray_steps(const int4 ray)
{
    const int dx = ray.z > ray.x ? ray.z - ray.x : ray.x - ray.z, dy = ray.w > ray.y ? ray.w - ray.y : ray.y - ray.w;
    return dx > dy ? dx : dy;
}

struct bl_walk { int x0, y0, sx, sy, dmaj, dmin, k, n, rem; bool xmajor; };

// the walker at cell k0 of `ray` (a traced ray with 0 <= k0 < K, so dmaj > 0)
BL_HD bl_walk bl_walk_begin(const int4 ray, int k0)
{
    bl_walk w;
    const int dx = ray.z > ray.x ? ray.z - ray.x : ray.x - ray.z, dy = ray.w > ray.y ? ray.w - ray.y : ray.y - ray.w;
    w.x0 = ray.x; w.y0 = ray.y;
    w.sx = ray.x < ray.z ? 1 : -1; w.sy = ray.y < ray.w ? 1 : -1;
    w.xmajor = dx >= dy;
    w.dmaj = w.xmajor ? dx : dy; w.dmin = w.xmajor ? dy : dx;
    w.k = k0;
    if (w.dmaj < 32768) {
        const unsigned int num = 2u * (unsigned int)k0 * (unsigned int)w.dmin + (unsigned int)w.dmaj;
        w.n = (int)(num / (2u * (unsigned int)w.dmaj));
        w.rem = (int)(num - (unsigned int)w.n * 2u * (unsigned int)w.dmaj);
    } else {
        const long long num = 2ll * k0 * w.dmin + w.dmaj;
        w.n = (int)(num / (2ll * w.dmaj));
        w.rem = (int)(num - (long long)w.n * 2ll * w.dmaj);
    }
    return w;
}
// yields the walker's cell and moves on to the next
BL_HD void bl_walk_step(bl_walk& w, int* x, int* y)
{
    *x = w.xmajor ? w.x0 + w.sx * w.k : w.x0 + w.sx * w.n;
    *y = w.xmajor ? w.y0 + w.sy * w.n : w.y0 + w.sy * w.k;
    w.k += 1;
    w.rem += 2 * w.dmin;
    if (w.rem >= 2 * w.dmaj) { w.rem -= 2 * w.dmaj; w.n += 1; }
}
// cell k alone: one division per cell, for a kernel whose lanes each take a cell of one ray
BL_HD void bl_walk_cell(const int4 ray, int k, int* x, int* y)
{
    bl_walk w = bl_walk_begin(ray, k);
    bl_walk_step(w, x, y);
}
// f(x, y) for the cells k0 .. min(k1, K) - 1 of the walk
template <class F>
BL_HD void bl_walk_range(const int4 ray, int k0, int k1, F f)
{
    const int K = bl_ray_steps(ray);
    if (k1 > K) k1 = K;
    if (k0 >= k1) return;
    bl_walk w = bl_walk_begin(ray, k0);
    while (w.k < k1) {
        int x, y;
        bl_walk_step(w, &x, &y);
        f(x, y);
    }
}
// segments of `seg` cells that the walk of a ray is cut into
BL_HD int bl_ray_segs(const int4 ray, int seg) { return ray.x == BL_NO_RAY ? 0 : (bl_ray_steps(ray) + seg - 1) / seg; }

#if defined(__HIPCC__)
// ---------------------------------------------------------------------------------------------------------------- workgroup pieces
// The bounding box of all start and end cells of a workgroup's traced rays: every thread gathers its rays' cells, then a wave's
// min / max by shuffle and one lane's four LDS atomics (a lane per ray hammering four words serialises the phase).
// s_box = {xmin, ymin, xmax, ymax} starts at {BL_NO_RAY, BL_NO_RAY, -BL_NO_RAY, -BL_NO_RAY}: xmin == BL_NO_RAY means no ray.
struct bl_box { int x_lo, y_lo, x_hi, y_hi; };
__device__ __forceinline__ bl_box bl_box_none() { bl_box b = {BL_NO_RAY, BL_NO_RAY, -BL_NO_RAY, -BL_NO_RAY}; return b; }
__device__ __forceinline__ void bl_box_add(bl_box& b, const int4 ray)
{
    if (ray.x != BL_NO_RAY) {
        b.x_lo = min(b.x_lo, min(ray.x, ray.z)); b.y_lo = min(b.y_lo, min(ray.y, ray.w));
        b.x_hi = max(b.x_hi, max(ray.x, ray.z)); b.y_hi = max(b.y_hi, max(ray.y, ray.w));
    }
}
__device__ __forceinline__ void bl_box_to_lds(bl_box b, int* s_box)
{
    for (int off = 32; off > 0; off >>= 1) {
        b.x_lo = min(b.x_lo, __shfl_xor(b.x_lo, off, 64)); b.y_lo = min(b.y_lo, __shfl_xor(b.y_lo, off, 64));
        b.x_hi = max(b.x_hi, __shfl_xor(b.x_hi, off, 64)); b.y_hi = max(b.y_hi, __shfl_xor(b.y_hi, off, 64));
    }
    if ((threadIdx.x & 63) == 0 && b.x_lo != BL_NO_RAY) {
        atomicMin(&s_box[0], b.x_lo); atomicMin(&s_box[1], b.y_lo);
        atomicMax(&s_box[2], b.x_hi); atomicMax(&s_box[3], b.y_hi);
    }
}

// Two uint16 counters per LDS dword: cell c counts in the low half of dword c >> 1 when c is even, in the high half when odd.
__device__ __forceinline__ unsigned int bl_cnt_add(unsigned int* s_cnt, int c) { return atomicAdd(&s_cnt[c >> 1], (c & 1) ? 0x10000u : 1u); }   // the pair as it was
__device__ __forceinline__ unsigned int bl_cnt_half(unsigned int pair, int c) { return (c & 1) ? (pair >> 16) : (pair & 0xffffu); }
__device__ __forceinline__ int bl_cnt_of(const unsigned int* s_cnt, int c) { return (int)bl_cnt_half(s_cnt[c >> 1], c); }
__device__ __forceinline__ void bl_cnt_clear(unsigned int* s_cnt, int c) { atomicAnd(&s_cnt[c >> 1], (c & 1) ? 0x0000ffffu : 0xffff0000u); }

// The segment table segp[0 .. R] is the exclusive prefix of the rays' bl_ray_segs: segment sg belongs to the last ray r with
// segp[r] <= sg and starts at step (sg - segp[r]) * seg of its walk.
__device__ __forceinline__ int bl_seg_ray(const int* segp, int R, int sg)
{
    int lo = 0, hi = R - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (segp[mid] <= sg) lo = mid; else hi = mid - 1; }
    return lo;
}

// Four counters (16 bits each, cell 0 lowest) onto the four cells of a grid dword: HIT ? min(127, v + k c) : max(-128, v - k c).
template <bool HIT>
__device__ __forceinline__ unsigned int bl_apply4(unsigned long long c, int v, int k)
{
    unsigned int nv = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int cnt = (int)((c >> (16 * b)) & 0xffffull);
        const int val = (int)(int8_t)(v >> (8 * b));
        const int r = HIT ? min(127, val + k * cnt) : max(-128, val - k * cnt);
        nv |= ((unsigned int)r & 0xffu) << (8 * b);
    }
    return nv;
}
#endif  // __HIPCC__

#endif  // BL_MAPRAY_DEV_H
