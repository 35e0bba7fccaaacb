// bl_scanlog_dev.h -- what the map rebuild (bl_scanlog.hip) and the batched submap rebuild of the loop-closure front
// end (bl_loopclose.hip) share: the log's layout, and every rule by which a window of logged scans becomes cells.
//   host and device  the log handle and a slot's three arrays
//   device           a scan's ray cells and their clipped box (a workgroup); the clamped add (a, lo, hi) packed in 32 bits, its
//                    composition with one scan, its value; the part of a ray's walk inside a tile; one scan folded into a tile's
//                    functions in LDS (a workgroup)
// What differs stays where it was: which scans a workgroup folds and where the functions go (chunks, pairs and a scratch of
// functions there; a whole window and the cells themselves here).
#ifndef BL_SCANLOG_DEV_H
#define BL_SCANLOG_DEV_H

#include "bl_internal.h"
#include "bl_mapray_dev.h"

#define RL_TILE 64
#define RL_TILE_CELLS (RL_TILE * RL_TILE)
#define RL_THREADS 256
#define RL_MAX_RAYS 8192                     // the mapper's own limit (MAP_MAX_RAYS)
#define RL_RAY_BYTES 16                      // int64 time + float range + float theta

struct bl_scanlog {
    bl_ctx* ctx;
    int capacity, max_rays;
    int head, size;                          // slot of entry 0; entries held
    int* h_kept;                             // kept rays per slot (host copy of d_kept)
    char* d_scans;                           // per slot: times[max_rays] | ranges[max_rays] | thetas[max_rays]
    int* d_kept;
    bl_pose_xyt_t* d_poses;
    // scratch of bl_scanlog_rebuild
    void* d_P; size_t cap_P;                 // pose table: prev, then the poses of the scans
    void* d_rays; size_t cap_rays;
    void* d_boxes; size_t cap_boxes;         // scan boxes, then chunk boxes
    void* d_tiles; size_t cap_tiles;         // per tile: pair count, then (ntiles + 1) starts
    void* d_pairs; size_t cap_pairs;
    void* d_fn; size_t cap_fn;
    hipEvent_t ev[4];
    bool have_stats;
    bl_scanlog_stats_t stats;
};

struct rl_slot { int64_t* times; float* ranges; float* thetas; };
__host__ __device__ __forceinline__ rl_slot rl_slot_of(char* scans, int max_rays, int slot)
{
    char* p = scans + (size_t)slot * max_rays * RL_RAY_BYTES;
    rl_slot s;
    s.times = (int64_t*)p; s.ranges = (float*)(p + (size_t)max_rays * 8); s.thetas = (float*)(p + (size_t)max_rays * 12);
    return s;
}

// ---------------------------------------------------------------- a scan's ray cells and box
__device__ __forceinline__ bool rl_box_empty(const int4 b) { return b.z < b.x || b.w < b.y; }

__device__ __forceinline__ bool rl_meets(const int4 b, int tx0, int ty0, int tx1, int ty1)
{
    return !rl_box_empty(b) && b.x <= tx1 && b.z >= tx0 && b.y <= ty1 && b.w >= ty0;
}

// By a whole workgroup of RL_THREADS: the cells of the first R rays of slot `s`, traced from pose p0 to pose p1 in frame f (the
// arithmetic of k_map_update: bl_mapray_dev.h), into rays[0 .. R), and the box of all of them clipped to the grid (empty: z < x)
// into *scan_box.  s_box: four ints of LDS.
__device__ __forceinline__ void rl_scan_rays(const bl_frame& f, float max_laser, const rl_slot& s, int R, const bl_pose_xyt_t p0,
                                             const bl_pose_xyt_t p1, int4* rays, int4* scan_box, int* s_box)
{
    const int tid = threadIdx.x;
    const bl_pose3 pb = {p0.x, p0.y, p0.theta}, pe = {p1.x, p1.y, p1.theta};
    const bool interp = p0.utime != p1.utime;                   // equal utimes: the pose itself (interpolation.hpp:27)
    const double t_den = interp ? (double)(p1.utime - p0.utime) : 1.0;
    if (tid < 4) s_box[tid] = tid < 2 ? BL_NO_RAY : -BL_NO_RAY;
    __syncthreads();
    bl_box box = bl_box_none();
    for (int r = tid; r < R; r += RL_THREADS) {
        const int4 ray = bl_ray_cells(f, max_laser, interp, p0.utime, t_den, pb, pe, s.ranges[r], s.thetas[r], interp ? s.times[r] : 0);
        bl_box_add(box, ray);
        rays[r] = ray;
    }
    bl_box_to_lds(box, s_box);
    __syncthreads();
    if (tid == 0) {
        int4 b = make_int4(1, 1, 0, 0);
        if (s_box[0] != BL_NO_RAY) {
            b = make_int4(max(s_box[0], 0), max(s_box[1], 0), min(s_box[2], f.width - 1), min(s_box[3], f.height - 1));
            if (rl_box_empty(b)) b = make_int4(1, 1, 0, 0);
        }
        *scan_box = b;
    }
}

// ---------------------------------------------------------------- the clamped add and one scan folded into a tile
// f = (a, lo, hi) packed: a in the low 16 bits (int16), lo in bits 16-23, hi in bits 24-31 (int8 each)
#define RL_IDENTITY 0x7f800000u
__device__ __forceinline__ unsigned int rl_pack(int a, int lo, int hi) { return ((unsigned int)a & 0xffffu) | (((unsigned int)lo & 0xffu) << 16) | (((unsigned int)hi & 0xffu) << 24); }
__device__ __forceinline__ int rl_a(unsigned int f) { return (int)(short)(f & 0xffffu); }
__device__ __forceinline__ int rl_lo(unsigned int f) { return (int)(int8_t)((f >> 16) & 0xffu); }
__device__ __forceinline__ int rl_hi(unsigned int f) { return (int)(int8_t)(f >> 24); }
__device__ __forceinline__ int rl_eval(unsigned int f, int v) { return max(rl_lo(f), min(rl_hi(f), v + rl_a(f))); }

// one scan on top of f: H hits (v -> min(127, v + hit H)), then M misses (v -> max(-128, v - miss M)); each add saturated to 255
__device__ __forceinline__ unsigned int rl_compose_scan(unsigned int f, int H, int M, int hit, int miss)
{
    int a = rl_a(f), lo = rl_lo(f), hi = rl_hi(f);
    const int up = min(255, hit * H), down = min(255, miss * M);
    a = min(255, a + up); lo = min(127, lo + up); hi = min(127, hi + up);
    a = max(-255, a - down); lo = max(-128, lo - down); hi = max(-128, hi - down);
    return rl_pack(a, lo, hi);
}

// The cells of the reference's Bresenham walk of `ray` that fall into the tile, counted in the high halves of s_cnt (start cell
// included, end cell excluded; the walk from any step: bl_mapray_dev.h).  Only the steps k whose major coordinate m0 + sm k lies in
// the tile are visited.
__device__ __forceinline__ void rl_walk(unsigned int* s_cnt, const int4 ray, int tx0, int ty0, int tx1, int ty1)
{
    const int K = bl_ray_steps(ray);
    if (K == 0) return;                                         // ahead of the clip: behind it k_rl_fold took 197 us for 182 (profiles/mapray_headline.json)
    const bool xmajor = abs(ray.z - ray.x) >= abs(ray.w - ray.y);
    const int m0 = xmajor ? ray.x : ray.y, m1 = xmajor ? ray.z : ray.w;
    const int ta = xmajor ? tx0 : ty0, tb = xmajor ? tx1 : ty1;
    long long k_lo = m0 < m1 ? (long long)ta - m0 : (long long)m0 - tb;
    long long k_hi = m0 < m1 ? (long long)tb - m0 : (long long)m0 - ta;
    if (k_lo < 0) k_lo = 0;
    if (k_hi > K - 1) k_hi = K - 1;
    if (k_lo > k_hi) return;
    bl_walk_range(ray, (int)k_lo, (int)k_hi + 1, [&](int x, int y) {
        if (x >= tx0 && x <= tx1 && y >= ty0 && y <= ty1) atomicAdd(&s_cnt[(y - ty0) * RL_TILE + (x - tx0)], 0x10000u);
    });
}

// By a whole workgroup of RL_THREADS: one scan's R ray cells folded into the tile (tx0, ty0) .. (tx1, ty1).  s_fn: the composed
// function of every cell; s_cnt: hits (low half) and misses (high half) of the scan in hand, all zero before and after.  Two
// barriers.
__device__ __forceinline__ void rl_fold_scan(unsigned int* s_fn, unsigned int* s_cnt, const int4* rays, int R, int tx0, int ty0, int tx1,
                                             int ty1, int hit, int miss)
{
    const int tid = threadIdx.x;
    for (int r = tid; r < R; r += RL_THREADS) {
        const int4 ray = rays[r];
        if (ray.x == BL_NO_RAY) continue;
        if (min(ray.x, ray.z) > tx1 || max(ray.x, ray.z) < tx0 || min(ray.y, ray.w) > ty1 || max(ray.y, ray.w) < ty0) continue;
        if (ray.z >= tx0 && ray.z <= tx1 && ray.w >= ty0 && ray.w <= ty1) atomicAdd(&s_cnt[(ray.w - ty0) * RL_TILE + (ray.z - tx0)], 1u);
        rl_walk(s_cnt, ray, tx0, ty0, tx1, ty1);
    }
    __syncthreads();
    for (int j = tid; j < RL_TILE_CELLS; j += RL_THREADS) {
        const unsigned int n = s_cnt[j];
        if (n) { s_fn[j] = rl_compose_scan(s_fn[j], (int)(n & 0xffffu), (int)(n >> 16), hit, miss); s_cnt[j] = 0u; }
    }
    __syncthreads();
}

#endif  // BL_SCANLOG_DEV_H
