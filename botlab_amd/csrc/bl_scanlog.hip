// bl_scanlog.hip -- scan history and map rebuild (include/botlab_hip.h, "scan history").
//
// The log is a device-resident ring of the last `capacity` scans: per slot the kept rays as bl_scan_upload packs them (times |
// ranges | thetas), the kept count and the pose.  bl_scanlog_rebuild makes the map that count sequential Mapping::updateMap calls
// would leave, the scans folded in parallel:
//
//   One scan's effect on a cell that is the end of H rays and is crossed by M rays is v -> max(-128, min(127, v + hit H) - miss M)
//   (bl_mapping.hip): two clamped adds.  A clamped add is f = (a, lo, hi): v -> max(lo, min(hi, v + a)), and f2 o f1 =
//   (a1 + a2, f2(lo1), f2(hi1)) is one again; `a` may be kept saturated to +-255 because |v| <= 128.  So a chunk of consecutive scans
//   folds into ONE function per cell (32 bits: int16, int8, int8), chunks fold independently of each other, and applying the chunks'
//   functions to the base cell in chunk order gives the sequential result byte for byte.
//
//   phase 0  k_rl_poses, k_rl_rays: the pose table; one workgroup per scan writes the rays' start and end cells (the arithmetic of
//            k_map_update: bl_mapray_dev.h) and the scan's bounding box clipped to the grid.  k_rl_chunk_boxes, k_rl_count_fill
//            (twice), k_rl_scan: the chunks' boxes and the list of (tile, chunk) pairs whose boxes meet, tile-major, chunks ascending.
//   phase 1  k_rl_fold: one workgroup per pair; the tile's functions and two uint16 counters per cell in LDS (8 B per cell).
//   phase 2  k_rl_apply: a thread per cell applies its tile's pairs' functions in order to the base cell.
// Tiles are RL_TILE x RL_TILE cells, chunks RL_CHUNK scans (more when there would be over RL_MAX_CHUNKS of them).
#include <string.h>

#include "bl_internal.h"
#include "bl_scanlog_dev.h"                  // the log's layout and the rules the loop-closure front end (bl_loopclose.hip) folds by as well

#define RL_CHUNK 16
#define RL_MAX_CHUNKS 4096
#define RL_MAX_BYTES (1ull << 30)

// ---------------------------------------------------------------- the log
__global__ void k_rl_append(const int64_t* times, const float* ranges, const float* thetas, int kept, rl_slot dst, int* d_kept,
                            bl_pose_xyt_t* d_pose, const bl_pose_xyt_t* pose_dev, bl_pose_xyt_t pose_host, int64_t utime)
{
    for (int i = threadIdx.x; i < kept; i += blockDim.x) { dst.times[i] = times[i]; dst.ranges[i] = ranges[i]; dst.thetas[i] = thetas[i]; }
    if (threadIdx.x == 0) {
        bl_pose_xyt_t p = pose_dev ? *pose_dev : pose_host;
        p.utime = utime;
        *d_pose = p;
        *d_kept = kept;
    }
}

extern "C" int bl_scanlog_create(bl_ctx* ctx, int capacity_scans, int max_rays_per_scan, bl_scanlog** out)
{
    BL_CHECK_ARG(out != nullptr);
    BL_CHECK_ARG(capacity_scans >= 1 && max_rays_per_scan >= 1 && max_rays_per_scan <= RL_MAX_RAYS);
    BL_CHECK_ARG((unsigned long long)capacity_scans * (unsigned long long)max_rays_per_scan * RL_RAY_BYTES <= RL_MAX_BYTES);
    BL_CHECK_ARG(ctx != nullptr);
    BL_HIP(hipSetDevice(ctx->device));
    bl_scanlog* l = new bl_scanlog();
    memset(l, 0, sizeof(*l));
    l->ctx = ctx; l->capacity = capacity_scans; l->max_rays = max_rays_per_scan;
    l->h_kept = new int[capacity_scans]();
    hipError_t e = hipMalloc((void**)&l->d_scans, (size_t)capacity_scans * max_rays_per_scan * RL_RAY_BYTES);
    if (e == hipSuccess) e = hipMalloc((void**)&l->d_kept, (size_t)capacity_scans * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void**)&l->d_poses, (size_t)capacity_scans * sizeof(bl_pose_xyt_t));
    if (e == hipSuccess) e = hipMemsetAsync(l->d_kept, 0, (size_t)capacity_scans * sizeof(int), ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(l->d_poses, 0, (size_t)capacity_scans * sizeof(bl_pose_xyt_t), ctx->stream);
    for (int i = 0; i < 4 && e == hipSuccess; ++i) e = hipEventCreate(&l->ev[i]);
    if (e != hipSuccess) { bl_set_error("bl_scanlog_create: %s", hipGetErrorString(e)); bl_scanlog_destroy(l); return BL_ERR_HIP; }
    *out = l;
    return BL_OK;
}

extern "C" void bl_scanlog_destroy(bl_scanlog* l)
{
    if (!l) return;
    (void)hipStreamSynchronize(l->ctx->stream);
    void* bufs[] = {l->d_scans, l->d_kept, l->d_poses, l->d_P, l->d_rays, l->d_boxes, l->d_tiles, l->d_pairs, l->d_fn};
    for (void* b : bufs) if (b) (void)hipFree(b);
    for (int i = 0; i < 4; ++i) if (l->ev[i]) (void)hipEventDestroy(l->ev[i]);
    delete[] l->h_kept;
    delete l;
}

static int scanlog_append(bl_scanlog* l, const bl_lidar_t* scan, const bl_pose_xyt_t* h_pose, const void* d_pose, int64_t utime)
{
    BL_CHECK_ARG(l != nullptr && scan != nullptr);
    BL_CHECK_ARG(scan->num_ranges >= 0 && scan->num_ranges <= RL_MAX_RAYS);
    bl_ctx* ctx = l->ctx;
    BL_HIP(hipSetDevice(ctx->device));
    int kept = 0;
    const int rc = bl_scan_upload(ctx, scan, &kept);           // the ctx's scan block: the very rays the mapper traces
    if (rc) return rc;
    BL_CHECK_ARG(kept <= l->max_rays);                          // refused: the log is as it was
    const bool full = l->size == l->capacity;
    const int slot = full ? l->head : (l->head + l->size) % l->capacity;
    bl_pose_xyt_t hp; hp.utime = 0; hp.x = hp.y = hp.theta = 0.0f;
    if (h_pose) hp = *h_pose;
    hipLaunchKernelGGL(k_rl_append, dim3(1), dim3(RL_THREADS), 0, ctx->stream, ctx->scan.times, ctx->scan.ranges, ctx->scan.thetas, kept,
                       rl_slot_of(l->d_scans, l->max_rays, slot), l->d_kept + slot, l->d_poses + slot, (const bl_pose_xyt_t*)d_pose, hp, utime);
    BL_HIP(hipGetLastError());
    l->h_kept[slot] = kept;
    if (full) l->head = (l->head + 1) % l->capacity; else l->size += 1;      // a full ring drops its oldest scan
    return BL_OK;
}

extern "C" int bl_scanlog_append(bl_scanlog* l, const bl_lidar_t* scan, const bl_pose_xyt_t* pose)
{
    BL_CHECK_ARG(pose != nullptr);
    return scanlog_append(l, scan, pose, nullptr, pose->utime);
}

extern "C" int bl_scanlog_append_dev_pose(bl_scanlog* l, const bl_lidar_t* scan, const void* d_pose, int64_t pose_utime)
{
    BL_CHECK_ARG(d_pose != nullptr);
    return scanlog_append(l, scan, nullptr, d_pose, pose_utime);
}

extern "C" int bl_scanlog_size(const bl_scanlog* l) { return l ? l->size : 0; }

void bl_scanlog_view_host(const bl_scanlog* l, bl_scanlog_view* out)
{
    out->ctx = l->ctx; out->capacity = l->capacity; out->head = l->head; out->size = l->size; out->d_poses = l->d_poses;
}

// entries first .. first + count - 1 lie in at most two runs of slots
template <class F>
static int scanlog_runs(const bl_scanlog* l, int first, int count, F f)
{
    const int s0 = (l->head + first) % l->capacity;
    const int n0 = count < l->capacity - s0 ? count : l->capacity - s0;
    int rc = f(s0, 0, n0);
    if (!rc && n0 < count) rc = f(0, n0, count - n0);
    return rc;
}

extern "C" int bl_scanlog_get_poses(bl_scanlog* l, int first, int count, bl_pose_xyt_t* out)
{
    BL_CHECK_ARG(l != nullptr && out != nullptr);
    BL_CHECK_ARG(first >= 0 && count >= 1 && first <= l->size && count <= l->size - first);
    BL_HIP(hipSetDevice(l->ctx->device));
    const int rc = scanlog_runs(l, first, count, [&](int slot, int at, int n) -> int {
        BL_HIP(hipMemcpyAsync(out + at, l->d_poses + slot, (size_t)n * sizeof(bl_pose_xyt_t), hipMemcpyDeviceToHost, l->ctx->stream));
        return BL_OK;
    });
    if (rc) return rc;
    BL_HIP(hipStreamSynchronize(l->ctx->stream));
    return BL_OK;
}

extern "C" int bl_scanlog_set_poses(bl_scanlog* l, int first, int count, const bl_pose_xyt_t* poses)
{
    BL_CHECK_ARG(l != nullptr && poses != nullptr);
    BL_CHECK_ARG(first >= 0 && count >= 1 && first <= l->size && count <= l->size - first);
    BL_HIP(hipSetDevice(l->ctx->device));
    const int rc = scanlog_runs(l, first, count, [&](int slot, int at, int n) -> int {
        BL_HIP(hipMemcpyAsync(l->d_poses + slot, poses + at, (size_t)n * sizeof(bl_pose_xyt_t), hipMemcpyHostToDevice, l->ctx->stream));
        return BL_OK;
    });
    if (rc) return rc;
    BL_HIP(hipStreamSynchronize(l->ctx->stream));             // the host array is the caller's and may be reused at once
    return BL_OK;
}

extern "C" int bl_scanlog_get_scan(bl_scanlog* l, int i, float* ranges, float* thetas, int64_t* times, int* kept)
{
    BL_CHECK_ARG(l != nullptr && i >= 0 && i < l->size);
    BL_HIP(hipSetDevice(l->ctx->device));
    const int slot = (l->head + i) % l->capacity;
    const int n = l->h_kept[slot];
    const rl_slot s = rl_slot_of(l->d_scans, l->max_rays, slot);
    if (kept) *kept = n;
    if (n > 0) {
        if (ranges) BL_HIP(hipMemcpyAsync(ranges, s.ranges, (size_t)n * 4, hipMemcpyDeviceToHost, l->ctx->stream));
        if (thetas) BL_HIP(hipMemcpyAsync(thetas, s.thetas, (size_t)n * 4, hipMemcpyDeviceToHost, l->ctx->stream));
        if (times) BL_HIP(hipMemcpyAsync(times, s.times, (size_t)n * 8, hipMemcpyDeviceToHost, l->ctx->stream));
    }
    BL_HIP(hipStreamSynchronize(l->ctx->stream));
    return BL_OK;
}

// ---------------------------------------------------------------- rebuild, phase 0: poses, ray cells, boxes, pairs
struct rl_args {
    int n;                      // active scans: scan i of them is entry e0 + i of the log, traced from P[p0 + i] to P[p0 + i + 1]
    int e0, p0;
    int head, capacity, max_rays, stride;
    int chunk, nchunks, ntx, nty;
    bl_frame frame;
    float max_laser; int hit, miss;
    char* scans; const int* kept; const bl_pose_xyt_t* P;
    int4* rays; int4* scan_box; int4* chunk_box;
    int* tile_cnt; int* tile_start; int2* pairs;
    unsigned int* fn;
    const int8_t* base; int8_t* out;
};

// P[0] = prev, P[1 + i] = the recorded pose of entry first + i (skipped when the caller's poses were copied there already)
__global__ void k_rl_poses(bl_pose_xyt_t* P, bl_pose_xyt_t prev, const bl_pose_xyt_t* ring, int head, int capacity, int first, int count, int recorded)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) P[0] = prev;
    if (recorded && i < count) P[1 + i] = ring[(head + first + i) % capacity];
}

// one workgroup per active scan: its rays' cells and the box of all of them, clipped to the grid (empty: z < x)
__global__ __launch_bounds__(RL_THREADS) void k_rl_rays(rl_args a)
{
    __shared__ int s_box[4];
    const int i = blockIdx.x;
    const int slot = (a.head + a.e0 + i) % a.capacity;
    rl_scan_rays(a.frame, a.max_laser, rl_slot_of(a.scans, a.max_rays, slot), min(a.kept[slot], a.stride), a.P[a.p0 + i], a.P[a.p0 + i + 1],
                 a.rays + (size_t)i * a.stride, &a.scan_box[i], s_box);
}

// a chunk's box: the union over its scans
__global__ void k_rl_chunk_boxes(rl_args a)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.nchunks) return;
    int4 u = make_int4(1, 1, 0, 0);
    for (int i = c * a.chunk; i < min(a.n, (c + 1) * a.chunk); ++i) {
        const int4 b = a.scan_box[i];
        if (rl_box_empty(b)) continue;
        u = rl_box_empty(u) ? b : make_int4(min(u.x, b.x), min(u.y, b.y), max(u.z, b.z), max(u.w, b.w));
    }
    a.chunk_box[c] = u;
}

// a thread per tile: how many chunks' boxes meet it (fill == 0), or the list of them at the tile's start (fill != 0)
__global__ void k_rl_count_fill(rl_args a, int fill)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.ntx * a.nty) return;
    const int ty = t / a.ntx, tx = t - ty * a.ntx;
    const int tx0 = tx * RL_TILE, ty0 = ty * RL_TILE;
    const int tx1 = min(tx0 + RL_TILE, a.frame.width) - 1, ty1 = min(ty0 + RL_TILE, a.frame.height) - 1;
    int n = 0;
    const int at = fill ? a.tile_start[t] : 0;
    for (int c = 0; c < a.nchunks; ++c)
        if (rl_meets(a.chunk_box[c], tx0, ty0, tx1, ty1)) {
            if (fill) a.pairs[at + n] = make_int2(t, c);
            ++n;
        }
    if (!fill) a.tile_cnt[t] = n;
}

// one workgroup: tile_start = the exclusive prefix of tile_cnt, tile_start[ntiles] = the number of pairs
__global__ __launch_bounds__(1024) void k_rl_scan(const int* cnt, int* start, int ntiles)
{
    __shared__ int s_w[16];
    __shared__ int s_base;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid == 0) s_base = 0;
    __syncthreads();
    for (int t0 = 0; t0 < ntiles; t0 += 1024) {
        const int t = t0 + tid;
        const int v = t < ntiles ? cnt[t] : 0;
        int incl = v;
        for (int off = 1; off < 64; off <<= 1) { const int o = __shfl_up(incl, off, 64); if (lane >= off) incl += o; }
        if (lane == 63) s_w[w] = incl;
        __syncthreads();
        int base = s_base;
        for (int k = 0; k < w; ++k) base += s_w[k];
        if (t < ntiles) start[t] = base + incl - v;
        __syncthreads();
        if (tid == 1023) s_base = base + incl;
        __syncthreads();
    }
    if (tid == 0) start[ntiles] = s_base;
}

// ---------------------------------------------------------------- phase 1: fold a chunk's scans into one function per cell of a tile
// The packed function (a, lo, hi), its composition with one scan, the walk inside a tile and one scan's fold: bl_scanlog_dev.h.
__global__ __launch_bounds__(RL_THREADS) void k_rl_fold(rl_args a)
{
    __shared__ unsigned int s_fn[RL_TILE_CELLS];                // the composed function of every cell
    __shared__ unsigned int s_cnt[RL_TILE_CELLS];               // hits (low half) and misses (high half) of the scan in hand
    const int tid = threadIdx.x;
    const int2 pr = a.pairs[blockIdx.x];
    const int t = pr.x, c = pr.y;
    const int ty = t / a.ntx, tx = t - ty * a.ntx;
    const int tx0 = tx * RL_TILE, ty0 = ty * RL_TILE;
    const int tx1 = min(tx0 + RL_TILE, a.frame.width) - 1, ty1 = min(ty0 + RL_TILE, a.frame.height) - 1;
    for (int i = tid; i < RL_TILE_CELLS; i += RL_THREADS) { s_fn[i] = RL_IDENTITY; s_cnt[i] = 0u; }
    __syncthreads();
    for (int i = c * a.chunk; i < min(a.n, (c + 1) * a.chunk); ++i) {
        if (!rl_meets(a.scan_box[i], tx0, ty0, tx1, ty1)) continue;            // uniform over the workgroup
        const int slot = (a.head + a.e0 + i) % a.capacity;
        rl_fold_scan(s_fn, s_cnt, a.rays + (size_t)i * a.stride, min(a.kept[slot], a.stride), tx0, ty0, tx1, ty1, a.hit, a.miss);
    }
    unsigned int* dst = a.fn + (size_t)blockIdx.x * RL_TILE_CELLS;
    for (int i = tid; i < RL_TILE_CELLS; i += RL_THREADS) dst[i] = s_fn[i];
}

// ---------------------------------------------------------------- phase 2: a tile's pairs, in chunk order, onto the base cell
// RL_APPLY_PARTS workgroups per tile, a thread per cell: with a long history a tile has hundreds of pairs, and the walk over them is
// the serial part of the rebuild
#define RL_APPLY_PARTS (RL_TILE_CELLS / RL_THREADS)
__global__ __launch_bounds__(RL_THREADS) void k_rl_apply(rl_args a)
{
    const int t = blockIdx.x / RL_APPLY_PARTS, j = (blockIdx.x % RL_APPLY_PARTS) * RL_THREADS + threadIdx.x;
    const int ty = t / a.ntx, tx = t - ty * a.ntx;
    const int p0 = a.tile_start[t], p1 = a.tile_start[t + 1];
    if (p0 == p1 && a.base == a.out) return;                    // nothing folds into this tile and the cells are in place
    const int x = tx * RL_TILE + (j & (RL_TILE - 1)), y = ty * RL_TILE + j / RL_TILE;
    if (x >= a.frame.width || y >= a.frame.height) return;
    const size_t at = (size_t)y * a.frame.width + x;
    int v = a.base ? (int)a.base[at] : 0;
    const unsigned int* fn = a.fn + j;
#pragma unroll 4
    for (int p = p0; p < p1; ++p) v = rl_eval(fn[(size_t)p * RL_TILE_CELLS], v);
    a.out[at] = (int8_t)v;
}

// ---------------------------------------------------------------- host side of the rebuild
static bool same_frame(const bl_frame& p, const bl_frame& q)
{
    return p.width == q.width && p.height == q.height && p.mpc == q.mpc && p.cpm == q.cpm && p.ox == q.ox && p.oy == q.oy;
}

extern "C" int bl_scanlog_rebuild(bl_scanlog* l, int first, int count, const bl_pose_xyt_t* poses, const bl_pose_xyt_t* prev_pose,
                                  float max_laser, int8_t hit, int8_t miss, const bl_grid* base, bl_grid* out)
{
    BL_CHECK_ARG(l != nullptr && out != nullptr);
    BL_CHECK_ARG(first >= 0 && count >= 1 && first <= l->size && count <= l->size - first);
    BL_CHECK_ARG(hit >= 0 && miss >= 0);
    BL_CHECK_ARG(out->ctx == l->ctx);
    BL_CHECK_ARG(base == nullptr || (base->ctx == l->ctx && same_frame(base->frame, out->frame)));
    bl_ctx* ctx = l->ctx;
    BL_HIP(hipSetDevice(ctx->device));
    const int W = out->frame.width, H = out->frame.height;
    rl_args a;
    memset(&a, 0, sizeof(a));
    a.p0 = prev_pose ? 0 : 1;                                   // without a previous pose the first scan only latches its pose
    a.e0 = first + a.p0;
    a.n = count - a.p0;
    a.head = l->head; a.capacity = l->capacity; a.max_rays = l->max_rays;
    int stride = 1;
    for (int i = 0; i < a.n; ++i) { const int k = l->h_kept[(l->head + a.e0 + i) % l->capacity]; if (k > stride) stride = k; }
    a.stride = stride;
    a.chunk = RL_CHUNK;
    if ((a.n + a.chunk - 1) / a.chunk > RL_MAX_CHUNKS) a.chunk = (a.n + RL_MAX_CHUNKS - 1) / RL_MAX_CHUNKS;
    a.nchunks = (a.n + a.chunk - 1) / a.chunk;
    a.ntx = (W + RL_TILE - 1) / RL_TILE; a.nty = (H + RL_TILE - 1) / RL_TILE;
    const int ntiles = a.ntx * a.nty;
    a.frame = out->frame;
    a.max_laser = max_laser; a.hit = hit; a.miss = miss;
    a.scans = l->d_scans; a.kept = l->d_kept;
    int rc = bl_grow(&l->d_P, &l->cap_P, (size_t)(count + 1) * sizeof(bl_pose_xyt_t), false, ctx);
    if (!rc) rc = bl_grow(&l->d_rays, &l->cap_rays, (size_t)(a.n > 0 ? a.n : 1) * stride * sizeof(int4), false, ctx);
    if (!rc) rc = bl_grow(&l->d_boxes, &l->cap_boxes, (size_t)(a.n + a.nchunks + 1) * sizeof(int4), false, ctx);
    if (!rc) rc = bl_grow(&l->d_tiles, &l->cap_tiles, (size_t)(2 * ntiles + 1) * sizeof(int), false, ctx);
    if (rc) return rc;
    a.P = (const bl_pose_xyt_t*)l->d_P;
    a.rays = (int4*)l->d_rays;
    a.scan_box = (int4*)l->d_boxes; a.chunk_box = a.scan_box + a.n;
    a.tile_cnt = (int*)l->d_tiles; a.tile_start = a.tile_cnt + ntiles;
    a.base = base ? base->cells : nullptr; a.out = out->cells;
    // `out` is rewritten wholesale: as after an upload, its mirror is stale and its cells start a new lineage
    out->mirror_valid = false;
    (void)bl_grid_new_lineage(out);

    BL_HIP(hipEventRecord(l->ev[0], ctx->stream));
    int npairs = 0;
    if (a.n > 0) {
        bl_pose_xyt_t prev; prev.utime = 0; prev.x = prev.y = prev.theta = 0.0f;
        if (prev_pose) prev = *prev_pose;
        if (poses) BL_HIP(hipMemcpyAsync((bl_pose_xyt_t*)l->d_P + 1, poses, (size_t)count * sizeof(bl_pose_xyt_t), hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(k_rl_poses, dim3((count + 255) / 256), dim3(256), 0, ctx->stream, (bl_pose_xyt_t*)l->d_P, prev, l->d_poses, l->head,
                           l->capacity, first, count, poses ? 0 : 1);
        hipLaunchKernelGGL(k_rl_rays, dim3(a.n), dim3(RL_THREADS), 0, ctx->stream, a);
        hipLaunchKernelGGL(k_rl_chunk_boxes, dim3((a.nchunks + 255) / 256), dim3(256), 0, ctx->stream, a);
        hipLaunchKernelGGL(k_rl_count_fill, dim3((ntiles + 255) / 256), dim3(256), 0, ctx->stream, a, 0);
        hipLaunchKernelGGL(k_rl_scan, dim3(1), dim3(1024), 0, ctx->stream, (const int*)a.tile_cnt, a.tile_start, ntiles);
        BL_HIP(hipGetLastError());
        // the one read-back: the number of pairs sizes the scratch (and the caller's pose array is free again)
        BL_HIP(hipMemcpyAsync(&npairs, a.tile_start + ntiles, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        BL_HIP(hipStreamSynchronize(ctx->stream));
    } else {
        BL_HIP(hipMemsetAsync(a.tile_start, 0, (size_t)(ntiles + 1) * sizeof(int), ctx->stream));
    }
    BL_HIP(hipEventRecord(l->ev[1], ctx->stream));
    if (npairs > 0) {
        rc = bl_grow(&l->d_pairs, &l->cap_pairs, (size_t)npairs * sizeof(int2), false, ctx);
        if (!rc) rc = bl_grow(&l->d_fn, &l->cap_fn, (size_t)npairs * RL_TILE_CELLS * sizeof(unsigned int), false, ctx);
        if (rc) return rc;
        a.pairs = (int2*)l->d_pairs; a.fn = (unsigned int*)l->d_fn;
        hipLaunchKernelGGL(k_rl_count_fill, dim3((ntiles + 255) / 256), dim3(256), 0, ctx->stream, a, 1);
        hipLaunchKernelGGL(k_rl_fold, dim3(npairs), dim3(RL_THREADS), 0, ctx->stream, a);
        BL_HIP(hipGetLastError());
    }
    BL_HIP(hipEventRecord(l->ev[2], ctx->stream));
    hipLaunchKernelGGL(k_rl_apply, dim3(ntiles * RL_APPLY_PARTS), dim3(RL_THREADS), 0, ctx->stream, a);
    BL_HIP(hipGetLastError());
    BL_HIP(hipEventRecord(l->ev[3], ctx->stream));
    memset(&l->stats, 0, sizeof(l->stats));
    l->stats.tiles = ntiles; l->stats.chunks = a.nchunks; l->stats.pairs = npairs;
    l->stats.scratch_bytes = (int64_t)npairs * RL_TILE_CELLS * (int64_t)sizeof(unsigned int);
    l->stats.chunk_scans = a.chunk; l->stats.tile_cells = RL_TILE; l->stats.scans = a.n;
    l->have_stats = true;
    return BL_OK;
}

extern "C" int bl_scanlog_last_stats(bl_scanlog* l, bl_scanlog_stats_t* stats)
{
    BL_CHECK_ARG(l != nullptr && stats != nullptr);
    if (!l->have_stats) { bl_set_error("bl_scanlog_last_stats: no rebuild yet"); return BL_ERR_STATE; }
    BL_HIP(hipSetDevice(l->ctx->device));
    BL_HIP(hipEventSynchronize(l->ev[3]));
    BL_HIP(hipEventElapsedTime(&l->stats.ms_total, l->ev[0], l->ev[3]));
    BL_HIP(hipEventElapsedTime(&l->stats.ms_geometry, l->ev[0], l->ev[1]));
    BL_HIP(hipEventElapsedTime(&l->stats.ms_fold, l->ev[1], l->ev[2]));
    BL_HIP(hipEventElapsedTime(&l->stats.ms_apply, l->ev[2], l->ev[3]));
    *stats = l->stats;
    return BL_OK;
}
