// bl_rangetable.hip -- the range table (include/botlab_hip.h, "range table"): for every cell of a map and Hn headings the beam model's
// expected range, computed once, so that the beam model can look it up (k_beam_lookup, bl_beam.hip) instead of walking the map for
// every particle and ray.  No reference counterpart; the definition in the header is the contract and tests/range_table_model.py
// restates it.
//
//   k_rt_build    over a box of cells (the whole grid for a build, the changed box widened by reach for an update): a workgroup per
//                 RT_WG_CELLS cells of the box in row order, a wave per RT_WAVE_CELLS of them one after the other, a LANE PER HEADING
//                 in rounds of 64.  The lane's walk from the cell towards cell + D[h] is the cast's own (beam_first_hit, bl_beam_dev.h),
//                 ended where it leaves the grid, and the entry the cast's length of the hit cell (beam_quarter).  An occupied start cell
//                 is settled without a walk.  D[] lives in LDS.  A round stores 64 consecutive uint16 of the cell's row: 128 bytes.
//                 The map bytes come from the grid through L2; the other form -- the workgroup's tile of cells widened by reach staged
//                 in LDS -- was not built and is not measured.
//
// Integers only behind the host-made directions; no atomics; no workgroup waits for another; no result depends on the launch shape.
#include <math.h>
#include <string.h>

#include "bl_beam_dev.h"

#define RT_THREADS 256
#define RT_WAVE_CELLS 16
#define RT_WG_CELLS ((RT_THREADS / 64) * RT_WAVE_CELLS)
#define RT_MIN_HEADINGS 64
#define RT_MAX_HEADINGS 1024
#define RT_MAX_ENTRIES (1ll << 31)

struct rt_args {
    const int8_t* cells; int W, H, Hn, occ_min;
    int bx0, by0, bw; long long ncells;                   // the box: its corner, its width and its cells
    const int2* dirs;
    uint16_t* table;
};

__global__ __launch_bounds__(RT_THREADS) void k_rt_build(rt_args a)
{
    __shared__ int2 s_dir[RT_MAX_HEADINGS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int W = a.W, H = a.H;
    for (int i = tid; i < a.Hn; i += RT_THREADS) s_dir[i] = a.dirs[i];
    __syncthreads();
    const long long c0 = (long long)blockIdx.x * RT_WG_CELLS + wave * RT_WAVE_CELLS;
    for (int q = 0; q < RT_WAVE_CELLS; ++q) {
        const long long c = c0 + q;
        if (c >= a.ncells) break;                                       // (uniform over the wave)
        const int by = (int)(c / a.bw), bx = (int)(c - (long long)by * a.bw);
        const int sx = a.bx0 + bx, sy = a.by0 + by;
        uint16_t* row = a.table + ((size_t)sy * W + sx) * a.Hn;
        if (a.cells[(size_t)sy * W + sx] >= a.occ_min) {                // (uniform over the wave): first = 0 whatever the heading
            for (int h = lane; h < a.Hn; h += 64) row[h] = 0;
            continue;
        }
        for (int h = lane; h < a.Hn; h += 64) {
            const int2 d = s_dir[h];
            const beam_hit hit = beam_first_hit(sx, sy, sx + d.x, sy + d.y,
                [&](int x, int y) { return a.cells[(size_t)y * W + x] >= a.occ_min; },
                [&](int x, int y) { return !((unsigned int)x < (unsigned int)W && (unsigned int)y < (unsigned int)H); });
            row[h] = (uint16_t)(hit.first < hit.K ? (uint32_t)beam_quarter(hit.x, hit.y, sx, sy) : (uint32_t)BL_RANGETABLE_NONE);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- host
struct bl_rangetable {
    bl_ctx* ctx;
    int headings;
    bool built, timed;
    bl_frame frame; int reach, occ_min;                   // of the last build
    uint16_t* d_table; size_t table_cap;                  // entries allocated
    int2* h_dirs; int2* d_dirs;                           // headings each; h_dirs pinned
    hipEvent_t ev_a, ev_b;
};

void bl_rangetable_view_host(const bl_rangetable* rt, bl_rangetable_view* out)
{
    out->ctx = rt->ctx; out->built = rt->built; out->frame = rt->frame; out->headings = rt->headings; out->reach = rt->reach;
    out->occ_min = rt->occ_min; out->d_table = rt->d_table;
}

extern "C" int bl_rangetable_create(bl_ctx* ctx, int headings, bl_rangetable** out)
{
    BL_CHECK_ARG(ctx != nullptr && out != nullptr);
    BL_CHECK_ARG(headings >= RT_MIN_HEADINGS && headings <= RT_MAX_HEADINGS && (headings & (headings - 1)) == 0);
    BL_HIP(hipSetDevice(ctx->device));
    bl_rangetable* rt = new bl_rangetable();
    memset((void*)rt, 0, sizeof(*rt));
    rt->ctx = ctx; rt->headings = headings;
    hipError_t e = hipMalloc((void**)&rt->d_dirs, (size_t)headings * sizeof(int2));
    if (e == hipSuccess) e = hipHostMalloc((void**)&rt->h_dirs, (size_t)headings * sizeof(int2), hipHostMallocDefault);
    if (e == hipSuccess) e = hipEventCreate(&rt->ev_a);
    if (e == hipSuccess) e = hipEventCreate(&rt->ev_b);
    if (e != hipSuccess) {
        bl_set_error("bl_rangetable_create: %s", hipGetErrorString(e));
        bl_rangetable_destroy(rt);
        return BL_ERR_HIP;
    }
    *out = rt;
    return BL_OK;
}

extern "C" void bl_rangetable_destroy(bl_rangetable* rt)
{
    if (!rt) return;
    (void)hipSetDevice(rt->ctx->device);
    (void)hipStreamSynchronize(rt->ctx->stream);
    if (rt->d_table) (void)hipFree(rt->d_table);
    if (rt->d_dirs) (void)hipFree(rt->d_dirs);
    if (rt->h_dirs) (void)hipHostFree(rt->h_dirs);
    if (rt->ev_a) (void)hipEventDestroy(rt->ev_a);
    if (rt->ev_b) (void)hipEventDestroy(rt->ev_b);
    delete rt;
}

// k_rt_build over the cells x0 .. x1, y0 .. y1 (inside the grid, not empty) of the built frame
static int rt_launch(bl_rangetable* rt, const bl_grid* map, int x0, int y0, int x1, int y1)
{
    bl_ctx* ctx = rt->ctx;
    rt_args a;
    a.cells = map->cells; a.W = rt->frame.width; a.H = rt->frame.height; a.Hn = rt->headings; a.occ_min = rt->occ_min;
    a.bx0 = x0; a.by0 = y0; a.bw = x1 - x0 + 1; a.ncells = (long long)a.bw * (y1 - y0 + 1);
    a.dirs = rt->d_dirs; a.table = rt->d_table;
    const long long blocks = (a.ncells + RT_WG_CELLS - 1) / RT_WG_CELLS;      // <= 2^31 / 64 / 64
    BL_HIP(hipEventRecord(rt->ev_a, ctx->stream));
    hipLaunchKernelGGL(k_rt_build, dim3((unsigned int)blocks), dim3(RT_THREADS), 0, ctx->stream, a);
    BL_HIP(hipGetLastError());
    BL_HIP(hipEventRecord(rt->ev_b, ctx->stream));
    rt->timed = true;
    return BL_OK;
}

extern "C" int bl_rangetable_build(bl_rangetable* rt, const bl_beam* beam, const bl_grid* map)
{
    BL_CHECK_ARG(rt != nullptr && beam != nullptr && map != nullptr);
    bl_beam_view bv;
    bl_beam_view_host(beam, &bv);
    BL_CHECK_ARG(bv.ctx == rt->ctx && map->ctx == rt->ctx);
    if (!bv.have_params) { bl_set_error("beam model has no parameters (bl_beam_set_params first)"); return BL_ERR_STATE; }
    int reach = 0;
    const int rr = beam_reach(bv.max_range, map->frame.cpm, &reach);
    if (rr) return rr;
    const int W = map->frame.width, H = map->frame.height, Hn = rt->headings;
    BL_CHECK_ARG(W >= 1 && H >= 1);
    const long long entries = (long long)W * H * Hn;
    BL_CHECK_ARG(entries <= RT_MAX_ENTRIES);                            // before anything is allocated
    bl_ctx* ctx = rt->ctx;
    BL_HIP(hipSetDevice(ctx->device));
    BL_HIP(hipStreamSynchronize(ctx->stream));                          // h_dirs may be on its way; the old table may be read
    if ((size_t)entries > rt->table_cap) {
        if (rt->d_table) BL_HIP(hipFree(rt->d_table));
        rt->d_table = nullptr; rt->table_cap = 0; rt->built = false;
        BL_HIP(hipMalloc((void**)&rt->d_table, (size_t)entries * sizeof(uint16_t)));
        rt->table_cap = (size_t)entries;
    }
    rt->built = false;
    for (int h = 0; h < Hn; ++h) {
        const double t = 2.0 * BL_PI * (double)h / (double)Hn;
        rt->h_dirs[h] = make_int2((int)lround((double)reach * cos(t)), (int)lround((double)reach * sin(t)));
    }
    BL_HIP(hipMemcpyAsync(rt->d_dirs, rt->h_dirs, (size_t)Hn * sizeof(int2), hipMemcpyHostToDevice, ctx->stream));
    rt->frame = map->frame; rt->reach = reach; rt->occ_min = bv.occ_min;
    const int rc = rt_launch(rt, map, 0, 0, W - 1, H - 1);
    if (rc) return rc;
    rt->built = true;
    return BL_OK;
}

static int rt_need_built(const bl_rangetable* rt)
{
    if (!rt) { bl_set_error("bad argument: no range table handle"); return BL_ERR_ARG; }
    if (!rt->built) { bl_set_error("range table not built (bl_rangetable_build first)"); return BL_ERR_STATE; }
    return BL_OK;
}

extern "C" int bl_rangetable_update(bl_rangetable* rt, const bl_grid* map, int x0, int y0, int x1, int y1)
{
    int rc = rt_need_built(rt);
    if (rc) return rc;
    BL_CHECK_ARG(map != nullptr && map->ctx == rt->ctx);
    const int W = rt->frame.width, H = rt->frame.height;
    BL_CHECK_ARG(map->frame.width == W && map->frame.height == H);
    if (x1 < x0 || y1 < y0 || x1 < 0 || y1 < 0 || x0 >= W || y0 >= H) return BL_OK;
    const long long r = rt->reach;                                     // (the corners may lie anywhere in int)
    const int wx0 = (int)(x0 - r > 0 ? x0 - r : 0), wy0 = (int)(y0 - r > 0 ? y0 - r : 0);
    const int wx1 = (int)(x1 + r < W - 1 ? x1 + r : W - 1), wy1 = (int)(y1 + r < H - 1 ? y1 + r : H - 1);
    BL_HIP(hipSetDevice(rt->ctx->device));
    return rt_launch(rt, map, wx0, wy0, wx1, wy1);
}

extern "C" int bl_rangetable_read(bl_rangetable* rt, int x0, int y0, int w, int h, uint16_t* out)
{
    int rc = rt_need_built(rt);
    if (rc) return rc;
    const int W = rt->frame.width, H = rt->frame.height, Hn = rt->headings;
    BL_CHECK_ARG(out != nullptr && x0 >= 0 && y0 >= 0 && w >= 1 && h >= 1 && w <= W - x0 && h <= H - y0);
    bl_ctx* ctx = rt->ctx;
    BL_HIP(hipSetDevice(ctx->device));
    const size_t row = (size_t)w * Hn;                                  // entries of one row of the rectangle: contiguous in the table
    for (int j = 0; j < h; ++j)
        BL_HIP(hipMemcpyAsync(out + (size_t)j * row, rt->d_table + ((size_t)(y0 + j) * W + x0) * Hn, row * sizeof(uint16_t), hipMemcpyDeviceToHost,
                              ctx->stream));
    BL_HIP(hipStreamSynchronize(ctx->stream));
    return BL_OK;
}

extern "C" int bl_rangetable_directions(const bl_rangetable* rt, int32_t* out)
{
    int rc = rt_need_built(rt);
    if (rc) return rc;
    BL_CHECK_ARG(out != nullptr);
    BL_HIP(hipSetDevice(rt->ctx->device));
    BL_HIP(hipStreamSynchronize(rt->ctx->stream));                      // h_dirs is pinned and may be on its way: wait, then read it
    memcpy(out, rt->h_dirs, (size_t)rt->headings * sizeof(int2));
    return BL_OK;
}

extern "C" int bl_rangetable_info(const bl_rangetable* rt, bl_rangetable_info_t* out)
{
    BL_CHECK_ARG(rt != nullptr && out != nullptr);
    memset(out, 0, sizeof(*out));
    out->headings = rt->headings;
    out->built = rt->built ? 1 : 0;
    if (rt->built) {
        out->width = rt->frame.width; out->height = rt->frame.height; out->reach = rt->reach; out->occ_min = rt->occ_min;
        out->bytes = 2ll * rt->frame.width * rt->frame.height * rt->headings;
    }
    return BL_OK;
}

extern "C" int bl_rangetable_last_device_ms(const bl_rangetable* rt, float* ms)
{
    BL_CHECK_ARG(rt != nullptr && ms != nullptr);
    if (!rt->timed) { bl_set_error("bl_rangetable_last_device_ms: no kernel launched yet"); return BL_ERR_STATE; }
    BL_HIP(hipEventSynchronize(rt->ev_b));
    BL_HIP(hipEventElapsedTime(ms, rt->ev_a, rt->ev_b));
    return BL_OK;
}
