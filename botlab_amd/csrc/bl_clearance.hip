// bl_clearance.hip -- the clearance grid (include/botlab_hip.h, "clearance grid"): per cell of a map the Chebyshev distance to the
// nearest occupied cell, capped at C, one uint8, so that the beam model's walk can leap over empty space (k_beam_leap, bl_beam.hip).
// No reference counterpart; the definition in the header is the contract and tests/clearance_model.py restates it.
//
// The Chebyshev distance separates: D(x, y) = min over dy of max(|dy|, R(x, y + dy)), R the distance along a row to that row's
// nearest occupied cell.  Two passes over a box of cells (the whole grid for a build, the changed box widened by C for an update):
//   k_clr_rows    a workgroup per CLR_THREADS / 64 chunks, a WAVE PER 64 CELLS of a row (chunks aligned to 64 in x).  The occupancy of
//                 the chunk and of the nw = (C + 62) / 64 <= 4 chunks on either side, one ballot each; a lane's distance to the
//                 nearest set bit on its right by count-trailing-zeros and on its left by count-leading-zeros, in its own word first
//                 and then outward word by word; min(C, .) stored as a uint8 of the intermediate `rows`.  A word farther than nw away
//                 holds no cell nearer than C.
//   k_clr_cols    a THREAD PER CELL, threads along x: best = rows[y][x], then dy = 1, 2, .. while dy < best:
//                 best = min(best, max(dy, min(rows[y - dy][x], rows[y + dy][x]))), rows outside the grid skipped.  The loop length is
//                 the answer itself; a wave's loads are 64 consecutive bytes of a row.
// After the cells of a box changed, `rows` changes only in the box's rows, within C of it in x; D only within C of it in x and y.
// The map bytes and the intermediate go through L2; an LDS-tiled form was not built and is not measured.
//
// Integers only; no atomics; no workgroup waits for another; no result depends on the launch shape.
#include <string.h>

#include "bl_internal.h"

#define CLR_THREADS 256
#define CLR_MAX_CAP 255
#define CLR_MAX_WORDS 4                   // (CLR_MAX_CAP + 62) / 64
#define CLR_MAX_CELLS (1ll << 30)

struct clr_args {
    const int8_t* cells; int W, H, occ_min, cap;
    int x0, y0, x1, y1;                                    // the box, inclusive, inside the grid
    uint8_t* rows; uint8_t* grid;
};

__global__ __launch_bounds__(CLR_THREADS) void k_clr_rows(clr_args a)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c0 = a.x0 >> 6, nchunks = (a.x1 >> 6) - c0 + 1;
    const long long item = (long long)blockIdx.x * (CLR_THREADS / 64) + wave;
    if (item >= (long long)nchunks * (a.y1 - a.y0 + 1)) return;          // (uniform over the wave)
    const int y = a.y0 + (int)(item / nchunks), chunk = c0 + (int)(item % nchunks);
    const int nw = (a.cap + 62) >> 6;
    const int8_t* row = a.cells + (size_t)y * a.W;
    unsigned long long word[2 * CLR_MAX_WORDS + 1];                       // word[CLR_MAX_WORDS + j]: chunk + j
#pragma unroll
    for (int j = -CLR_MAX_WORDS; j <= CLR_MAX_WORDS; ++j) {
        const int x = (chunk + j) * 64 + lane;
        bool occ = false;
        if (j >= -nw && j <= nw && x >= 0 && x < a.W) occ = row[x] >= a.occ_min;
        word[CLR_MAX_WORDS + j] = __ballot(occ);
    }
    const unsigned long long own = word[CLR_MAX_WORDS];
    int right = CLR_MAX_CAP, left = CLR_MAX_CAP;
    const unsigned long long up = own >> lane, down = own << (63 - lane);
    if (up) {
        right = __builtin_ctzll(up);
    } else {
        bool found = false;
#pragma unroll
        for (int j = 1; j <= CLR_MAX_WORDS; ++j) {
            const unsigned long long w = word[CLR_MAX_WORDS + j];
            if (!found && w) { right = 64 * j - lane + __builtin_ctzll(w); found = true; }
        }
    }
    if (down) {
        left = __builtin_clzll(down);
    } else {
        bool found = false;
#pragma unroll
        for (int j = 1; j <= CLR_MAX_WORDS; ++j) {
            const unsigned long long w = word[CLR_MAX_WORDS - j];
            if (!found && w) { left = lane + 64 * (j - 1) + 1 + __builtin_clzll(w); found = true; }
        }
    }
    const int x = chunk * 64 + lane;
    if (x >= a.x0 && x <= a.x1) a.rows[(size_t)y * a.W + x] = (uint8_t)min(a.cap, min(left, right));
}

__global__ __launch_bounds__(CLR_THREADS) void k_clr_cols(clr_args a)
{
    const int nxb = (a.x1 - a.x0) / CLR_THREADS + 1;                    // a row of the box takes nxb workgroups
    const int x = a.x0 + (int)(blockIdx.x % nxb) * CLR_THREADS + threadIdx.x, y = a.y0 + (int)(blockIdx.x / nxb);
    if (x > a.x1) return;
    const uint8_t* col = a.rows + x;
    int best = col[(size_t)y * a.W];
    for (int dy = 1; dy < best; ++dy) {
        int v = CLR_MAX_CAP;
        if (y - dy >= 0) v = col[(size_t)(y - dy) * a.W];
        if (y + dy < a.H) v = min(v, (int)col[(size_t)(y + dy) * a.W]);
        best = min(best, max(dy, v));
    }
    a.grid[(size_t)y * a.W + x] = (uint8_t)best;
}

// ---------------------------------------------------------------------------------------------------------------- host
struct bl_clearance {
    bl_ctx* ctx;
    int cap;
    bool built, timed;
    bl_frame frame; int occ_min;                          // of the last build
    uint8_t* d_grid; uint8_t* d_rows; size_t cells_cap;    // cells allocated, each
    hipEvent_t ev_a, ev_b;
};

void bl_clearance_view_host(const bl_clearance* cl, bl_clearance_view* out)
{
    out->ctx = cl->ctx; out->built = cl->built; out->frame = cl->frame; out->cap = cl->cap; out->occ_min = cl->occ_min; out->d_grid = cl->d_grid;
}

extern "C" int bl_clearance_create(bl_ctx* ctx, int cap, bl_clearance** out)
{
    BL_CHECK_ARG(ctx != nullptr && out != nullptr);
    BL_CHECK_ARG(cap >= 1 && cap <= CLR_MAX_CAP);
    BL_HIP(hipSetDevice(ctx->device));
    bl_clearance* cl = new bl_clearance();
    memset((void*)cl, 0, sizeof(*cl));
    cl->ctx = ctx; cl->cap = cap;
    hipError_t e = hipEventCreate(&cl->ev_a);
    if (e == hipSuccess) e = hipEventCreate(&cl->ev_b);
    if (e != hipSuccess) {
        bl_set_error("bl_clearance_create: %s", hipGetErrorString(e));
        bl_clearance_destroy(cl);
        return BL_ERR_HIP;
    }
    *out = cl;
    return BL_OK;
}

extern "C" void bl_clearance_destroy(bl_clearance* cl)
{
    if (!cl) return;
    (void)hipSetDevice(cl->ctx->device);
    (void)hipStreamSynchronize(cl->ctx->stream);
    if (cl->d_grid) (void)hipFree(cl->d_grid);
    if (cl->d_rows) (void)hipFree(cl->d_rows);
    if (cl->ev_a) (void)hipEventDestroy(cl->ev_a);
    if (cl->ev_b) (void)hipEventDestroy(cl->ev_b);
    delete cl;
}

// the two passes after the cells x0 .. x1, y0 .. y1 (inside the grid, not empty) of the built frame changed (all of them: a build)
static int clr_launch(bl_clearance* cl, const bl_grid* map, int x0, int y0, int x1, int y1)
{
    bl_ctx* ctx = cl->ctx;
    const int W = cl->frame.width, H = cl->frame.height, C = cl->cap;
    clr_args a;
    a.cells = map->cells; a.W = W; a.H = H; a.occ_min = cl->occ_min; a.cap = C;
    a.rows = cl->d_rows; a.grid = cl->d_grid;
    a.x0 = x0 - C > 0 ? x0 - C : 0; a.x1 = x1 + C < W - 1 ? x1 + C : W - 1;
    a.y0 = y0; a.y1 = y1;
    const long long items = (long long)((a.x1 >> 6) - (a.x0 >> 6) + 1) * (a.y1 - a.y0 + 1);
    BL_HIP(hipEventRecord(cl->ev_a, ctx->stream));
    hipLaunchKernelGGL(k_clr_rows, dim3((unsigned int)((items + CLR_THREADS / 64 - 1) / (CLR_THREADS / 64))), dim3(CLR_THREADS), 0, ctx->stream, a);
    a.y0 = y0 - C > 0 ? y0 - C : 0; a.y1 = y1 + C < H - 1 ? y1 + C : H - 1;
    const long long blocks = (long long)((a.x1 - a.x0) / CLR_THREADS + 1) * (a.y1 - a.y0 + 1);    // < 2^31: W * H <= 2^30
    hipLaunchKernelGGL(k_clr_cols, dim3((unsigned int)blocks), dim3(CLR_THREADS), 0, ctx->stream, a);
    BL_HIP(hipGetLastError());
    BL_HIP(hipEventRecord(cl->ev_b, ctx->stream));
    cl->timed = true;
    return BL_OK;
}

extern "C" int bl_clearance_build(bl_clearance* cl, const bl_grid* map, int occ_min)
{
    BL_CHECK_ARG(cl != nullptr && map != nullptr && map->ctx == cl->ctx);
    BL_CHECK_ARG(occ_min >= 1 && occ_min <= 127);
    const int W = map->frame.width, H = map->frame.height;
    BL_CHECK_ARG(W >= 1 && H >= 1 && (long long)W * H <= CLR_MAX_CELLS);
    const size_t cells = (size_t)W * H;
    bl_ctx* ctx = cl->ctx;
    BL_HIP(hipSetDevice(ctx->device));
    if (cells > cl->cells_cap) {
        BL_HIP(hipStreamSynchronize(ctx->stream));                      // the old grid may be read
        if (cl->d_grid) BL_HIP(hipFree(cl->d_grid));
        cl->d_grid = nullptr; cl->cells_cap = 0; cl->built = false;
        if (cl->d_rows) BL_HIP(hipFree(cl->d_rows));
        cl->d_rows = nullptr;
        BL_HIP(hipMalloc((void**)&cl->d_grid, cells));
        BL_HIP(hipMalloc((void**)&cl->d_rows, cells));
        cl->cells_cap = cells;
    }
    cl->built = false;
    cl->frame = map->frame; cl->occ_min = occ_min;
    const int rc = clr_launch(cl, map, 0, 0, W - 1, H - 1);
    if (rc) return rc;
    cl->built = true;
    return BL_OK;
}

static int clr_need_built(const bl_clearance* cl)
{
    if (!cl) { bl_set_error("bad argument: no clearance grid handle"); return BL_ERR_ARG; }
    if (!cl->built) { bl_set_error("clearance grid not built (bl_clearance_build first)"); return BL_ERR_STATE; }
    return BL_OK;
}

extern "C" int bl_clearance_update(bl_clearance* cl, const bl_grid* map, int x0, int y0, int x1, int y1)
{
    int rc = clr_need_built(cl);
    if (rc) return rc;
    BL_CHECK_ARG(map != nullptr && map->ctx == cl->ctx);
    const int W = cl->frame.width, H = cl->frame.height;
    BL_CHECK_ARG(map->frame.width == W && map->frame.height == H);
    if (x1 < x0 || y1 < y0 || x1 < 0 || y1 < 0 || x0 >= W || y0 >= H) return BL_OK;
    BL_HIP(hipSetDevice(cl->ctx->device));                              // (the corners may lie anywhere in int: clipped before they are widened)
    return clr_launch(cl, map, x0 > 0 ? x0 : 0, y0 > 0 ? y0 : 0, x1 < W - 1 ? x1 : W - 1, y1 < H - 1 ? y1 : H - 1);
}

extern "C" int bl_clearance_read(bl_clearance* cl, int x0, int y0, int w, int h, uint8_t* out)
{
    int rc = clr_need_built(cl);
    if (rc) return rc;
    const int W = cl->frame.width, H = cl->frame.height;
    BL_CHECK_ARG(out != nullptr && x0 >= 0 && y0 >= 0 && w >= 1 && h >= 1 && w <= W - x0 && h <= H - y0);
    bl_ctx* ctx = cl->ctx;
    BL_HIP(hipSetDevice(ctx->device));
    if (w == W) {
        BL_HIP(hipMemcpyAsync(out, cl->d_grid + (size_t)y0 * W, (size_t)w * h, hipMemcpyDeviceToHost, ctx->stream));
    } else {
        for (int j = 0; j < h; ++j)
            BL_HIP(hipMemcpyAsync(out + (size_t)j * w, cl->d_grid + (size_t)(y0 + j) * W + x0, (size_t)w, hipMemcpyDeviceToHost, ctx->stream));
    }
    BL_HIP(hipStreamSynchronize(ctx->stream));
    return BL_OK;
}

extern "C" int bl_clearance_info(const bl_clearance* cl, bl_clearance_info_t* out)
{
    BL_CHECK_ARG(cl != nullptr && out != nullptr);
    memset(out, 0, sizeof(*out));
    out->cap = cl->cap;
    out->built = cl->built ? 1 : 0;
    if (cl->built) {
        out->width = cl->frame.width; out->height = cl->frame.height; out->occ_min = cl->occ_min;
        out->bytes = (int64_t)cl->frame.width * cl->frame.height;
    }
    return BL_OK;
}

extern "C" int bl_clearance_last_device_ms(const bl_clearance* cl, float* ms)
{
    BL_CHECK_ARG(cl != nullptr && ms != nullptr);
    if (!cl->timed) { bl_set_error("bl_clearance_last_device_ms: no kernel launched yet"); return BL_ERR_STATE; }
    BL_HIP(hipEventSynchronize(cl->ev_b));
    BL_HIP(hipEventElapsedTime(ms, cl->ev_a, cl->ev_b));
    return BL_OK;
}
