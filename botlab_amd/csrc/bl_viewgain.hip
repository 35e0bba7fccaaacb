// bl_viewgain.hip -- the view gain (include/botlab_hip.h, "view gain"): how many distinct unknown cells a fan of rays cast from a
// candidate cell reaches before a blocking cell or the edge of the grid ends each ray.  No reference counterpart; the definition
// in the header is the contract and tests/view_gain_model.py restates it.  Everything is integer arithmetic.
//
//   k_view_gain   one workgroup per candidate: a bitmap of the (2R + 1)^2 window around the candidate in LDS, cleared; the rays
//                 dealt over the threads, each thread walking its rays cell by cell (the Bresenham walk of the definition, formed
//                 in registers from the ray's end offset) and OR-ing a bit with an LDS atomic for every unknown cell it passes;
//                 then a popcount of the bitmap, reduced over the workgroup.  The cells are read straight from the grid:
//                 neighbouring candidates share most of their window, so L2 serves most of it.
//
// The bitmap makes the count one of DISTINCT cells -- rays overlap near the candidate -- and an OR does not care in which order
// the rays arrive.
#include <math.h>
#include <string.h>

#include "bl_internal.h"

#define VG_MAX_RADIUS 255
#define VG_MAX_RAYS 4096
#define VG_MAX_THREADS 256

struct bl_viewgain {
    bl_ctx* ctx;
    bool have_params;
    bl_viewgain_params_t params;
    std::vector<int32_t>* h_ends;      // x, y per ray
    int* ends; int ends_cap;           // device: the same, one int2 per ray
    int threads;                       // workgroup size for this n_rays
    void* q_dev; size_t q_cap;         // candidates
    void* o_dev; size_t o_cap;         // gains
    uint32_t* bits_dev; size_t bits_cap;   // debug_seen: the bitmap of one candidate
};

struct vg_args {
    const int8_t* cells; int W, H;
    const int2* ends; int n_rays;
    int R, occupied_above, unknown_lo, unknown_hi;
    const int2* cand; int n;
    uint32_t* gain;
    uint32_t* bits_out;                // null, or where workgroup 0 leaves its bitmap
};

__global__ __launch_bounds__(VG_MAX_THREADS) void k_view_gain(vg_args a)
{
    extern __shared__ uint32_t s_bits[];
    __shared__ uint32_t s_sum;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int side = 2 * a.R + 1;
    const int words = (side * side + 31) >> 5;
    const int2 c = a.cand[blockIdx.x];
    const bool on_grid = c.x >= 0 && c.y >= 0 && c.x < a.W && c.y < a.H;          // the same for the whole workgroup
    for (int i = tid; i < words; i += nt) s_bits[i] = 0;
    if (tid == 0) s_sum = 0;
    __syncthreads();
    if (on_grid) {
        for (int k = tid; k < a.n_rays; k += nt) {
            const int2 e = a.ends[k];
            const int dx = abs(e.x), dy = abs(e.y);
            const int sx = (e.x > 0) - (e.x < 0), sy = (e.y > 0) - (e.y < 0);
            int steps = max(dx, dy);                  // the walk moves along the longer axis every time: it ends after this many
            int err = dx - dy, x = 0, y = 0;
            while (steps-- > 0) {
                const int e2 = 2 * err;
                if (e2 >= -dy) { err -= dy; x += sx; }
                if (e2 <= dx) { err += dx; y += sy; }
                const int gx = c.x + x, gy = c.y + y;
                if (gx < 0 || gy < 0 || gx >= a.W || gy >= a.H) break;
                const int v = a.cells[(size_t)gy * a.W + gx];
                if (v > a.occupied_above) break;
                if (v >= a.unknown_lo && v <= a.unknown_hi) {
                    const int bit = (y + a.R) * side + x + a.R;                   // |x|, |y| <= R: inside the window
                    atomicOr(&s_bits[bit >> 5], 1u << (bit & 31));
                }
            }
        }
    }
    __syncthreads();
    uint32_t mine = 0;
    for (int i = tid; i < words; i += nt) mine += (uint32_t)__popc(s_bits[i]);
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_down(mine, off, 64);
    if ((tid & 63) == 0 && mine) atomicAdd(&s_sum, mine);
    if (a.bits_out && blockIdx.x == 0)
        for (int i = tid; i < words; i += nt) a.bits_out[i] = s_bits[i];
    __syncthreads();
    if (tid == 0) a.gain[blockIdx.x] = s_sum;
}

// ---------------------------------------------------------------------------------------------------------------- host
extern "C" int bl_viewgain_create(bl_ctx* ctx, bl_viewgain** out)
{
    BL_CHECK_ARG(ctx != nullptr && out != nullptr);
    bl_viewgain* vg = new bl_viewgain();
    memset((void*)vg, 0, sizeof(*vg));
    vg->ctx = ctx;
    vg->h_ends = new std::vector<int32_t>();
    *out = vg;
    return BL_OK;
}

extern "C" void bl_viewgain_destroy(bl_viewgain* vg)
{
    if (!vg) return;
    (void)hipSetDevice(vg->ctx->device);
    (void)hipStreamSynchronize(vg->ctx->stream);
    void* dev[] = {vg->ends, vg->q_dev, vg->o_dev, vg->bits_dev};
    for (void* q : dev) if (q) (void)hipFree(q);
    delete vg->h_ends;
    delete vg;
}

extern "C" int bl_viewgain_set_params(bl_viewgain* vg, const bl_viewgain_params_t* p)
{
    BL_CHECK_ARG(vg != nullptr && p != nullptr);
    BL_CHECK_ARG(p->radius_cells >= 1 && p->radius_cells <= VG_MAX_RADIUS);
    BL_CHECK_ARG(p->n_rays >= 1 && p->n_rays <= VG_MAX_RAYS);
    BL_CHECK_ARG(p->occupied_above >= -128 && p->occupied_above <= 127);
    BL_CHECK_ARG(p->unknown_lo >= -128 && p->unknown_hi <= 127 && p->unknown_lo <= p->unknown_hi);
    bl_ctx* ctx = vg->ctx;
    BL_HIP(hipSetDevice(ctx->device));
    vg->have_params = false;
    const int K = p->n_rays;
    std::vector<int32_t> ends((size_t)K * 2);
    for (int k = 0; k < K; ++k) {                                     // the ray table of the definition, in double
        const double t = 2.0 * M_PI * (double)k / (double)K;
        ends[(size_t)2 * k] = (int32_t)lround((double)p->radius_cells * cos(t));
        ends[(size_t)2 * k + 1] = (int32_t)lround((double)p->radius_cells * sin(t));
    }
    if (K > vg->ends_cap) {
        BL_HIP(hipStreamSynchronize(ctx->stream));
        if (vg->ends) BL_HIP(hipFree(vg->ends));
        vg->ends = nullptr; vg->ends_cap = 0;
        BL_HIP(hipMalloc((void**)&vg->ends, (size_t)K * 8));
        vg->ends_cap = K;
    }
    BL_HIP(hipMemcpyAsync(vg->ends, ends.data(), (size_t)K * 8, hipMemcpyHostToDevice, ctx->stream));
    BL_HIP(hipStreamSynchronize(ctx->stream));                       // `ends` is pageable host memory
    *vg->h_ends = ends;
    // the workgroup size that wastes the fewest ray slots (ceil(K / threads) * threads), the larger one on a tie
    int best = VG_MAX_THREADS;
    for (int t = VG_MAX_THREADS; t >= 64; t >>= 1)
        if ((K + t - 1) / t * t < (K + best - 1) / best * best) best = t;
    vg->threads = best;
    vg->params = *p;
    vg->have_params = true;
    return BL_OK;
}

static int vg_need_params(const bl_viewgain* vg)
{
    if (!vg) { bl_set_error("bad argument: no view-gain handle"); return BL_ERR_ARG; }
    if (!vg->have_params) { bl_set_error("view gain has no parameters (bl_viewgain_set_params first)"); return BL_ERR_STATE; }
    return BL_OK;
}

extern "C" int bl_viewgain_ray_ends(bl_viewgain* vg, int32_t* xy, int* n)
{
    int rc = vg_need_params(vg);
    if (rc) return rc;
    if (n) *n = vg->params.n_rays;
    if (xy) memcpy(xy, vg->h_ends->data(), vg->h_ends->size() * 4);
    return BL_OK;
}

// n candidates already at vg->q_dev; gains to vg->o_dev
static int vg_launch(bl_viewgain* vg, const bl_grid* map, int n, uint32_t* bits_out)
{
    const bl_viewgain_params_t& p = vg->params;
    vg_args a;
    a.cells = map->cells; a.W = map->frame.width; a.H = map->frame.height;
    a.ends = (const int2*)vg->ends; a.n_rays = p.n_rays;
    a.R = p.radius_cells; a.occupied_above = p.occupied_above; a.unknown_lo = p.unknown_lo; a.unknown_hi = p.unknown_hi;
    a.cand = (const int2*)vg->q_dev; a.n = n;
    a.gain = (uint32_t*)vg->o_dev;
    a.bits_out = bits_out;
    const int side = 2 * p.radius_cells + 1;
    const size_t lds = (size_t)((side * side + 31) / 32) * 4;          // at most 32 644 bytes (R = 255)
    hipLaunchKernelGGL(k_view_gain, dim3((unsigned int)n), dim3((unsigned int)vg->threads), lds, vg->ctx->stream, a);
    BL_HIP(hipGetLastError());
    return BL_OK;
}

extern "C" int bl_viewgain_compute(bl_viewgain* vg, const bl_grid* map, const int32_t* xy_cells, int n, uint32_t* out_gain)
{
    int rc = vg_need_params(vg);
    if (rc) return rc;
    BL_CHECK_ARG(map != nullptr && map->ctx == vg->ctx && n >= 0 && (n == 0 || (xy_cells != nullptr && out_gain != nullptr)));
    if (n == 0) return BL_OK;
    bl_ctx* ctx = vg->ctx;
    BL_HIP(hipSetDevice(ctx->device));
    rc = bl_grow(&vg->q_dev, &vg->q_cap, (size_t)n * 8, false, ctx);
    if (!rc) rc = bl_grow(&vg->o_dev, &vg->o_cap, (size_t)n * 4, false, ctx);
    if (rc) return rc;
    BL_HIP(hipMemcpyAsync(vg->q_dev, xy_cells, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
    BL_HIP(hipStreamSynchronize(ctx->stream));                       // the caller's cells are pageable host memory
    rc = vg_launch(vg, map, n, nullptr);
    if (rc) return rc;
    BL_HIP(hipMemcpyAsync(out_gain, vg->o_dev, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    BL_HIP(hipStreamSynchronize(ctx->stream));
    return BL_OK;
}

extern "C" int bl_viewgain_debug_seen(bl_viewgain* vg, const bl_grid* map, int x, int y, uint8_t* out)
{
    int rc = vg_need_params(vg);
    if (rc) return rc;
    BL_CHECK_ARG(map != nullptr && map->ctx == vg->ctx && out != nullptr);
    bl_ctx* ctx = vg->ctx;
    BL_HIP(hipSetDevice(ctx->device));
    const int side = 2 * vg->params.radius_cells + 1;
    const size_t words = (size_t)(side * side + 31) / 32;
    rc = bl_grow(&vg->q_dev, &vg->q_cap, 8, false, ctx);
    if (!rc) rc = bl_grow(&vg->o_dev, &vg->o_cap, 4, false, ctx);
    if (!rc) rc = bl_grow((void**)&vg->bits_dev, &vg->bits_cap, words * 4, false, ctx);
    if (rc) return rc;
    const int32_t cell[2] = {x, y};
    BL_HIP(hipMemcpyAsync(vg->q_dev, cell, 8, hipMemcpyHostToDevice, ctx->stream));
    BL_HIP(hipStreamSynchronize(ctx->stream));
    rc = vg_launch(vg, map, 1, vg->bits_dev);
    if (rc) return rc;
    std::vector<uint32_t> bits(words);
    BL_HIP(hipMemcpyAsync(bits.data(), vg->bits_dev, words * 4, hipMemcpyDeviceToHost, ctx->stream));
    BL_HIP(hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < side * side; ++i) out[i] = (uint8_t)(bits[(size_t)i >> 5] >> (i & 31) & 1u);
    return BL_OK;
}
