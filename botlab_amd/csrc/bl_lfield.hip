// bl_lfield.hip -- the likelihood field (include/botlab_hip.h, "likelihood field"): an int8 grid whose cells hold a Gaussian of
// their distance to the nearest occupied cell.  No reference counterpart; the definition in the header is the contract and
// tests/likelihood_field_model.py restates it.
//
// The expensive half is the capped exact Euclidean transform of bl_edt.hip, and the two passes are the same device functions
// (bl_edt_dev.h) with two differences: a source is a cell with log-odds >= occ_min, not >= 0, and the column pass ends in a table
// look-up that stores a byte, not in a uint16 code.
//
//   k_lfield_rows  a workgroup per row: edt_rows_body with the threshold occ_min.
//   k_lfield_cols  a workgroup per tile of 64 x 64 cells: g of its rows and of R rows of halo in LDS ((64 + 2 R) x 64 bytes), the
//                  table T[0 .. R^2 + 1] behind it (at most 4098 bytes: 16386 in all at R = 64).  A cell's squared distance, capped
//                  at FAR = R^2 + 1, indexes the table.  A map without a source (the has_source word, read on the device: no host
//                  round trip) stores T[FAR] = 0 everywhere.
//
// Integers only on the device; no workgroup waits for another; the result does not depend on the launch shape.
#include <math.h>
#include <string.h>

#include "bl_edt_dev.h"

#define LF_TABLE_MAX (BL_LFIELD_MAX_CELLS * BL_LFIELD_MAX_CELLS + 2)

__global__ __launch_bounds__(EDT_ROW_THREADS) void k_lfield_rows(const int8_t* __restrict__ cells, uint8_t* __restrict__ g, unsigned int* __restrict__ has_source,
                                                                int W, int R, int occ_min)
{
    __shared__ unsigned long long s_mask[EDT_ROW_WORDS];
    __shared__ int s_any;
    edt_rows_body(cells, g, has_source, W, R, occ_min, s_mask, &s_any);
}

__global__ __launch_bounds__(EDT_TX * EDT_WAVES) void k_lfield_cols(const uint8_t* __restrict__ g, const unsigned int* __restrict__ has_source,
                                                                    const int8_t* __restrict__ table, int8_t* __restrict__ field, int W, int H, int R)
{
    extern __shared__ uint8_t s_g[];                                               // [(EDT_TY + 2 R)][EDT_TX], then the table [R^2 + 2]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = blockIdx.x * EDT_TX + lane, y0 = blockIdx.y * EDT_TY;
    const int far = R * R + 1;
    int8_t* s_t = (int8_t*)(s_g + (EDT_TY + 2 * R) * EDT_TX);
#pragma unroll 1
    for (int k = threadIdx.x; k <= far; k += EDT_TX * EDT_WAVES) s_t[k] = table[k];
    edt_cols_stage(g, s_g, W, H, R);                                               // (its barrier covers the table too)
    if (x >= W) return;
    const bool none = *has_source == 0u;
    for (int ly = wave; ly < EDT_TY; ly += EDT_WAVES) {
        const int y = y0 + ly;
        if (y >= H) break;
        if (none) { field[(size_t)y * W + x] = s_t[far]; continue; }
        const int best = edt_col_d2(s_g + (R + ly) * EDT_TX + lane, R);
        field[(size_t)y * W + x] = s_t[best < far ? best : far];
    }
}

// ---------------------------------------------------------------------------------------------------------------- host
struct bl_lfield {
    bl_ctx* ctx;
    bl_lfield_params_t params; bool have_params;
    bl_grid* grid;                                // the field; null before the first compute
    uint8_t* d_g; size_t d_g_cap;                 // the row pass's result
    unsigned int* d_src;                          // "the map has a source"
    int8_t* d_table;                              // LF_TABLE_MAX bytes
    int8_t* h_table;                              // pinned, LF_TABLE_MAX bytes: what d_table holds once ev_table has passed
    int table_n;                                  // entries of the last compute's table (0: none yet)
    hipEvent_t ev_table, ev_a, ev_b;
    bool computed;
};

extern "C" int bl_lfield_create(bl_ctx* ctx, bl_lfield** out)
{
    BL_CHECK_ARG(ctx != nullptr && out != nullptr);
    BL_HIP(hipSetDevice(ctx->device));
    bl_lfield* lf = new bl_lfield();
    memset((void*)lf, 0, sizeof(*lf));
    lf->ctx = ctx;
    hipError_t e = hipMalloc((void**)&lf->d_src, sizeof(unsigned int));
    if (e == hipSuccess) e = hipMalloc((void**)&lf->d_table, LF_TABLE_MAX);
    if (e == hipSuccess) e = hipHostMalloc((void**)&lf->h_table, LF_TABLE_MAX, hipHostMallocDefault);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&lf->ev_table, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreate(&lf->ev_a);
    if (e == hipSuccess) e = hipEventCreate(&lf->ev_b);
    if (e != hipSuccess) {
        bl_set_error("bl_lfield_create: %s", hipGetErrorString(e));
        bl_lfield_destroy(lf);
        return BL_ERR_HIP;
    }
    *out = lf;
    return BL_OK;
}

extern "C" void bl_lfield_destroy(bl_lfield* lf)
{
    if (!lf) return;
    (void)hipSetDevice(lf->ctx->device);
    (void)hipStreamSynchronize(lf->ctx->stream);
    if (lf->grid) bl_grid_destroy(lf->grid);
    if (lf->d_g) (void)hipFree(lf->d_g);
    if (lf->d_src) (void)hipFree(lf->d_src);
    if (lf->d_table) (void)hipFree(lf->d_table);
    if (lf->h_table) (void)hipHostFree(lf->h_table);
    if (lf->ev_table) (void)hipEventDestroy(lf->ev_table);
    if (lf->ev_a) (void)hipEventDestroy(lf->ev_a);
    if (lf->ev_b) (void)hipEventDestroy(lf->ev_b);
    delete lf;
}

extern "C" int bl_lfield_set_params(bl_lfield* lf, const bl_lfield_params_t* p)
{
    BL_CHECK_ARG(lf != nullptr && p != nullptr);
    BL_CHECK_ARG(isfinite(p->sigma) && p->sigma > 0.0f);
    BL_CHECK_ARG(p->max_cells >= 1 && p->max_cells <= BL_LFIELD_MAX_CELLS);
    BL_CHECK_ARG(p->occ_min >= 1 && p->occ_min <= 127);
    BL_CHECK_ARG(p->peak >= 1 && p->peak <= 127);
    lf->params = *p;
    lf->have_params = true;
    return BL_OK;
}

// T[k] = (int8) floor(peak * exp(-(k m^2) / (2 s^2)) + 0.5), k = 0 .. R^2; T[R^2 + 1] = 0
static void lf_table(const bl_lfield_params_t& p, float mpc, int8_t* T)
{
    const int R2 = p.max_cells * p.max_cells;
    const double m = (double)mpc, s = (double)p.sigma;
    for (int k = 0; k <= R2; ++k) T[k] = (int8_t)floor((double)p.peak * exp(-((double)k * (m * m)) / (2.0 * (s * s))) + 0.5);
    T[R2 + 1] = 0;
}

extern "C" int bl_lfield_compute(bl_lfield* lf, const bl_grid* map)
{
    BL_CHECK_ARG(lf != nullptr && map != nullptr);
    if (!lf->have_params) { bl_set_error("likelihood field has no parameters (bl_lfield_set_params first)"); return BL_ERR_STATE; }
    bl_ctx* ctx = lf->ctx;
    BL_CHECK_ARG(map->ctx == ctx);
    const int W = map->frame.width, H = map->frame.height, R = lf->params.max_cells;
    BL_CHECK_ARG(W >= 1 && H >= 1 && W <= EDT_ROW_WORDS * 64);
    BL_HIP(hipSetDevice(ctx->device));
    const size_t cells = (size_t)W * H;
    if (!lf->grid || lf->grid->frame.width != W || lf->grid->frame.height != H) {
        bl_grid* fresh = nullptr;
        int rc = bl_grid_create(ctx, W, H, map->frame.mpc, map->frame.cpm, map->frame.ox, map->frame.oy, &fresh);
        if (rc) return rc;
        if (lf->grid) bl_grid_destroy(lf->grid);
        lf->grid = fresh;
    }
    if (cells > lf->d_g_cap) {
        BL_HIP(hipStreamSynchronize(ctx->stream));
        if (lf->d_g) BL_HIP(hipFree(lf->d_g));
        lf->d_g = nullptr; lf->d_g_cap = 0;
        BL_HIP(hipMalloc((void**)&lf->d_g, cells));
        lf->d_g_cap = cells;
    }
    // the table: uploaded only when it differs from the one the device holds (or is about to hold)
    int8_t T[LF_TABLE_MAX];
    const int n = R * R + 2;
    lf_table(lf->params, map->frame.mpc, T);
    if (n != lf->table_n || memcmp(T, lf->h_table, (size_t)n) != 0) {
        if (lf->table_n) BL_HIP(hipEventSynchronize(lf->ev_table));               // the pinned buffer may still be on its way
        memcpy(lf->h_table, T, (size_t)n);
        lf->table_n = n;
        BL_HIP(hipMemcpyAsync(lf->d_table, lf->h_table, (size_t)n, hipMemcpyHostToDevice, ctx->stream));
        BL_HIP(hipEventRecord(lf->ev_table, ctx->stream));
    }
    // the cells are rewritten wholesale: what an upload, a reset and a copy do (bl_internal.h, struct bl_grid)
    bl_grid* f = lf->grid;
    f->frame = map->frame;
    f->mirror_valid = false;
    (void)bl_grid_new_lineage(f);
    BL_HIP(hipEventRecord(lf->ev_a, ctx->stream));
    BL_HIP(hipMemsetAsync(lf->d_src, 0, sizeof(unsigned int), ctx->stream));
    hipLaunchKernelGGL(k_lfield_rows, dim3((unsigned int)H), dim3(EDT_ROW_THREADS), 0, ctx->stream, (const int8_t*)map->cells, lf->d_g, lf->d_src, W, R,
                       (int)lf->params.occ_min);
    BL_HIP(hipGetLastError());
    const size_t lds = (size_t)(EDT_TY + 2 * R) * EDT_TX + (size_t)n;             // at most 16386 bytes
    hipLaunchKernelGGL(k_lfield_cols, dim3((unsigned int)((W + EDT_TX - 1) / EDT_TX), (unsigned int)((H + EDT_TY - 1) / EDT_TY)), dim3(EDT_TX * EDT_WAVES),
                       lds, ctx->stream, (const uint8_t*)lf->d_g, (const unsigned int*)lf->d_src, (const int8_t*)lf->d_table, f->cells, W, H, R);
    BL_HIP(hipGetLastError());
    BL_HIP(hipEventRecord(lf->ev_b, ctx->stream));
    lf->computed = true;
    return BL_OK;
}

extern "C" const bl_grid* bl_lfield_grid(const bl_lfield* lf) { return lf ? lf->grid : nullptr; }

extern "C" int bl_lfield_table(const bl_lfield* lf, int8_t* T, int* n)
{
    BL_CHECK_ARG(lf != nullptr && n != nullptr);
    if (!lf->computed) { bl_set_error("bl_lfield_table: no bl_lfield_compute yet"); return BL_ERR_STATE; }
    *n = lf->table_n;
    if (T) memcpy(T, lf->h_table, (size_t)lf->table_n);
    return BL_OK;
}

extern "C" int bl_lfield_last_device_ms(const bl_lfield* lf, float* ms)
{
    BL_CHECK_ARG(lf != nullptr && ms != nullptr);
    if (!lf->computed) { bl_set_error("bl_lfield_last_device_ms: no bl_lfield_compute yet"); return BL_ERR_STATE; }
    BL_HIP(hipEventSynchronize(lf->ev_b));
    BL_HIP(hipEventElapsedTime(ms, lf->ev_a, lf->ev_b));
    return BL_OK;
}
