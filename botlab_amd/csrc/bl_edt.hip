// bl_edt.hip -- the exact Euclidean distance transform of an occupancy grid (include/botlab_hip.h, "Euclidean distance grid"),
// capped at R cells, as two gfx950 kernels.  Nothing of this exists in the reference: its distance grid is the L1 transform of
// bl_planning.hip, which the search keeps.
//
// Sources are the cells with log-odds >= 0.  code(c) = min over sources of dx^2 + dy^2 when that is <= R^2, FAR = R^2 + 1 when it
// is more, 0xFFFF everywhere when the map has no source.  The squared distance separates: with g(x, y) the distance along the row
// to the nearest source OF THAT ROW, d^2(x, y) = min over dy of g(x, y + dy)^2 + dy^2.  Only |dy| <= R and g <= R can give a
// value <= R^2, so the row pass keeps min(g, R + 1) in one byte (R <= 254) and the column pass looks R rows up and down.
//
//   k_edt_rows  a workgroup per row.  The row's source bits go to LDS, a 64-bit ballot word per 64 cells; a cell then finds the
//               nearest set bit on either side with clz / ctz over at most (R + 1) / 64 + 2 words.  ORs the word "the map has a
//               source" once per row that has one (the only atomic of the transform).
//   k_edt_cols  a workgroup per tile of 64 columns x 64 rows.  g of its rows and of R rows above and below is staged in LDS
//               ((64 + 2 R) x 64 bytes: 36 KB at R = 254); a row outside the grid is staged as R + 1, "no source", never as a
//               copy of the border row.  Lanes run along x.  A cell starts from g^2 and scans dy = 1, 2, ... both ways at once,
//               stopping at the first dy with dy^2 >= best: every later candidate is at least dy^2, so the stop is exact.
//
// Integers only; no workgroup waits for another; the result does not depend on the launch shape.
#include "bl_edt_dev.h"

__global__ __launch_bounds__(EDT_ROW_THREADS) void k_edt_rows(const int8_t* __restrict__ cells, uint8_t* __restrict__ g, unsigned int* __restrict__ has_source,
                                                             int W, int R)
{
    __shared__ unsigned long long s_mask[EDT_ROW_WORDS];
    __shared__ int s_any;
    edt_rows_body(cells, g, has_source, W, R, 0, s_mask, &s_any);
}

__global__ __launch_bounds__(EDT_TX * EDT_WAVES) void k_edt_cols(const uint8_t* __restrict__ g, const unsigned int* __restrict__ has_source,
                                                                 uint16_t* __restrict__ codes, int W, int H, int R)
{
    extern __shared__ uint8_t s_g[];                                               // [(EDT_TY + 2 R)][EDT_TX]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = blockIdx.x * EDT_TX + lane, y0 = blockIdx.y * EDT_TY;
    edt_cols_stage(g, s_g, W, H, R);
    if (x >= W) return;
    const bool none = *has_source == 0u;
    const int far = R * R + 1;
    for (int ly = wave; ly < EDT_TY; ly += EDT_WAVES) {
        const int y = y0 + ly;
        if (y >= H) break;
        if (none) { codes[(size_t)y * W + x] = (uint16_t)0xFFFF; continue; }
        const int best = edt_col_d2(s_g + (R + ly) * EDT_TX + lane, R);
        codes[(size_t)y * W + x] = (uint16_t)(best < far ? best : far);
    }
}

// f[k] = (float)(sqrt((double)k) * (double)meters_per_cell), k = 0 .. R^2 + 1
void bl_edt_table(int R, float mpc, std::vector<float>* out)
{
    const int n = R * R + 2;
    out->resize((size_t)n);
    for (int k = 0; k < n; ++k) (*out)[(size_t)k] = (float)(sqrt((double)k) * (double)mpc);
}

// The transform of `cells` (W x H) into `codes`, on ctx's stream: the source word reset, the row pass, the column pass.
int bl_edt_transform(bl_ctx* ctx, const int8_t* cells, int W, int H, int R, uint8_t* g, unsigned int* has_source, uint16_t* codes)
{
    BL_CHECK_ARG(ctx != nullptr && cells != nullptr && g != nullptr && has_source != nullptr && codes != nullptr);
    BL_CHECK_ARG(W >= 1 && H >= 1 && W <= EDT_ROW_WORDS * 64 && R >= 1 && R <= BL_EDT_MAX_CELLS);
    BL_HIP(hipMemsetAsync(has_source, 0, sizeof(unsigned int), ctx->stream));
    hipLaunchKernelGGL(k_edt_rows, dim3((unsigned int)H), dim3(EDT_ROW_THREADS), 0, ctx->stream, cells, g, has_source, W, R);
    BL_HIP(hipGetLastError());
    const size_t lds = (size_t)(EDT_TY + 2 * R) * EDT_TX;                          // at most 36608 bytes
    hipLaunchKernelGGL(k_edt_cols, dim3((unsigned int)((W + EDT_TX - 1) / EDT_TX), (unsigned int)((H + EDT_TY - 1) / EDT_TY)), dim3(EDT_TX * EDT_WAVES),
                       lds, ctx->stream, (const uint8_t*)g, (const unsigned int*)has_source, codes, W, H, R);
    BL_HIP(hipGetLastError());
    return BL_OK;
}
