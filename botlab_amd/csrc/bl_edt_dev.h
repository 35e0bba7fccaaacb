// bl_edt_dev.h -- the two passes of the capped exact Euclidean transform as device functions, shared by the Euclidean distance grid
// (bl_edt.hip: sources are log-odds >= 0, the result is the uint16 code) and the likelihood field (bl_lfield.hip: sources are
// log-odds >= occ_min, the result is an int8 looked up by the code).  What differs between the two is the source threshold of the
// row pass and what the column pass does with a cell's squared distance; everything here is common.
//
// The squared distance separates: with g(x, y) the distance along the row to the nearest source OF THAT ROW,
// d^2(x, y) = min over dy of g(x, y + dy)^2 + dy^2.  Only |dy| <= R and g <= R can give a value <= R^2, so the row pass keeps
// min(g, R + 1) in one byte (R <= 254) and the column pass looks R rows up and down.
#ifndef BL_EDT_DEV_H
#define BL_EDT_DEV_H

#include "bl_internal.h"

#define EDT_TX 64            // columns of a tile = lanes of a wave
#define EDT_TY 64            // rows of a tile
#define EDT_WAVES 4
#define EDT_ROW_THREADS 256
#define EDT_ROW_WORDS 1024   // 64-bit source words of a row: rows up to 65536 cells (bl_dist: W + H < 65535)

// The row pass of the workgroup's row blockIdx.x (EDT_ROW_THREADS threads).  The row's source bits -- log-odds >= src_min -- go to
// s_mask, a 64-bit ballot word per 64 cells; a cell then finds the nearest set bit on either side with clz / ctz over at most
// (R + 1) / 64 + 2 words.  ORs the word "the map has a source" once per row that has one (the only atomic of the transform).
__device__ __forceinline__ void edt_rows_body(const int8_t* __restrict__ cells, uint8_t* __restrict__ g, unsigned int* __restrict__ has_source, int W,
                                              int R, int src_min, unsigned long long* s_mask, int* s_any)
{
    const int y = blockIdx.x;
    const int8_t* __restrict__ row = cells + (size_t)y * W;
    const int words = (W + 63) >> 6;
    if (threadIdx.x == 0) *s_any = 0;
    __syncthreads();
    bool any = false;
    for (int x = threadIdx.x; x < words * 64; x += EDT_ROW_THREADS) {             // whole waves: the ballot needs every lane of a word
        const bool src = x < W && row[x] >= src_min;
        const unsigned long long m = __ballot(src);
        if ((threadIdx.x & 63) == 0) { s_mask[x >> 6] = m; any = any || m != 0ull; }
    }
    if (any) *s_any = 1;
    __syncthreads();
    if (threadIdx.x == 0 && *s_any) atomicOr(has_source, 1u);
    const int cap = R + 1;
    for (int x = threadIdx.x; x < W; x += EDT_ROW_THREADS) {
        const int wi = x >> 6, b = x & 63;
        int best = cap;
        // nearest source at or left of x
        unsigned long long m = s_mask[wi] & (~0ull >> (63 - b));
        if (m) best = min(best, b - (63 - __clzll((long long)m)));
        else {
            int base = b + 1;                                                      // distance from x to bit 63 of the word before
            for (int k = wi - 1; k >= 0 && base < best; --k, base += 64) {
                m = s_mask[k];
                if (m) { best = min(best, base + __clzll((long long)m)); break; }
            }
        }
        // nearest source at or right of x
        m = s_mask[wi] & (~0ull << b);
        if (m) best = min(best, (int)__ffsll((unsigned long long)m) - 1 - b);
        else {
            int base = 64 - b;                                                     // distance from x to bit 0 of the next word
            for (int k = wi + 1; k < words && base < best; ++k, base += 64) {
                m = s_mask[k];
                if (m) { best = min(best, base + (int)__ffsll((unsigned long long)m) - 1); break; }
            }
        }
        g[(size_t)y * W + x] = (uint8_t)best;
    }
}

// The column pass stages g of the tile's rows (blockIdx.y) and of R rows above and below in s_g ([(EDT_TY + 2 R)][EDT_TX] bytes); a
// row outside the grid is staged as R + 1, "no source", never as a copy of the border row.  Lanes run along x.  Ends in the barrier.
__device__ __forceinline__ void edt_cols_stage(const uint8_t* __restrict__ g, uint8_t* s_g, int W, int H, int R)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = blockIdx.x * EDT_TX + lane, y0 = blockIdx.y * EDT_TY;
    const int rows = EDT_TY + 2 * R;
    const int cap = R + 1;
    for (int r = wave; r < rows; r += EDT_WAVES) {
        const int y = y0 - R + r;
        s_g[r * EDT_TX + lane] = (x < W && y >= 0 && y < H) ? g[(size_t)y * W + x] : (uint8_t)cap;
    }
    __syncthreads();
}

// The squared distance of the cell whose staged byte is col[0], uncapped (a value above R^2 means "farther than R").  It starts
// from g^2 and scans dy = 1, 2, ... both ways at once, stopping at the first dy with dy^2 >= best: every later candidate is at
// least dy^2, so the stop is exact.
__device__ __forceinline__ int edt_col_d2(const uint8_t* __restrict__ col, int R)
{
    const int g0 = col[0];
    int best = g0 * g0;
    for (int dy = 1; dy <= R; ++dy) {
        const int d2 = dy * dy;
        if (d2 >= best) break;
        const int a = col[-dy * EDT_TX], b = col[dy * EDT_TX];
        const int m = min(a, b);
        best = min(best, m * m + d2);
    }
    return best;
}

#endif
