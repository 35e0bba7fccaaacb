// bl_navfield_dev.h -- what the kernels that read a navigation field share with the kernels that compute it (bl_navfield.hip): the
// handle, the per-cell cost, the cell of a pose and the move of the descent.  bl_localplan.hip scores the end of a rollout by the
// move bl_navfield_paths would take from it, so that rule lives here once.
#ifndef BL_NAVFIELD_DEV_H
#define BL_NAVFIELD_DEV_H

#include "bl_internal.h"

#define NAV_UNREACHED 0xFFFFFFFFu

struct bl_navfield {
    bl_ctx* ctx;
    size_t capacity;                   // cells allocated
    uint32_t* field;
    unsigned int* tile_flag;           // per tile: the last round it was listed for
    unsigned int* lists;               // 3 x tiles
    size_t tiles_cap;
    int32_t* table; int table_cap;     // device: per distance code, -1 not traversable, else the penalty
    int table_n;                       // its entries for the field computed last (the distance grid's table_n)
    unsigned int* state;               // device NST_WORDS
    unsigned int* h_state;             // pinned copy
    int32_t* goals; int goals_cap;     // device x, y pairs
    bl_frame frame; bool valid;
    const uint16_t* l1;                // the distance grid the field was computed from (for the descent's corner rule)
    const bl_dist* dist;
    bl_navfield_params_t params;
    int n_goals;
    std::vector<uint8_t>* h_trav; std::vector<int32_t>* h_pen;
    int64_t stats[5];
    // paths / gather scratch
    void* q_dev; size_t q_cap; void* q_host; size_t q_host_cap;
    void* o_dev; size_t o_cap;
};

__device__ __forceinline__ int nav_cost(const uint16_t* __restrict__ l1, const int32_t* __restrict__ table, int table_n, int W, int H,
                                        int x, int y)
{
    if (x < 0 || y < 0 || x >= W || y >= H) return -1;
    const int n = l1[(size_t)y * W + x];
    if (n == 0xFFFF || n >= table_n) return -1;
    return table[n];
}

// the moves in the order of the definition: (+x), (-x), (+y), (-y), (+x+y), (-x+y), (+x-y), (-x-y)
static __device__ __constant__ int NAV_DX[8] = {1, -1, 0, 0, 1, -1, 1, -1};
static __device__ __constant__ int NAV_DY[8] = {0, 0, 1, -1, 1, 1, -1, -1};

// the cell of a pose as the search finds it (global_position_to_grid_cell: a truncating cast), false when it is off the grid
__device__ __forceinline__ bool nav_pose_cell(const bl_frame& f, float gx, float gy, int* cx, int* cy)
{
    const double vx = ((double)gx - (double)f.ox) * (double)f.cpm, vy = ((double)gy - (double)f.oy) * (double)f.cpm;
    if (!(vx > -1.0 && vx < (double)f.width && vy > -1.0 && vy < (double)f.height)) return false;     // NaN: off the grid
    *cx = (int)vx; *cy = (int)vy;
    return true;
}

// the move the descent takes from the traversable cell (cx, cy): the allowed move minimising step + field(c'), -1 when no allowed
// move leads to a reached cell; *to_f is the field of the cell it leads to
__device__ __forceinline__ int nav_descent_move(const uint32_t* __restrict__ field, const uint16_t* __restrict__ l1,
                                                const int32_t* __restrict__ table, int table_n, int W, int H, int cx, int cy, uint32_t* to_f)
{
    const bool px = nav_cost(l1, table, table_n, W, H, cx + 1, cy) >= 0, mx = nav_cost(l1, table, table_n, W, H, cx - 1, cy) >= 0;
    const bool py = nav_cost(l1, table, table_n, W, H, cx, cy + 1) >= 0, my = nav_cost(l1, table, table_n, W, H, cx, cy - 1) >= 0;
    uint32_t best = NAV_UNREACHED, best_f = 0;
    int bm = -1;
    for (int m = 0; m < 8; ++m) {
        const int dx = NAV_DX[m], dy = NAV_DY[m];
        bool ok;
        if (m < 4) ok = m == 0 ? px : m == 1 ? mx : m == 2 ? py : my;
        else ok = (dx > 0 ? px : mx) && (dy > 0 ? py : my) && nav_cost(l1, table, table_n, W, H, cx + dx, cy + dy) >= 0;
        if (!ok) continue;
        const uint32_t v = field[(size_t)(cy + dy) * W + cx + dx];
        if (v == NAV_UNREACHED) continue;
        const uint32_t w = v + (m < 4 ? 10u : 14u);
        if (w < best) { best = w; best_f = v; bm = m; }       // ties: the first move in the fixed order
    }
    *to_f = best_f;
    return bm;
}

#endif  // BL_NAVFIELD_DEV_H
