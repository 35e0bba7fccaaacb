// bl_navfield.hip -- the goal-rooted navigation field (include/botlab_hip.h, "navigation field"): the exact cost-to-go of every
// cell of a distance grid to a set of goal cells over 8-connected moves, and steepest-descent paths through it.  No reference
// counterpart; the definition in the header is the contract and tests/nav_field_model.py restates it.
//
// The field is the least fixed point of  field(c) = penalty(c) + min over allowed moves (step + field(c'))  with field = 0 on the
// goal set.  All quantities are non-negative integers and every update is a monotone minimum, so ANY order of relaxations reaches
// the same fixed point: the kernels are free to work tile by tile, on whatever values of the neighbouring tiles they happen to
// read, as long as a tile is relaxed again after a cell its halo shows got lower.
//
//   k_nav_init    every cell UNREACHED; counts the traversable cells (the bound on the rounds)
//   k_nav_goals   the goal set (listed cells dilated by reach_cells, traversable ones only) -> 0; their tiles and the tiles around
//                 them form the list of round 1
//   k_nav_relax   one round: a workgroup per listed tile stages the tile + a one-cell halo (field, and penalty / traversability
//                 through the per-distance table) in LDS, sweeps it to its fixed point there, stores the cells that got lower and
//                 lists the neighbouring tiles whose halo they are part of for the NEXT round
//   k_nav_paths   one thread per start: the descent
//
// No workgroup waits for another: a round reads the list the previous launch wrote, and an empty list ends every workgroup at
// once.  The host enqueues rounds a group at a time and reads the next round's list length from a pinned word behind each group.
#include <math.h>
#include <string.h>

#include "bl_internal.h"
#include "bl_navfield_dev.h"                // the handle, nav_cost, nav_pose_cell, the moves and nav_descent_move

#define NAV_TILE 32                    // cells a side: one thread per cell, 1024 threads
#define NAV_HALO (NAV_TILE + 2)
#define NAV_RELAX_GRID 1024            // workgroups of a round; each walks the list with this stride
#define NAV_MAX_TILE_SWEEPS 4096       // a 34 x 34 Bellman-Ford needs at most 1156; beyond: the tile lists itself again
#define NAV_MAX_REACH 1024
#define NAV_MAX_GAIN 4095

// words of bl_navfield::state (device)
#define NST_COUNT 0                    // [3] length of the tile list of round r at r % 3
#define NST_TRAVERSABLE 3
#define NST_GOALSET 4
#define NST_ROUNDS 5                   // rounds that found a non-empty list
#define NST_TILES 6                    // [2] tiles relaxed (64 bits)
#define NST_SWEEPS 8                   // [2] in-LDS sweeps over a tile (64 bits)
#define NST_REACHED 10
#define NST_WORDS 16

struct nav_geom { int W, H, TX, TY; };

// ---------------------------------------------------------------------------------------------------------------- kernels
__global__ __launch_bounds__(256) void k_nav_init(uint32_t* __restrict__ field, const uint16_t* __restrict__ l1,
                                                  const int32_t* __restrict__ table, int table_n, size_t n, unsigned int* state)
{
    unsigned int mine = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        field[i] = NAV_UNREACHED;
        const int d = l1[i];
        mine += (d != 0xFFFF && d < table_n && table[d] >= 0) ? 1u : 0u;
    }
    __shared__ unsigned int s_sum;
    if (threadIdx.x == 0) s_sum = 0;
    __syncthreads();
    if (mine) atomicAdd(&s_sum, mine);
    __syncthreads();
    if (threadIdx.x == 0 && s_sum) atomicAdd(&state[NST_TRAVERSABLE], s_sum);
}

// list tile t for round `round` (once)
__device__ __forceinline__ void nav_list_tile(unsigned int* tile_flag, unsigned int* lists, unsigned int* state, int ntiles, int t,
                                              unsigned int round)
{
    const unsigned int old = atomicMax(&tile_flag[t], round);
    if (old < round) {
        const unsigned int at = atomicAdd(&state[NST_COUNT + round % 3], 1u);
        if (at < (unsigned int)ntiles) lists[(size_t)(round % 3) * ntiles + at] = (unsigned int)t;
    }
}

// one thread per (listed goal, row of its reach window)
__global__ __launch_bounds__(256) void k_nav_goals(uint32_t* __restrict__ field, const uint16_t* __restrict__ l1,
                                                   const int32_t* __restrict__ table, int table_n, nav_geom g,
                                                   const int32_t* __restrict__ goals, int n_goals, int reach, unsigned int* tile_flag,
                                                   unsigned int* lists, unsigned int* state)
{
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    const int rows = 2 * reach + 1;
    if (id >= (long long)n_goals * rows) return;
    const int k = (int)(id / rows), dy = (int)(id % rows) - reach;
    const int gx = goals[2 * k], gy = goals[2 * k + 1];
    if (gx < 0 || gy < 0 || gx >= g.W || gy >= g.H) return;          // a listed cell outside the grid contributes nothing
    const int y = gy + dy;
    if (y < 0 || y >= g.H) return;
    const int ntiles = g.TX * g.TY;
    for (int x = max(gx - reach, 0); x <= min(gx + reach, g.W - 1); ++x) {
        if (nav_cost(l1, table, table_n, g.W, g.H, x, y) < 0) continue;
        if (atomicExch(&field[(size_t)y * g.W + x], 0u) != 0u) atomicAdd(&state[NST_GOALSET], 1u);
        const int tx = x / NAV_TILE, ty = y / NAV_TILE;
        for (int oy = -1; oy <= 1; ++oy)
            for (int ox = -1; ox <= 1; ++ox) {
                const int ux = tx + ox, uy = ty + oy;
                if (ux >= 0 && uy >= 0 && ux < g.TX && uy < g.TY) nav_list_tile(tile_flag, lists, state, ntiles, uy * g.TX + ux, 1u);
            }
    }
}

__global__ __launch_bounds__(NAV_TILE * NAV_TILE) void k_nav_relax(uint32_t* __restrict__ field, const uint16_t* __restrict__ l1,
                                                                   const int32_t* __restrict__ table, int table_n, nav_geom g,
                                                                   unsigned int* tile_flag, unsigned int* lists, unsigned int* state,
                                                                   unsigned int round)
{
    __shared__ uint32_t s_f[NAV_HALO * NAV_HALO];
    __shared__ int32_t s_c[NAV_HALO * NAV_HALO];
    __shared__ unsigned int s_marks;
    const int ntiles = g.TX * g.TY;
    const unsigned int count = min(state[NST_COUNT + round % 3], (unsigned int)ntiles);
    const int tid = threadIdx.x;
    if (blockIdx.x == 0 && tid == 0) {
        state[NST_COUNT + (round + 2) % 3] = 0;          // the list of round - 1 (read by the launch before this one) becomes round + 2's
        if (count) atomicAdd(&state[NST_ROUNDS], 1u);
    }
    const unsigned int* list = lists + (size_t)(round % 3) * ntiles;
    const int lx = tid % NAV_TILE, ly = tid / NAV_TILE;
    const int at = (ly + 1) * NAV_HALO + lx + 1;
    for (unsigned int i = blockIdx.x; i < count; i += gridDim.x) {
        const int t = (int)list[i];
        const int x0 = (t % g.TX) * NAV_TILE, y0 = (t / g.TX) * NAV_TILE;
        if (tid == 0) s_marks = 0;
        for (int j = tid; j < NAV_HALO * NAV_HALO; j += NAV_TILE * NAV_TILE) {
            const int x = x0 - 1 + j % NAV_HALO, y = y0 - 1 + j / NAV_HALO;
            const int c = nav_cost(l1, table, table_n, g.W, g.H, x, y);
            s_c[j] = c;
            s_f[j] = c >= 0 ? field[(size_t)y * g.W + x] : NAV_UNREACHED;
        }
        __syncthreads();
        const int pen = s_c[at];
        const uint32_t loaded = s_f[at];
        uint32_t cur = loaded;
        // which of the eight moves this cell may take: both ends traversable, a diagonal only past two traversable side cells
        unsigned int allowed = 0;
        if (pen >= 0) {
            const bool px = s_c[at + 1] >= 0, mx = s_c[at - 1] >= 0, py = s_c[at + NAV_HALO] >= 0, my = s_c[at - NAV_HALO] >= 0;
            allowed = (px ? 1u : 0u) | (mx ? 2u : 0u) | (py ? 4u : 0u) | (my ? 8u : 0u);
            if (px && py && s_c[at + NAV_HALO + 1] >= 0) allowed |= 16u;
            if (mx && py && s_c[at + NAV_HALO - 1] >= 0) allowed |= 32u;
            if (px && my && s_c[at - NAV_HALO + 1] >= 0) allowed |= 64u;
            if (mx && my && s_c[at - NAV_HALO - 1] >= 0) allowed |= 128u;
        }
        int sweeps = 0;
        int changed;
        do {
            uint32_t best = NAV_UNREACHED;
            if (allowed && cur != 0) {
#pragma unroll
                for (int m = 0; m < 8; ++m) {
                    if (!(allowed >> m & 1u)) continue;
                    const uint32_t v = s_f[at + NAV_DY[m] * NAV_HALO + NAV_DX[m]];
                    if (v == NAV_UNREACHED) continue;
                    const uint32_t w = v + (m < 4 ? 10u : 14u);
                    best = min(best, w);
                }
                if (best != NAV_UNREACHED) best += (uint32_t)pen;
            }
            changed = best < cur;
            if (changed) { cur = best; s_f[at] = best; }      // a neighbour reads the old or the new value: both are bounds from above
            ++sweeps;
        } while (__syncthreads_or(changed) && sweeps < NAV_MAX_TILE_SWEEPS);
        const bool inside = x0 + lx < g.W && y0 + ly < g.H;
        if (inside && cur < loaded) {
            field[(size_t)(y0 + ly) * g.W + x0 + lx] = cur;
            // the tiles whose halo holds this cell
            unsigned int mk = 0;
            const bool w = lx == 0, e = lx == NAV_TILE - 1, s = ly == 0, n = ly == NAV_TILE - 1;
            if (w) mk |= 1u; if (e) mk |= 2u; if (s) mk |= 4u; if (n) mk |= 8u;
            if (w && s) mk |= 16u; if (e && s) mk |= 32u; if (w && n) mk |= 64u; if (e && n) mk |= 128u;
            if (sweeps >= NAV_MAX_TILE_SWEEPS) mk |= 256u;
            if (mk) atomicOr(&s_marks, mk);
        }
        __syncthreads();
        if (tid < 9 && (s_marks >> tid & 1u)) {
            const int ox = tid == 8 ? 0 : (tid == 0 || tid == 4 || tid == 6) ? -1 : (tid == 1 || tid == 5 || tid == 7) ? 1 : 0;
            const int oy = tid == 8 ? 0 : (tid == 2 || tid == 4 || tid == 5) ? -1 : (tid == 3 || tid == 6 || tid == 7) ? 1 : 0;
            const int ux = t % g.TX + ox, uy = t / g.TX + oy;
            if (ux >= 0 && uy >= 0 && ux < g.TX && uy < g.TY) nav_list_tile(tile_flag, lists, state, ntiles, uy * g.TX + ux, round + 1);
        }
        if (tid == 0) {
            atomicAdd((unsigned long long*)&state[NST_TILES], 1ull);
            atomicAdd((unsigned long long*)&state[NST_SWEEPS], (unsigned long long)sweeps);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_nav_count_reached(const uint32_t* __restrict__ field, size_t n, unsigned int* state)
{
    unsigned int mine = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) mine += field[i] != NAV_UNREACHED ? 1u : 0u;
    __shared__ unsigned int s_sum;
    if (threadIdx.x == 0) s_sum = 0;
    __syncthreads();
    if (mine) atomicAdd(&s_sum, mine);
    __syncthreads();
    if (threadIdx.x == 0 && s_sum) atomicAdd(&state[NST_REACHED], s_sum);
}

__global__ __launch_bounds__(256) void k_nav_gather(const uint32_t* __restrict__ field, int W, int H, const int2* __restrict__ q, int n,
                                                    uint32_t* __restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int2 c = q[i];
    out[i] = (c.x >= 0 && c.y >= 0 && c.x < W && c.y < H) ? field[(size_t)c.y * W + c.x] : NAV_UNREACHED;
}

struct nav_path_args {
    const uint32_t* field; const uint16_t* l1; const int32_t* table; int table_n;
    bl_frame frame;
    const int32_t* goals; int n_goals, reach;
    const bl_pose_xyt_t* starts; int n;
    bl_pose_xyt_t* out; int cap;
    int* lens; int32_t* labels; uint32_t* costs;
    float theta[8];                    // atan2f(dy, dx) of the eight moves, from the host's libm
};

__global__ __launch_bounds__(64) void k_nav_paths(nav_path_args a)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= a.n) return;
    const int W = a.frame.width, H = a.frame.height;
    const bl_pose_xyt_t start = a.starts[i];
    bl_pose_xyt_t* out = a.out + (size_t)i * a.cap;
    if (a.cap >= 1) out[0] = start;
    int len = 1, label = -1;
    uint32_t cost = NAV_UNREACHED;
    int cx = 0, cy = 0;
    bool on = nav_pose_cell(a.frame, start.x, start.y, &cx, &cy);
    if (on && nav_cost(a.l1, a.table, a.table_n, W, H, cx, cy) >= 0) cost = a.field[(size_t)cy * W + cx];
    else on = false;
    uint32_t f = cost;
    if (on && f != NAV_UNREACHED) {
        const long long max_steps = (long long)W * H;
        for (long long step = 0; f != 0 && step < max_steps; ++step) {
            uint32_t best_f = 0;
            const int bm = nav_descent_move(a.field, a.l1, a.table, a.table_n, W, H, cx, cy, &best_f);
            if (bm < 0 || best_f >= f) break;                         // cannot happen on a field at its fixed point
            cx += NAV_DX[bm]; cy += NAV_DY[bm]; f = best_f;
            if (len < a.cap) {
                bl_pose_xyt_t p;
                p.utime = start.utime;
                p.x = (float)((double)a.frame.ox + (double)cx * (double)a.frame.mpc);      // as bl_astar_search writes a path cell
                p.y = (float)((double)a.frame.oy + (double)cy * (double)a.frame.mpc);
                p.theta = a.theta[bm];
                out[len] = p;
            }
            ++len;
        }
        if (f == 0) {                                                 // on the goal set: the lowest listed index that covers the cell
            for (int k = 0; k < a.n_goals; ++k) {
                const int gx = a.goals[2 * k], gy = a.goals[2 * k + 1];
                if (gx < 0 || gy < 0 || gx >= W || gy >= H) continue;
                if (abs(gx - cx) <= a.reach && abs(gy - cy) <= a.reach) { label = k; break; }
            }
        }
    }
    a.lens[i] = len; a.labels[i] = label; a.costs[i] = cost;
}

// ---------------------------------------------------------------------------------------------------------------- host
extern "C" int bl_navfield_create(bl_ctx* ctx, bl_navfield** out)
{
    BL_CHECK_ARG(ctx != nullptr && out != nullptr);
    BL_HIP(hipSetDevice(ctx->device));
    bl_navfield* nf = new bl_navfield();
    memset((void*)nf, 0, sizeof(*nf));
    nf->ctx = ctx;
    nf->h_trav = new std::vector<uint8_t>();
    nf->h_pen = new std::vector<int32_t>();
    hipError_t e = hipMalloc((void**)&nf->state, NST_WORDS * sizeof(unsigned int));
    if (e == hipSuccess) e = hipHostMalloc((void**)&nf->h_state, NST_WORDS * sizeof(unsigned int), hipHostMallocDefault);
    if (e != hipSuccess) {
        bl_set_error("bl_navfield_create: %s", hipGetErrorString(e));
        bl_navfield_destroy(nf);
        return BL_ERR_HIP;
    }
    *out = nf;
    return BL_OK;
}

extern "C" void bl_navfield_destroy(bl_navfield* nf)
{
    if (!nf) return;
    (void)hipSetDevice(nf->ctx->device);
    (void)hipStreamSynchronize(nf->ctx->stream);
    void* dev[] = {nf->field, nf->tile_flag, nf->lists, nf->table, nf->state, nf->goals, nf->q_dev, nf->o_dev};
    for (void* q : dev) if (q) (void)hipFree(q);
    if (nf->h_state) (void)hipHostFree(nf->h_state);
    if (nf->q_host) (void)hipHostFree(nf->q_host);
    delete nf->h_trav;
    delete nf->h_pen;
    delete nf;
}

// the two per-distance tables of the definition, in double on the host
static void nav_build_tables(bl_navfield* nf, const float* f, int ln, const bl_navfield_params_t& p)
{
    nf->h_trav->assign((size_t)ln, 0);
    nf->h_pen->assign((size_t)ln, 0);
    const double minD = p.minDistanceToObstacle, maxD = p.maxDistanceWithCost;
    for (int n = 0; n < ln; ++n) {
        if (!bl_search_traversable(f[n], minD)) continue;             // the search's isValid, by the search's own code
        (*nf->h_trav)[n] = 1;
        const double d = (double)f[n];
        if (d >= maxD || maxD <= minD) continue;
        (*nf->h_pen)[n] = (int32_t)floor((double)p.obstacle_gain * pow((maxD - d) / (maxD - minD), p.distanceCostExponent));
    }
}

static int nav_params_ok(const bl_navfield_params_t* p)
{
    BL_CHECK_ARG(p != nullptr);
    BL_CHECK_ARG(p->obstacle_gain >= 0 && p->obstacle_gain <= NAV_MAX_GAIN);
    BL_CHECK_ARG(p->reach_cells >= 0 && p->reach_cells <= NAV_MAX_REACH);
    BL_CHECK_ARG(p->minDistanceToObstacle == p->minDistanceToObstacle && p->maxDistanceWithCost == p->maxDistanceWithCost);
    BL_CHECK_ARG(p->distanceCostExponent >= 0.0 && p->distanceCostExponent < INFINITY);    // a traversable cell's penalty stays within [0, gain]
    return BL_OK;
}

extern "C" int bl_navfield_compute(bl_navfield* nf, const bl_dist* dist, const bl_navfield_params_t* params, const int32_t* goal_xy_cells,
                                   int n_goals)
{
    BL_CHECK_ARG(nf != nullptr);
    nf->valid = false;                                               // a compute that is refused leaves no field: the last one answers for other arguments
    BL_CHECK_ARG(dist != nullptr && n_goals >= 0 && (n_goals == 0 || goal_xy_cells != nullptr));
    int rc = nav_params_ok(params);
    if (rc) return rc;
    bl_ctx* ctx = nf->ctx;
    bl_dist_host_view v;
    rc = bl_dist_view_host(dist, &v);
    if (rc) return rc;
    BL_CHECK_ARG(v.ctx == ctx);
    const int W = v.frame.width, H = v.frame.height;
    const size_t n = (size_t)W * H;
    if ((double)n * (double)(14 + params->obstacle_gain) > 4294967294.0) {
        bl_set_error("bl_navfield_compute: %d x %d cells at obstacle_gain %d could exceed a 32-bit cost", W, H, params->obstacle_gain);
        return BL_ERR_ARG;
    }
    BL_HIP(hipSetDevice(ctx->device));
    const nav_geom g = {W, H, (W + NAV_TILE - 1) / NAV_TILE, (H + NAV_TILE - 1) / NAV_TILE};
    const size_t ntiles = (size_t)g.TX * g.TY;
    if (n > nf->capacity) {
        BL_HIP(hipStreamSynchronize(ctx->stream));
        if (nf->field) BL_HIP(hipFree(nf->field));
        nf->field = nullptr; nf->capacity = 0;
        BL_HIP(hipMalloc((void**)&nf->field, n * 4));
        nf->capacity = n;
    }
    if (ntiles > nf->tiles_cap) {
        BL_HIP(hipStreamSynchronize(ctx->stream));
        if (nf->tile_flag) BL_HIP(hipFree(nf->tile_flag));
        if (nf->lists) BL_HIP(hipFree(nf->lists));
        nf->tile_flag = nullptr; nf->lists = nullptr; nf->tiles_cap = 0;
        BL_HIP(hipMalloc((void**)&nf->tile_flag, ntiles * 4));
        BL_HIP(hipMalloc((void**)&nf->lists, 3 * ntiles * 4));
        nf->tiles_cap = ntiles;
    }
    const int ln = v.table_n;
    if (v.metric == BL_DIST_EUCLIDEAN && params->maxDistanceWithCost > params->minDistanceToObstacle &&
        params->maxDistanceWithCost > (double)v.lut_host[v.max_cells * v.max_cells]) {
        bl_set_error("bl_navfield_compute: maxDistanceWithCost %g lies beyond the Euclidean grid's cap of %d cells (%g m): a far cell's penalty would be "
                     "priced from a lower bound of its distance", params->maxDistanceWithCost, v.max_cells, (double)v.lut_host[v.max_cells * v.max_cells]);
        return BL_ERR_ARG;
    }
    if (ln > nf->table_cap) {
        BL_HIP(hipStreamSynchronize(ctx->stream));
        if (nf->table) BL_HIP(hipFree(nf->table));
        nf->table = nullptr; nf->table_cap = 0;
        BL_HIP(hipMalloc((void**)&nf->table, (size_t)ln * 4));
        nf->table_cap = ln;
    }
    if (n_goals > nf->goals_cap) {
        BL_HIP(hipStreamSynchronize(ctx->stream));
        if (nf->goals) BL_HIP(hipFree(nf->goals));
        nf->goals = nullptr; nf->goals_cap = 0;
        BL_HIP(hipMalloc((void**)&nf->goals, (size_t)n_goals * 8));
        nf->goals_cap = n_goals;
    }
    nav_build_tables(nf, v.lut_host, ln, *params);
    std::vector<int32_t> tab((size_t)ln);
    for (int i = 0; i < ln; ++i) tab[(size_t)i] = (*nf->h_trav)[(size_t)i] ? (*nf->h_pen)[(size_t)i] : -1;
    BL_HIP(hipMemcpyAsync(nf->table, tab.data(), (size_t)ln * 4, hipMemcpyHostToDevice, ctx->stream));
    if (n_goals) BL_HIP(hipMemcpyAsync(nf->goals, goal_xy_cells, (size_t)n_goals * 8, hipMemcpyHostToDevice, ctx->stream));
    BL_HIP(hipMemsetAsync(nf->state, 0, NST_WORDS * sizeof(unsigned int), ctx->stream));
    BL_HIP(hipMemsetAsync(nf->tile_flag, 0, ntiles * 4, ctx->stream));
    BL_HIP(hipStreamSynchronize(ctx->stream));                       // `tab` and the caller's goals are pageable host memory
    const unsigned int blocks = (unsigned int)((n + 255) / 256 > 16384 ? 16384 : (n + 255) / 256);
    hipLaunchKernelGGL(k_nav_init, dim3(blocks), dim3(256), 0, ctx->stream, nf->field, v.l1, nf->table, ln, n, nf->state);
    BL_HIP(hipGetLastError());
    const int reach = params->reach_cells;
    if (n_goals) {
        const long long threads = (long long)n_goals * (2 * reach + 1);
        hipLaunchKernelGGL(k_nav_goals, dim3((unsigned int)((threads + 255) / 256)), dim3(256), 0, ctx->stream, nf->field, v.l1, nf->table, ln, g,
                           nf->goals, n_goals, reach, nf->tile_flag, nf->lists, nf->state);
        BL_HIP(hipGetLastError());
    }
    // rounds, a group at a time; behind each group the host reads the words
    const unsigned int relax_grid = (unsigned int)(ntiles < NAV_RELAX_GRID ? ntiles : NAV_RELAX_GRID);
    unsigned int round = 1;
    int group = 4;
    bool done = false, over = false;
    while (!done) {
        for (int k = 0; k < group; ++k, ++round) {
            hipLaunchKernelGGL(k_nav_relax, dim3(relax_grid), dim3(NAV_TILE * NAV_TILE), 0, ctx->stream, nf->field, v.l1, nf->table, ln, g,
                               nf->tile_flag, nf->lists, nf->state, round);
        }
        BL_HIP(hipGetLastError());
        BL_HIP(hipMemcpyAsync(nf->h_state, nf->state, NST_WORDS * sizeof(unsigned int), hipMemcpyDeviceToHost, ctx->stream));
        BL_HIP(hipStreamSynchronize(ctx->stream));
        done = nf->h_state[NST_COUNT + round % 3] == 0;                // the list of the round that would come next
        // Bellman-Ford: a cell whose cheapest path crosses k tile borders is final after round k + 1, so no list is left
        // after round (traversable cells) + 1
        if (!done && (uint64_t)round > (uint64_t)nf->h_state[NST_TRAVERSABLE] + 1) { over = true; break; }
        if (group < 64) group *= 2;
    }
    if (over) {
        bl_set_error("bl_navfield_compute: still relaxing after %u rounds on %u traversable cells", round - 1, nf->h_state[NST_TRAVERSABLE]);
        return BL_ERR_STATE;
    }
    hipLaunchKernelGGL(k_nav_count_reached, dim3(blocks), dim3(256), 0, ctx->stream, nf->field, n, nf->state);
    BL_HIP(hipGetLastError());
    BL_HIP(hipMemcpyAsync(nf->h_state, nf->state, NST_WORDS * sizeof(unsigned int), hipMemcpyDeviceToHost, ctx->stream));
    BL_HIP(hipStreamSynchronize(ctx->stream));
    rc = bl_dist_view_host(dist, &v);                                 // a whole-grid transform that gave up shows here
    if (rc) return rc;
    const unsigned int* s = nf->h_state;
    nf->stats[0] = s[NST_ROUNDS];
    nf->stats[1] = (int64_t)((uint64_t)s[NST_SWEEPS] | (uint64_t)s[NST_SWEEPS + 1] << 32);
    nf->stats[2] = s[NST_TRAVERSABLE];
    nf->stats[3] = s[NST_REACHED];
    nf->stats[4] = s[NST_GOALSET];
    nf->frame = v.frame; nf->l1 = v.l1; nf->dist = dist; nf->params = *params; nf->n_goals = n_goals; nf->table_n = ln;
    nf->valid = true;
    return BL_OK;
}

extern "C" int bl_navfield_compute_to_pose(bl_navfield* nf, const bl_dist* dist, const bl_navfield_params_t* params, const bl_pose_xyt_t* goal)
{
    BL_CHECK_ARG(nf != nullptr && dist != nullptr && goal != nullptr);
    bl_dist_host_view v;
    int rc = bl_dist_view_host(dist, &v);
    if (rc) return rc;
    int32_t cell[2] = {-1, -1};
    const double vx = ((double)goal->x - (double)v.frame.ox) * (double)v.frame.cpm, vy = ((double)goal->y - (double)v.frame.oy) * (double)v.frame.cpm;
    if (vx > -1.0 && vx < (double)v.frame.width && vy > -1.0 && vy < (double)v.frame.height) { cell[0] = (int32_t)vx; cell[1] = (int32_t)vy; }
    return bl_navfield_compute(nf, dist, params, cell, 1);
}

static int nav_need_field(const bl_navfield* nf)
{
    if (!nf || !nf->valid) { bl_set_error("navigation field not computed (bl_navfield_compute first)"); return nf ? BL_ERR_STATE : BL_ERR_ARG; }
    return BL_OK;
}

extern "C" int bl_navfield_paths(bl_navfield* nf, const bl_pose_xyt_t* starts, int n, bl_pose_xyt_t* out_paths, int cap_each, int* out_lens,
                                 int32_t* out_goal, uint32_t* out_cost)
{
    int rc = nav_need_field(nf);
    if (rc) return rc;
    BL_CHECK_ARG(n >= 0 && cap_each >= 1 && (n == 0 || (starts != nullptr && out_paths != nullptr && out_lens != nullptr)));
    if (n == 0) return BL_OK;
    bl_ctx* ctx = nf->ctx;
    BL_HIP(hipSetDevice(ctx->device));
    bl_dist_host_view v;
    rc = bl_dist_view_host(nf->dist, &v);
    if (rc) return rc;
    if (v.l1 != nf->l1 || v.frame.width != nf->frame.width || v.frame.height != nf->frame.height || v.table_n != nf->table_n) {
        bl_set_error("bl_navfield_paths: the distance grid was resized since the field was computed");
        return BL_ERR_STATE;
    }
    const size_t tail = (size_t)n * 12;                                // lens, labels, costs
    const size_t out_bytes = (size_t)n * cap_each * sizeof(bl_pose_xyt_t) + tail;
    rc = bl_grow(&nf->q_dev, &nf->q_cap, (size_t)n * sizeof(bl_pose_xyt_t), false, ctx);
    if (!rc) rc = bl_grow(&nf->o_dev, &nf->o_cap, out_bytes, false, ctx);
    if (rc) return rc;
    BL_HIP(hipMemcpyAsync(nf->q_dev, starts, (size_t)n * sizeof(bl_pose_xyt_t), hipMemcpyHostToDevice, ctx->stream));
    BL_HIP(hipStreamSynchronize(ctx->stream));
    nav_path_args a;
    a.field = nf->field; a.l1 = nf->l1; a.table = nf->table; a.table_n = nf->table_n;
    a.frame = nf->frame;
    a.goals = nf->goals; a.n_goals = nf->n_goals; a.reach = nf->params.reach_cells;
    a.starts = (const bl_pose_xyt_t*)nf->q_dev; a.n = n;
    a.out = (bl_pose_xyt_t*)nf->o_dev; a.cap = cap_each;
    char* tail_dev = (char*)nf->o_dev + (size_t)n * cap_each * sizeof(bl_pose_xyt_t);
    a.lens = (int*)tail_dev; a.labels = (int32_t*)(tail_dev + (size_t)n * 4); a.costs = (uint32_t*)(tail_dev + (size_t)n * 8);
    static const int dx[8] = {1, -1, 0, 0, 1, -1, 1, -1}, dy[8] = {0, 0, 1, -1, 1, 1, -1, -1};
    for (int m = 0; m < 8; ++m) a.theta[m] = atan2f((float)dy[m], (float)dx[m]);
    hipLaunchKernelGGL(k_nav_paths, dim3((n + 63) / 64), dim3(64), 0, ctx->stream, a);
    BL_HIP(hipGetLastError());
    std::vector<int32_t> t((size_t)n * 3);
    BL_HIP(hipMemcpyAsync(t.data(), tail_dev, tail, hipMemcpyDeviceToHost, ctx->stream));
    BL_HIP(hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < n; ++i) {
        const int len = t[(size_t)i];
        out_lens[i] = len;
        if (out_goal) out_goal[i] = t[(size_t)n + i];
        if (out_cost) out_cost[i] = (uint32_t)t[(size_t)2 * n + i];
        const int wr = len < cap_each ? len : cap_each;
        BL_HIP(hipMemcpyAsync(out_paths + (size_t)i * cap_each, (const bl_pose_xyt_t*)nf->o_dev + (size_t)i * cap_each, (size_t)wr * sizeof(bl_pose_xyt_t),
                              hipMemcpyDeviceToHost, ctx->stream));
    }
    BL_HIP(hipStreamSynchronize(ctx->stream));
    return BL_OK;
}

extern "C" int bl_navfield_gather(bl_navfield* nf, const int32_t* xy_cells, int n, uint32_t* out)
{
    int rc = nav_need_field(nf);
    if (rc) return rc;
    BL_CHECK_ARG(n >= 0 && (n == 0 || (xy_cells != nullptr && out != nullptr)));
    if (n == 0) return BL_OK;
    bl_ctx* ctx = nf->ctx;
    BL_HIP(hipSetDevice(ctx->device));
    rc = bl_grow(&nf->q_dev, &nf->q_cap, (size_t)n * 8, false, ctx);
    if (!rc) rc = bl_grow(&nf->o_dev, &nf->o_cap, (size_t)n * 4, false, ctx);
    if (rc) return rc;
    BL_HIP(hipMemcpyAsync(nf->q_dev, xy_cells, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
    BL_HIP(hipStreamSynchronize(ctx->stream));
    hipLaunchKernelGGL(k_nav_gather, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, nf->field, nf->frame.width, nf->frame.height,
                       (const int2*)nf->q_dev, n, (uint32_t*)nf->o_dev);
    BL_HIP(hipGetLastError());
    BL_HIP(hipMemcpyAsync(out, nf->o_dev, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    BL_HIP(hipStreamSynchronize(ctx->stream));
    return BL_OK;
}

extern "C" int bl_navfield_download(bl_navfield* nf, uint32_t* cells)
{
    int rc = nav_need_field(nf);
    if (rc) return rc;
    BL_CHECK_ARG(cells != nullptr);
    BL_HIP(hipSetDevice(nf->ctx->device));
    BL_HIP(hipMemcpyAsync(cells, nf->field, (size_t)nf->frame.width * nf->frame.height * 4, hipMemcpyDeviceToHost, nf->ctx->stream));
    BL_HIP(hipStreamSynchronize(nf->ctx->stream));
    return BL_OK;
}

extern "C" int bl_navfield_shape(const bl_navfield* nf, int* width, int* height)
{
    int rc = nav_need_field(nf);
    if (rc) return rc;
    if (width) *width = nf->frame.width;
    if (height) *height = nf->frame.height;
    return BL_OK;
}

extern "C" void* bl_navfield_device_ptr(bl_navfield* nf) { return nf && nf->valid ? (void*)nf->field : nullptr; }

extern "C" int bl_navfield_tables(bl_navfield* nf, uint8_t* traversable, int32_t* penalty, int* n)
{
    int rc = nav_need_field(nf);
    if (rc) return rc;
    const size_t ln = nf->h_trav->size();
    if (n) *n = (int)ln;
    if (traversable) memcpy(traversable, nf->h_trav->data(), ln);
    if (penalty) memcpy(penalty, nf->h_pen->data(), ln * 4);
    return BL_OK;
}

extern "C" int bl_navfield_stats(bl_navfield* nf, int64_t* out)
{
    int rc = nav_need_field(nf);
    if (rc) return rc;
    BL_CHECK_ARG(out != nullptr);
    for (int i = 0; i < 5; ++i) out[i] = nf->stats[i];
    return BL_OK;
}
