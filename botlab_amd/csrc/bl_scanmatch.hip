// bl_scanmatch.hip -- correlative scan matching (Olson 2009, exhaustive form): the pose of a scan against the map from a bounded
// window of (dx, dy, dtheta) around a centre pose, without odometry.  The definition is in include/botlab_hip.h; the numpy
// restatement the tests compare with, bit for bit, is "the model" (tests/scan_match_model.py).
//
// One stream-ordered sequence per match on the ctx stream: header + rays H2D, k_sm_raster, k_sm_score, k_sm_final, result D2H.
//   k_sm_raster  one thread per (heading, ray): the ray's endpoint cell at that heading, scoreRay's float arithmetic; endpoints that
//                no shift of the window can bring onto the grid become a sentinel; the bounding box of the others is kept (one
//                vector atomic min / max per wave and bound).
//   k_sm_score   a workgroup owns one heading and a slice of its (dj, di) candidates, lanes along di (row-major over the window), so
//                the lanes of a wave read consecutive bytes of a map row for one ray.  The heading's endpoints are wave-uniform:
//                64 at a time sit one per lane and are broadcast through scalar registers.  When the bounding box widened by the window and
//                clipped to the grid fits in the LDS, the positive part of those cells is staged there (path 0); otherwise the grid is read directly (path 1).
//                Every workgroup leaves its best 64-bit key and how many of its candidates share that key's score.
//   k_sm_final   one workgroup: maximum of the keys (order-independent), sum of the tie counts, the result struct.
// bl_scanmatch_match_prior runs the same sequence with the prior forms of the last two (k_sm_score_prior,
// k_sm_final_prior: the objective score - pen in the key, the volume and the tie count) and, when the moments are wanted, behind them
//   k_sm_moments        a streaming pass over the stored objective volume: a wave owns whole rows of di, every lane a fixed di; the
//                       weight of a candidate from one multiplication by a reciprocal of half_life and a 64-entry table in LDS;
//                       64-bit integer sums, one record per workgroup, no atomics.
//   k_sm_moments_final  one workgroup: the sum of the records, the sub-cell fractions from the winner's six neighbours.
// The rules these kernels, the wide match's (below) and the per-particle matcher (bl_rbslam_match.h) have in common -- the key, the map
// window, the endpoint of a ray, the lookup sum, a workgroup's best key, the pose of the winner, the valid rays -- are in
// bl_scanmatch_dev.h.  The bodies of the plain and the prior sequence -- rasteriser, scoring, result, moments -- are in
// bl_scanmatch_seq_dev.h: the kernels here are their one-match launches, bl_loopclose.hip's a match per loop candidate.
#include <string.h>

#define BL_SM_HELPER                   // this translation unit defines the header's two helpers with external linkage (bindings call them)
#include "bl_internal.h"
#include "bl_scanmatch_dev.h"          // every rule the per-particle matcher (bl_rbslam_match.h) scores by as well
#include "bl_scanmatch_seq_dev.h"      // the header of a match and the bodies of this sequence: the batched matches of bl_loopclose.hip run them too

// the wide match's (below): what k_sm_raster reads and writes is its base, and base.result is the result
struct smw_head {
    sm_head base;
    int32_t hlog, nbx, nby, exhaustive;
    long long candidates;
    unsigned int kept; int32_t pad;
    unsigned long long scored;
};

// Capacities are in bytes (bl_grow).  Every match ends in a stream synchronize, so no two are in flight on a handle and one header
// and one set of ray buffers serve the plain, the prior and the wide match.
struct bl_scanmatch {
    bl_ctx* ctx = nullptr;
    smw_head* d_head = nullptr;        // the plain match uses its base
    float* d_rays = nullptr; size_t rays_bytes = 0;        // ranges[ray_cap] | thetas[ray_cap]
    int ray_cap = 0;
    int2* d_ends = nullptr; size_t ends_cap = 0;           // [heading][ray]
    sm_block_best* d_best = nullptr; size_t best_cap = 0;  // one per workgroup of k_sm_score
    int32_t* d_volume = nullptr; size_t volume_cap = 0;
    void* staging = nullptr;           // pinned: smw_head | ranges | thetas
    size_t staging_bytes = 0;
    bool volume_kept = false;
    int vol_nx = 0, vol_ny = 0, vol_nt = 0;
    int last_path = -1;
    // the match with a prior: the moments record (best_obj and pen_best from k_sm_final_prior, the rest from k_sm_moments_final),
    // its pinned copy, one partial record per workgroup of k_sm_moments
    bl_scan_match_moments_t* d_mom = nullptr;
    bl_scan_match_moments_t* h_mom = nullptr;
    struct sm_partial* d_partial = nullptr;
    // the wide match (below)
    unsigned char* d_pool = nullptr; size_t pool_cap = 0;          // M_h, (W + B - 1) x (H + B - 1)
    unsigned char* d_pool_rows = nullptr; size_t pool_rows_cap = 0;
    int32_t* d_bounds = nullptr; size_t bounds_cap = 0;            // [heading][block row][block column]
    uint32_t* d_list = nullptr; size_t list_cap = 0;               // the kept blocks, in no particular order
    int2* d_seeds = nullptr; size_t seeds_cap = 0;                 // per heading: (best exact score of its seed block, its largest bound)
    struct smw_record* d_rec = nullptr;
    bool wide_ready = false, wide_matched = false;
    bl_scan_match_wide_stats_t wide_stats = bl_scan_match_wide_stats_t();
};

// ---------------------------------------------------------------------------------------------------------------- rasteriser
__global__ __launch_bounds__(256) void k_sm_raster(sm_head* __restrict__ head, const float* __restrict__ ranges,
                                                   const float* __restrict__ thetas, bl_frame f, int2* __restrict__ ends)
{
    sm_raster_body(head, ranges, thetas, f, ends, blockIdx.x);
}

// ---------------------------------------------------------------------------------------------------------------- scoring
// The map window, the prior's penalty and the scoring loop of both forms: bl_scanmatch_seq_dev.h.
// grid: (slices, headings).  Dynamic LDS: uint8 window[lds_window_bytes].
__global__ __launch_bounds__(1024) void k_sm_score(sm_head* __restrict__ head, const int8_t* __restrict__ cells, bl_frame f,
                                                    const int2* __restrict__ ends, int lds_window_bytes,
                                                    sm_block_best* __restrict__ best, int32_t* __restrict__ volume)
{
    sm_score_body<false>(head, cells, f, ends, lds_window_bytes, best, volume, sm_prior_k());
}
__global__ __launch_bounds__(1024) void k_sm_score_prior(sm_head* __restrict__ head, const int8_t* __restrict__ cells, bl_frame f,
                                                          const int2* __restrict__ ends, int lds_window_bytes,
                                                          sm_block_best* __restrict__ best, int32_t* __restrict__ volume, sm_prior_k pr)
{
    sm_score_body<true>(head, cells, f, ends, lds_window_bytes, best, volume, pr);
}

// ---------------------------------------------------------------------------------------------------------------- result
// sm_write_result and the final body of both forms: bl_scanmatch_seq_dev.h.
__global__ __launch_bounds__(256) void k_sm_final(sm_head* __restrict__ head, const sm_block_best* __restrict__ best, int nblocks,
                                                  bl_frame f)
{
    sm_final_body<false>(head, best, nblocks, f, sm_prior_k(), nullptr);
}
__global__ __launch_bounds__(256) void k_sm_final_prior(sm_head* __restrict__ head, const sm_block_best* __restrict__ best, int nblocks,
                                                        bl_frame f, sm_prior_k pr, bl_scan_match_moments_t* __restrict__ mom)
{
    sm_final_body<true>(head, best, nblocks, f, pr, mom);
}

// ---------------------------------------------------------------------------------------------------------------- moments
// The weight, the streaming pass and its reduction: bl_scanmatch_seq_dev.h.
__global__ __launch_bounds__(SM_MOM_THREADS) void k_sm_moments(const sm_head* __restrict__ head, const int32_t* __restrict__ volume,
                                                               const bl_scan_match_moments_t* __restrict__ mom, uint32_t magic,
                                                               int shift, sm_partial* __restrict__ partial)
{
    sm_moments_body(head, volume, mom, magic, shift, partial);
}

__global__ __launch_bounds__(256) void k_sm_moments_final(const sm_head* __restrict__ head, const int32_t* __restrict__ volume,
                                                          const sm_partial* __restrict__ partial, int nparts,
                                                          bl_scan_match_moments_t* __restrict__ mom)
{
    sm_moments_final_body(head, volume, partial, nparts, mom);
}

// ---------------------------------------------------------------------------------------------------------------- host
extern "C" int bl_scanmatch_create(bl_ctx* ctx, bl_scanmatch** out)
{
    BL_CHECK_ARG(ctx != nullptr && out != nullptr);
    BL_HIP(hipSetDevice(ctx->device));
    // per create: the attribute belongs to the current device, and contexts of several devices and threads make matchers
    BL_HIP(hipFuncSetAttribute((const void*)k_sm_score, hipFuncAttributeMaxDynamicSharedMemorySize, SM_LDS_MAX));
    BL_HIP(hipFuncSetAttribute((const void*)k_sm_score_prior, hipFuncAttributeMaxDynamicSharedMemorySize, SM_LDS_MAX));
    bl_scanmatch* sm = new bl_scanmatch();
    sm->ctx = ctx;
    hipError_t e = hipMalloc((void**)&sm->d_head, sizeof(smw_head));
    if (e != hipSuccess) { bl_set_error("hipMalloc failed: %s", hipGetErrorString(e)); delete sm; return BL_ERR_HIP; }
    *out = sm;
    return BL_OK;
}

extern "C" void bl_scanmatch_destroy(bl_scanmatch* sm)
{
    if (!sm) return;
    (void)hipStreamSynchronize(sm->ctx->stream);
    (void)hipFree(sm->d_head); (void)hipFree(sm->d_rays); (void)hipFree(sm->d_ends); (void)hipFree(sm->d_best); (void)hipFree(sm->d_volume);
    (void)hipFree(sm->d_mom); (void)hipFree(sm->d_partial);
    if (sm->h_mom) (void)hipHostFree(sm->h_mom);
    if (sm->staging) (void)hipHostFree(sm->staging);
    (void)hipFree(sm->d_pool); (void)hipFree(sm->d_pool_rows);
    (void)hipFree(sm->d_bounds); (void)hipFree(sm->d_list); (void)hipFree(sm->d_seeds); (void)hipFree(sm->d_rec);
    delete sm;
}

// What every match begins with, behind its checks.  The ray buffers (device ranges | thetas, and the pinned block: the larger header,
// then the same) and the endpoints for every heading of `rays` valid rays; then the pinned header zeroed and filled but for what is
// the wide match's alone, and the valid rays packed behind it.  *reach: the largest valid range.
static int sm_begin(bl_scanmatch* sm, const bl_lidar_t* scan, const bl_pose_xyt_t* centre, int nx, int ny, int ntheta, float dtheta,
                    float max_range, int min_score, int rays, float* reach)
{
    bl_ctx* ctx = sm->ctx;
    const size_t want = (size_t)(((rays > 0 ? rays : 1) + 255) & ~255) * 2 * sizeof(float);
    int rc = bl_grow((void**)&sm->d_rays, &sm->rays_bytes, want, false, ctx);
    if (rc) return rc;
    if ((rc = bl_grow(&sm->staging, &sm->staging_bytes, sizeof(smw_head) + sm->rays_bytes, true, ctx))) return rc;
    sm->ray_cap = (int)(sm->rays_bytes / (2 * sizeof(float)));
    const int rp = (rays + 63) & ~63;
    if ((rc = bl_grow((void**)&sm->d_ends, &sm->ends_cap, (size_t)(2 * ntheta + 1) * (rp > 0 ? rp : 64) * sizeof(int2), false, ctx))) return rc;

    smw_head* hd = (smw_head*)sm->staging;
    float* h_ranges = (float*)(hd + 1);
    memset(hd, 0, sizeof(smw_head));
    sm_head* h = &hd->base;
    h->cx = centre->x; h->cy = centre->y; h->ctheta = centre->theta; h->dtheta = dtheta;
    h->utime = scan->utime;
    h->nx = nx; h->ny = ny; h->ntheta = ntheta; h->rays = rays;
    h->min_score = min_score;
    h->bbox[0] = INT32_MAX; h->bbox[1] = INT32_MAX; h->bbox[2] = INT32_MIN; h->bbox[3] = INT32_MIN;
    (void)sm_valid_rays(scan, max_range, h_ranges, h_ranges + sm->ray_cap, reach);
    return BL_OK;
}

// head_bytes of the pinned header and the packed rays to the device, then the endpoints of every heading
static int sm_upload_and_raster(bl_scanmatch* sm, size_t head_bytes, int nk, int rays, const bl_frame& f)
{
    bl_ctx* ctx = sm->ctx;
    BL_HIP(hipMemcpyAsync(sm->d_head, sm->staging, head_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (rays > 0)
        BL_HIP(hipMemcpyAsync(sm->d_rays, (char*)sm->staging + sizeof(smw_head), sm->rays_bytes, hipMemcpyHostToDevice, ctx->stream));
    const long long total = (long long)nk * ((rays + 63) & ~63);
    if (total > 0)
        hipLaunchKernelGGL(k_sm_raster, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, &sm->d_head->base, sm->d_rays,
                           sm->d_rays + sm->ray_cap, f, sm->d_ends);
    return BL_OK;
}

// bl_scanmatch_match (prior == nullptr) and bl_scanmatch_match_prior.  A refused plain match forgets a kept volume, as it always
// has; a refused match with a prior changes nothing.
static int sm_match(bl_scanmatch* sm, const bl_grid* map, const bl_lidar_t* scan, const bl_pose_xyt_t* centre,
                    const bl_scan_match_params_t* params, const bl_scan_match_prior_t* prior, bl_scan_match_result_t* result,
                    bl_scan_match_moments_t* moments)
{
    BL_CHECK_ARG(sm != nullptr);
    if (!prior) sm->volume_kept = false;   // "the last match" includes a refused one: bl_scanmatch_volume then answers BL_ERR_STATE
    BL_CHECK_ARG(map != nullptr && scan != nullptr && centre != nullptr && params != nullptr && result != nullptr);
    BL_CHECK_ARG(map->ctx == sm->ctx);
    BL_CHECK_ARG(params->nx >= 0 && params->nx <= SM_MAX_N && params->ny >= 0 && params->ny <= SM_MAX_N);
    BL_CHECK_ARG(params->ntheta >= 0 && params->ntheta <= SM_MAX_NTHETA);
    BL_CHECK_ARG(params->dtheta > 0.0f);
    BL_CHECK_ARG(scan->num_ranges >= 0 && (scan->num_ranges == 0 || (scan->ranges != nullptr && scan->thetas != nullptr)));
    const int rays = sm_valid_rays(scan, params->max_range, nullptr, nullptr, nullptr);
    BL_CHECK_ARG(rays <= SM_MAX_RAYS);
    const bool want_moments = prior != nullptr && prior->want_moments != 0;
    if (prior) {
        BL_CHECK_ARG(sm_prior_ok(prior));
        BL_CHECK_ARG(!want_moments || (prior->half_life >= 1 && prior->half_life <= BL_SM_MAX_HALF_LIFE && moments != nullptr));
        sm->volume_kept = false;       // accepted: from here on this is the last match
    }
    const bool keep = params->keep_volume != 0 || want_moments;
    bl_ctx* ctx = sm->ctx;
    BL_HIP(hipSetDevice(ctx->device));

    // ---- buffers; the header and the valid rays
    const int nk = 2 * params->ntheta + 1, cw = 2 * params->nx + 1, ch = 2 * params->ny + 1, ncand = cw * ch;
    float rmax = 0;
    int rc = sm_begin(sm, scan, centre, params->nx, params->ny, params->ntheta, params->dtheta, params->max_range, params->min_score, rays,
                      &rmax);
    if (rc) return rc;
    // slices of a heading's candidates: enough workgroups to fill the device, none with less than a wave of candidates
    int threads = 0;
    const int slices = sm_score_slices(ncand, nk, 1024, &threads);
    const int nblocks = slices * nk;
    if ((rc = bl_grow((void**)&sm->d_best, &sm->best_cap, (size_t)nblocks * sizeof(sm_block_best), false, ctx))) return rc;
    if (keep && (rc = bl_grow((void**)&sm->d_volume, &sm->volume_cap, (size_t)nk * ncand * sizeof(int32_t), false, ctx))) return rc;
    // the moments pass: a wave per SM_MOM_BATCH rows of the volume, at most SM_MOM_MAX_GROUPS workgroups
    const int mom_groups = sm_moment_groups(nk * ch);
    if (prior && !sm->d_mom) {
        BL_HIP(hipMalloc((void**)&sm->d_mom, sizeof(bl_scan_match_moments_t)));
        BL_HIP(hipMalloc((void**)&sm->d_partial, SM_MOM_MAX_GROUPS * sizeof(sm_partial)));
        BL_HIP(hipHostMalloc((void**)&sm->h_mom, sizeof(bl_scan_match_moments_t), hipHostMallocDefault));
    }

    // ---- LDS for the window (sm_window_lds: an upper bound from the longest valid range)
    const bl_frame& f = map->frame;
    const int lds_window = sm_window_lds(rmax, f, params->nx, params->ny);
    const size_t lds_bytes = (size_t)(lds_window > 16 ? lds_window : 16);   // never empty: a masked-out lookup reads byte 0

    sm_head* d_head = &sm->d_head->base;
    sm_head* h = &((smw_head*)sm->staging)->base;
    if ((rc = sm_upload_and_raster(sm, sizeof(sm_head), nk, rays, f))) return rc;
    if (!prior) {
        hipLaunchKernelGGL(k_sm_score, dim3(slices, nk), dim3(threads), lds_bytes, ctx->stream, d_head, map->cells, f, sm->d_ends,
                           lds_window, sm->d_best, params->keep_volume ? sm->d_volume : (int32_t*)nullptr);
        hipLaunchKernelGGL(k_sm_final, dim3(1), dim3(256), 0, ctx->stream, d_head, sm->d_best, nblocks, f);
    } else {
        sm_prior_k pr; pr.a_xx = prior->a_xx; pr.a_xy = prior->a_xy; pr.a_yy = prior->a_yy; pr.a_tt = prior->a_tt;
        hipLaunchKernelGGL(k_sm_score_prior, dim3(slices, nk), dim3(threads), lds_bytes, ctx->stream, d_head, map->cells, f,
                           sm->d_ends, lds_window, sm->d_best, keep ? sm->d_volume : (int32_t*)nullptr, pr);
        hipLaunchKernelGGL(k_sm_final_prior, dim3(1), dim3(256), 0, ctx->stream, d_head, sm->d_best, nblocks, f, pr, sm->d_mom);
        if (want_moments) {
            // floor(64 d / half_life) as a multiplication (sm_weight): shift = 30 + L with 2^L >= half_life, magic = ceil(2^shift / half_life)
            int shift = 0;
            uint32_t magic = 0;
            sm_weight_magic(prior->half_life, &magic, &shift);
            hipLaunchKernelGGL(k_sm_moments, dim3(mom_groups), dim3(SM_MOM_THREADS), 0, ctx->stream, d_head, sm->d_volume, sm->d_mom,
                               magic, shift, sm->d_partial);
            hipLaunchKernelGGL(k_sm_moments_final, dim3(1), dim3(256), 0, ctx->stream, d_head, sm->d_volume, sm->d_partial,
                               mom_groups, sm->d_mom);
        }
    }
    BL_HIP(hipGetLastError());
    BL_HIP(hipMemcpyAsync(h, d_head, sizeof(sm_head), hipMemcpyDeviceToHost, ctx->stream));
    if (want_moments)
        BL_HIP(hipMemcpyAsync(sm->h_mom, sm->d_mom, sizeof(bl_scan_match_moments_t), hipMemcpyDeviceToHost, ctx->stream));
    BL_HIP(hipStreamSynchronize(ctx->stream));
    *result = h->result;
    if (want_moments) *moments = *sm->h_mom;
    sm->last_path = h->path;
    if (keep) { sm->volume_kept = true; sm->vol_nx = params->nx; sm->vol_ny = params->ny; sm->vol_nt = params->ntheta; }
    return BL_OK;
}

extern "C" int bl_scanmatch_match(bl_scanmatch* sm, const bl_grid* map, const bl_lidar_t* scan, const bl_pose_xyt_t* centre,
                                  const bl_scan_match_params_t* params, bl_scan_match_result_t* result)
{
    return sm_match(sm, map, scan, centre, params, nullptr, result, nullptr);
}

extern "C" int bl_scanmatch_match_prior(bl_scanmatch* sm, const bl_grid* map, const bl_lidar_t* scan, const bl_pose_xyt_t* centre,
                                        const bl_scan_match_params_t* params, const bl_scan_match_prior_t* prior,
                                        bl_scan_match_result_t* result, bl_scan_match_moments_t* moments)
{
    BL_CHECK_ARG(prior != nullptr);
    return sm_match(sm, map, scan, centre, params, prior, result, moments);
}

extern "C" int bl_scanmatch_volume(bl_scanmatch* sm, int32_t* scores)
{
    BL_CHECK_ARG(sm != nullptr && scores != nullptr);
    if (!sm->volume_kept) { bl_set_error("bl_scanmatch_volume: the last match did not keep its score volume"); return BL_ERR_STATE; }
    BL_HIP(hipSetDevice(sm->ctx->device));
    const size_t n = (size_t)(2 * sm->vol_nt + 1) * (2 * sm->vol_ny + 1) * (2 * sm->vol_nx + 1);
    BL_HIP(hipMemcpyAsync(scores, sm->d_volume, n * sizeof(int32_t), hipMemcpyDeviceToHost, sm->ctx->stream));
    BL_HIP(hipStreamSynchronize(sm->ctx->stream));
    return BL_OK;
}

extern "C" int bl_scanmatch_debug_path(const bl_scanmatch* sm)
{
    return sm ? sm->last_path : -1;
}

// ================================================================================================================ wide match
// bl_scanmatch_match_wide: the same definition over windows up to the whole map, exact, by one level of pruning (Olson's
// multi-resolution speed-up with a single pooled level).  DESIGN.md 4.12.
//
// Why the result is the exhaustive one.  P = the positive part of the map, 0 outside the grid.  B = 2^h.  The pooled map
// M[y][x] = max P[y .. y+B-1][x .. x+B-1], defined for x >= -(B-1), y >= -(B-1).  The block of shifts di in [i0, i0+B), dj in
// [j0, j0+B) at heading dk has bound = sum over the rays of M[ey + j0][ex + i0]; every term is at least its ray's term of any
// score of the block, so bound >= every score of the block (also of the shifts of an edge block that lie outside the window).  Let
// L be the exact score of ANY candidate of the window.  A candidate with score >= L lies in a block with bound >= score >= L.  The
// best score is >= L, so the best candidate and every candidate tying with it lie in blocks with bound >= L: scoring exactly the
// blocks with bound >= L (>=, not >) and reducing them with the total order of the definition gives the winner, its tie-break and
// `ties` of the exhaustive form.  Blocks partition the window, edge blocks are clipped to it: every candidate is counted once.
// If the largest bound is 0 every score is 0 and the answer is the centre with ties = the number of candidates, nothing scored.
//
// Stream-ordered on the ctx stream, no host round trip before the result:
//   k_sm_raster        as above (its on-grid test with the wide window).
//   k_smw_pool_rows / k_smw_pool_cols   M, separable sliding maximum, one byte per cell, rebuilt per match.
//   k_smw_bounds       a wave owns 64 consecutive blocks of a block row of one heading, lanes along the block index: endpoints
//                      wave-uniform and broadcast as in k_sm_score, reads of M at stride B; one int32 per (heading, block).
//   k_smw_seed         a workgroup per heading: its best-bounded block (ties to the lowest index) scored exactly; the centre
//                      heading's workgroup also scores (0, 0, 0).  L = the largest of these scores.
//   k_smw_compact      every workgroup recomputes L from the per-heading records (<= 1441 pairs), then appends the blocks with
//                      bound >= L to a list (one atomic add per wave claims the slots: the order of the list decides nothing).
//   k_smw_exact        256 persistent workgroups; a wave takes 64 candidates of a kept block at a time (an 8 x 8 block is one
//                      step), endpoints broadcast; the positive map from LDS when the whole grid fits (path 0), else the grid
//                      through L2 (path 1).  Per workgroup one (key, ties, scored) record; no atomic.  With exhaustive != 0 the
//                      list is every block and the pooling, bounds, seed and compaction launches are left out.
//   k_smw_final        one workgroup: maximum of the two-word keys, ties saturating at INT32_MAX, the result.
#define SMW_MAX_N 4096
#define SMW_MAX_NTHETA 720
#define SMW_MAX_BLOCKS (1ll << 26)     // budget: 256 MiB of bounds (int32 per block) and as much for the list of kept blocks
#define SMW_MAX_EXHAUSTIVE (1ll << 31) // candidates the exhaustive form accepts
#define SMW_GROUPS 256
#define SMW_THREADS 1024

// The candidate order in two words (compared hi first): score (< 2^20: 4096 rays x 127), small d2 = di*di + dj*dj (<= 2^25) |
// small |dk| (<= 720), small dk, small dj, small di.  hi of a real candidate is never 0.
struct smw_key { unsigned long long hi, lo; };
__device__ __forceinline__ smw_key smw_make_key(int score, int di, int dj, int dk)
{
    const uint32_t d2 = (uint32_t)(di * di + dj * dj);
    const uint32_t adk = (uint32_t)(dk < 0 ? -dk : dk);
    smw_key k;
    k.hi = ((unsigned long long)(uint32_t)score << 32) | (unsigned long long)(0x3ffffffu - d2);
    k.lo = ((unsigned long long)(1023u - adk) << 32) | ((unsigned long long)(dk <= 0 ? 1u : 0u) << 31) |
           ((unsigned long long)(uint32_t)(SMW_MAX_N - dj) << 14) | (unsigned long long)(uint32_t)(SMW_MAX_N - di);
    return k;
}
__device__ __forceinline__ bool smw_less(const smw_key& a, const smw_key& b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }
__device__ __forceinline__ smw_key smw_wave_max(smw_key v)
{
    for (int off = 32; off > 0; off >>= 1) {
        smw_key o; o.hi = __shfl_xor(v.hi, off, 64); o.lo = __shfl_xor(v.lo, off, 64);
        if (smw_less(v, o)) v = o;
    }
    return v;
}

struct smw_record { smw_key key; unsigned long long ties, scored; };

__global__ __launch_bounds__(256) void k_smw_pool_rows(const int8_t* __restrict__ cells, int W, int H, int B, int mw,
                                                       unsigned char* __restrict__ rows)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)H * mw) return;
    const int y = (int)(idx / mw), x0 = (int)(idx - (long long)y * mw) - (B - 1);
    int m = 0;
    for (int t = 0; t < B; ++t) {
        const int x = x0 + t;
        if (x >= 0 && x < W) m = max(m, (int)cells[(size_t)y * W + x]);
    }
    rows[idx] = (unsigned char)m;
}

__global__ __launch_bounds__(256) void k_smw_pool_cols(const unsigned char* __restrict__ rows, int H, int B, int mw, int mh,
                                                       unsigned char* __restrict__ pool)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)mh * mw) return;
    const int yp = (int)(idx / mw), xp = (int)(idx - (long long)yp * mw), y0 = yp - (B - 1);
    int m = 0;
    for (int t = 0; t < B; ++t) {
        const int y = y0 + t;
        if (y >= 0 && y < H) m = max(m, (int)rows[(size_t)y * mw + xp]);
    }
    pool[idx] = (unsigned char)m;
}

__global__ __launch_bounds__(256) void k_smw_bounds(const smw_head* __restrict__ head, const unsigned char* __restrict__ pool, int mw,
                                                    int mh, const int2* __restrict__ ends, int32_t* __restrict__ bounds)
{
    const int nk = 2 * head->base.ntheta + 1, h = head->hlog, B = 1 << h, nbx = head->nbx, nby = head->nby;
    const int rp = (head->base.rays + 63) & ~63;
    const int nchunk = (nbx + 63) >> 6, lane = threadIdx.x & 63;
    const long long gw = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gw >= (long long)nk * nby * nchunk) return;                          // whole waves leave
    const int k = (int)(gw / ((long long)nby * nchunk));
    const int rem = (int)(gw - (long long)k * nby * nchunk);
    const int bj = rem / nchunk, bi = (rem - bj * nchunk) * 64 + lane;
    const unsigned ox = (unsigned)(-head->base.nx + (bi << h) + B - 1), oy = (unsigned)(-head->base.ny + (bj << h) + B - 1);
    const int acc = sm_lookup_sum<false>(ends + (size_t)k * rp, rp, lane, ox, oy, pool, (unsigned)mw, (unsigned)mh, (unsigned)mw);
    if (bi < nbx) bounds[((size_t)k * nby + bj) * nbx + bi] = acc;
}

__global__ __launch_bounds__(256) void k_smw_seed(smw_head* __restrict__ head, const int8_t* __restrict__ cells, bl_frame f,
                                                  const int2* __restrict__ ends, const int32_t* __restrict__ bounds,
                                                  int2* __restrict__ seeds)
{
    __shared__ unsigned long long s_key[4];
    __shared__ int s_top[4];
    const int nt = head->base.ntheta, nx = head->base.nx, ny = head->base.ny, h = head->hlog, B = 1 << h, nbx = head->nbx;
    const int nb = nbx * head->nby, rp = (head->base.rays + 63) & ~63;
    const int k = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int32_t* __restrict__ kb = bounds + (size_t)k * nb;
    const int2* __restrict__ k_ends = ends + (size_t)k * rp;
    unsigned long long key = 0;
    for (int i = tid; i < nb; i += 256) {
        const unsigned long long c = ((unsigned long long)(uint32_t)kb[i] << 32) | (unsigned long long)(0xffffffffu - (uint32_t)i);
        key = c > key ? c : key;
    }
    key = sm_wave_max(key);
    if (lane == 0) s_key[wave] = key;
    __syncthreads();
    key = 0;
    for (int w = 0; w < 4; ++w) key = s_key[w] > key ? s_key[w] : key;
    const int bound = (int)(uint32_t)(key >> 32), idx = (int)(0xffffffffu - (uint32_t)key);
    const int bj = idx / nbx, bi = idx - bj * nbx;
    const int i0 = -nx + (bi << h), j0 = -ny + (bj << h);
    int top = 0;
    const bool any = bound > 0;                                              // a heading whose bounds are all 0 scores 0 everywhere: nothing to learn
    for (int cb = tid & ~63; any && cb < B * B; cb += 256) {                 // wave-uniform trip count
        const int c = cb + lane, di = i0 + (c & (B - 1)), dj = j0 + (c >> h);
        const int acc = sm_lookup_sum<true>(k_ends, rp, lane, (unsigned)di, (unsigned)dj, (const unsigned char*)cells, (unsigned)f.width,
                                      (unsigned)f.height, (unsigned)f.width);
        if (c < B * B && di <= nx && dj <= ny) top = max(top, acc);
    }
    for (int off = 32; off > 0; off >>= 1) top = max(top, __shfl_xor(top, off, 64));
    if (lane == 0) s_top[wave] = top;
    __syncthreads();
    if (k == nt && any) {                                                    // the centre's score, a ray per thread (0 when its heading's bounds are)
        int acc = 0;
        for (int r = tid; r < rp; r += 256) {
            const int2 e = k_ends[r];
            const bool in = (unsigned)e.x < (unsigned)f.width && (unsigned)e.y < (unsigned)f.height;
            const int v = cells[in ? (size_t)e.y * f.width + e.x : (size_t)0];
            acc += (in && v > 0) ? v : 0;
        }
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
        __syncthreads();
        if (lane == 0) s_key[wave] = (unsigned long long)(uint32_t)acc;
        __syncthreads();
        if (tid == 0) head->base.score_centre = (int)(s_key[0] + s_key[1] + s_key[2] + s_key[3]);
    }
    if (tid == 0) {
        seeds[k] = make_int2(max(max(s_top[0], s_top[1]), max(s_top[2], s_top[3])), bound);
        const long long n = (long long)(min(i0 + B - 1, nx) - i0 + 1) * (min(j0 + B - 1, ny) - j0 + 1) + (k == nt ? 1 : 0);
        if (any) atomicAdd(&head->scored, (unsigned long long)n);            // a count for the statistics; decides nothing
    }
}

// the threshold L and the largest bound, from the per-heading records; every lane of the workgroup returns the same pair
__device__ __forceinline__ int2 smw_threshold(const smw_head* __restrict__ head, const int2* __restrict__ seeds, int* s_a, int* s_b)
{
    const int nk = 2 * head->base.ntheta + 1, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    int L = 0, M = 0;
    for (int i = tid; i < nk; i += 256) { const int2 s = seeds[i]; L = max(L, s.x); M = max(M, s.y); }
    for (int off = 32; off > 0; off >>= 1) { L = max(L, __shfl_xor(L, off, 64)); M = max(M, __shfl_xor(M, off, 64)); }
    if (lane == 0) { s_a[wave] = L; s_b[wave] = M; }
    __syncthreads();
    L = max(max(max(s_a[0], s_a[1]), max(s_a[2], s_a[3])), head->base.score_centre);
    M = max(max(s_b[0], s_b[1]), max(s_b[2], s_b[3]));
    return make_int2(L, M);
}

__global__ __launch_bounds__(256) void k_smw_compact(smw_head* __restrict__ head, const int2* __restrict__ seeds,
                                                     const int32_t* __restrict__ bounds, long long nblocks, uint32_t* __restrict__ list)
{
    __shared__ int s_a[4], s_b[4];
    const int2 lm = smw_threshold(head, seeds, s_a, s_b);
    if (lm.y == 0) return;                                                   // every score is 0: nothing to score
    const int lane = threadIdx.x & 63;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool keep = idx < nblocks && bounds[idx] >= lm.x;
    const unsigned long long mask = __ballot(keep);
    if (mask == 0) return;
    unsigned int base = 0;
    if (lane == 0) base = atomicAdd(&head->kept, (unsigned int)__popcll(mask));
    base = __shfl(base, 0, 64);
    if (keep) list[base + (unsigned int)__popcll(mask & ((1ull << lane) - 1ull))] = (uint32_t)idx;
}

// grid: SMW_GROUPS workgroups of SMW_THREADS.  Dynamic LDS (STAGED): the positive part of the whole grid, rows at `pitch`.
template <bool STAGED>
__global__ __launch_bounds__(SMW_THREADS) void k_smw_exact(smw_head* __restrict__ head, const int8_t* __restrict__ cells, bl_frame f,
                                                           const int2* __restrict__ ends, const uint32_t* __restrict__ list,
                                                           long long nblocks, int pitch, smw_record* __restrict__ rec)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_map[];
    __shared__ smw_key s_key[SMW_THREADS / 64];
    __shared__ unsigned long long s_ties[SMW_THREADS / 64], s_scored[SMW_THREADS / 64];
    const int nt = head->base.ntheta, nx = head->base.nx, ny = head->base.ny, h = head->hlog, B = 1 << h, nbx = head->nbx;
    const int per = nbx * head->nby, rp = (head->base.rays + 63) & ~63;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int chunks = (B * B + 63) >> 6;
    const long long nwork = (list ? (long long)head->kept : nblocks) * chunks;
    if ((long long)blockIdx.x >= nwork) {                                    // wave 0 of workgroup b starts at work b: nothing here
        if (tid == 0) { smw_record r; r.key.hi = 0; r.key.lo = 0; r.ties = 0; r.scored = 0; rec[blockIdx.x] = r; }
        return;
    }
    if (STAGED) {                                                            // the window is the whole grid: its pitch is `pitch`
        sm_stage_window(cells, f.width, sm_clip_window(0, 0, f.width - 1, f.height - 1, true, f), s_map, tid, SMW_THREADS);
        __syncthreads();
    }
    smw_key key; key.hi = 0; key.lo = 0;
    int top = -1; unsigned long long ties = 0, scored = 0;
    const long long nwaves = (long long)gridDim.x * (SMW_THREADS / 64);
    for (long long w = (long long)wave * gridDim.x + blockIdx.x; w < nwork; w += nwaves) {        // wave-uniform
        const long long item = w / chunks;
        const int chunk = (int)(w - item * chunks);
        const long long b = list ? (long long)list[item] : item;
        const int k = (int)(b / per), rem = (int)(b - (long long)k * per);
        const int bj = rem / nbx, bi = rem - bj * nbx, dk = k - nt;
        const int c = chunk * 64 + lane;
        const int di = -nx + (bi << h) + (c & (B - 1)), dj = -ny + (bj << h) + (c >> h);
        const int acc = STAGED ? sm_lookup_sum<false>(ends + (size_t)k * rp, rp, lane, (unsigned)di, (unsigned)dj, s_map, (unsigned)f.width,
                                                (unsigned)f.height, (unsigned)pitch)
                               : sm_lookup_sum<true>(ends + (size_t)k * rp, rp, lane, (unsigned)di, (unsigned)dj, (const unsigned char*)cells,
                                               (unsigned)f.width, (unsigned)f.height, (unsigned)f.width);
        if (c >= B * B || di > nx || dj > ny) continue;                      // an edge block's shifts outside the window
        ++scored;
        if (!list && dk == 0 && di == 0 && dj == 0) head->base.score_centre = acc;
        const smw_key kc = smw_make_key(acc, di, dj, dk);
        if (smw_less(key, kc)) key = kc;
        if (acc > top) { top = acc; ties = 1; } else if (acc == top) ++ties;
    }
    const smw_key wkey = smw_wave_max(key);
    if (lane == 0) s_key[wave] = wkey;
    __syncthreads();
    smw_key bkey; bkey.hi = 0; bkey.lo = 0;
    for (int w = 0; w < SMW_THREADS / 64; ++w) if (smw_less(bkey, s_key[w])) bkey = s_key[w];
    unsigned long long n = (top >= 0 && (uint32_t)top == (uint32_t)(bkey.hi >> 32)) ? ties : 0;
    for (int off = 32; off > 0; off >>= 1) { n += __shfl_xor(n, off, 64); scored += __shfl_xor(scored, off, 64); }
    if (lane == 0) { s_ties[wave] = n; s_scored[wave] = scored; }
    __syncthreads();
    if (tid == 0) {
        smw_record r; r.key = bkey; r.ties = 0; r.scored = 0;
        for (int w = 0; w < SMW_THREADS / 64; ++w) { r.ties += s_ties[w]; r.scored += s_scored[w]; }
        rec[blockIdx.x] = r;
    }
}

__global__ __launch_bounds__(256) void k_smw_final(smw_head* __restrict__ head, const smw_record* __restrict__ rec, int nrec,
                                                   const int2* __restrict__ seeds, bl_frame f)
{
    __shared__ int s_a[4], s_b[4];
    __shared__ smw_key s_key[4];
    __shared__ unsigned long long s_ties[4], s_scored[4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    bool flat = false;                                                       // pruned, and no bound above 0
    if (seeds) flat = smw_threshold(head, seeds, s_a, s_b).y == 0;
    smw_key key; key.hi = 0; key.lo = 0;
    for (int i = tid; i < nrec; i += 256) { const smw_record r = rec[i]; if (r.ties && smw_less(key, r.key)) key = r.key; }
    key = smw_wave_max(key);
    if (lane == 0) s_key[wave] = key;
    __syncthreads();
    key.hi = 0; key.lo = 0;
    for (int w = 0; w < 4; ++w) if (smw_less(key, s_key[w])) key = s_key[w];
    unsigned long long n = 0, scored = 0;
    for (int i = tid; i < nrec; i += 256) {
        const smw_record r = rec[i];
        scored += r.scored;
        if (r.ties && (r.key.hi >> 32) == (key.hi >> 32)) n += r.ties;
    }
    for (int off = 32; off > 0; off >>= 1) { n += __shfl_xor(n, off, 64); scored += __shfl_xor(scored, off, 64); }
    if (lane == 0) { s_ties[wave] = n; s_scored[wave] = scored; }
    __syncthreads();
    if (tid == 0) {
        unsigned long long ties = s_ties[0] + s_ties[1] + s_ties[2] + s_ties[3];
        int score = (int)(uint32_t)(key.hi >> 32);
        int di = SMW_MAX_N - (int)(uint32_t)(key.lo & 0x3fffu), dj = SMW_MAX_N - (int)(uint32_t)((key.lo >> 14) & 0x3fffu);
        const int adk = 1023 - (int)(uint32_t)(key.lo >> 32);
        int dk = (key.lo & 0x80000000ull) ? -adk : adk;
        if (flat) { score = 0; di = 0; dj = 0; dk = 0; ties = (unsigned long long)head->candidates; }
        head->scored += s_scored[0] + s_scored[1] + s_scored[2] + s_scored[3];
        sm_write_result(&head->base, f, di, dj, dk, score, ties > (unsigned long long)INT32_MAX ? INT32_MAX : (int32_t)ties);
    }
}

static long long smw_blocks(const bl_scan_match_wide_params_t* p, int h, int* nbx, int* nby)
{
    const int B = 1 << h;
    *nbx = (2 * p->nx + 1 + B - 1) >> h; *nby = (2 * p->ny + 1 + B - 1) >> h;
    return (long long)(2 * p->ntheta + 1) * *nbx * *nby;
}

extern "C" int bl_scanmatch_match_wide(bl_scanmatch* sm, const bl_grid* map, const bl_lidar_t* scan, const bl_pose_xyt_t* centre,
                                       const bl_scan_match_wide_params_t* params, bl_scan_match_result_t* result)
{
    BL_CHECK_ARG(sm != nullptr && map != nullptr && scan != nullptr && centre != nullptr && params != nullptr && result != nullptr);
    BL_CHECK_ARG(map->ctx == sm->ctx);
    BL_CHECK_ARG(params->nx >= 0 && params->nx <= SMW_MAX_N && params->ny >= 0 && params->ny <= SMW_MAX_N);
    BL_CHECK_ARG(params->ntheta >= 0 && params->ntheta <= SMW_MAX_NTHETA);
    BL_CHECK_ARG(params->dtheta > 0.0f);
    BL_CHECK_ARG(params->block_log2 >= 0 && params->block_log2 <= 6);
    BL_CHECK_ARG(scan->num_ranges >= 0 && (scan->num_ranges == 0 || (scan->ranges != nullptr && scan->thetas != nullptr)));
    const int rays = sm_valid_rays(scan, params->max_range, nullptr, nullptr, nullptr);
    BL_CHECK_ARG(rays <= SM_MAX_RAYS);
    const int nk = 2 * params->ntheta + 1;
    const long long candidates = (long long)nk * (2 * params->nx + 1) * (2 * params->ny + 1);
    const bool exhaustive = params->exhaustive != 0;
    BL_CHECK_ARG(!exhaustive || candidates <= SMW_MAX_EXHAUSTIVE);
    // the block size: 8 x 8 unless asked otherwise, grown until the bounds fit the budget (64 x 64 always does)
    int h = params->block_log2 ? params->block_log2 : 3, nbx = 0, nby = 0;
    long long nblocks = smw_blocks(params, h, &nbx, &nby);
    if (!exhaustive) {
        while (params->block_log2 == 0 && nblocks > SMW_MAX_BLOCKS) nblocks = smw_blocks(params, ++h, &nbx, &nby);
        BL_CHECK_ARG(nblocks <= SMW_MAX_BLOCKS);
    }
    bl_ctx* ctx = sm->ctx;
    const bl_frame& f = map->frame;
    BL_CHECK_ARG(f.width > 0 && f.height > 0);
    BL_HIP(hipSetDevice(ctx->device));

    // ---- buffers
    const int B = 1 << h, mw = f.width + B - 1, mh = f.height + B - 1;
    const int pitch = (f.width + 3) & ~3;
    const bool staged = (long long)pitch * f.height <= (long long)SM_LDS_MAX;
    if (!sm->wide_ready) {
        BL_HIP(hipFuncSetAttribute((const void*)k_smw_exact<true>, hipFuncAttributeMaxDynamicSharedMemorySize, SM_LDS_MAX));
        BL_HIP(hipMalloc((void**)&sm->d_rec, SMW_GROUPS * sizeof(smw_record)));
        sm->wide_ready = true;
    }
    int rc = sm_begin(sm, scan, centre, params->nx, params->ny, params->ntheta, params->dtheta, params->max_range, params->min_score, rays,
                      nullptr);
    if (rc) return rc;
    if (!exhaustive) {
        if ((rc = bl_grow((void**)&sm->d_pool, &sm->pool_cap, (size_t)mw * mh, false, ctx))) return rc;
        if ((rc = bl_grow((void**)&sm->d_pool_rows, &sm->pool_rows_cap, (size_t)mw * f.height, false, ctx))) return rc;
        if ((rc = bl_grow((void**)&sm->d_bounds, &sm->bounds_cap, (size_t)nblocks * sizeof(int32_t), false, ctx))) return rc;
        if ((rc = bl_grow((void**)&sm->d_list, &sm->list_cap, (size_t)nblocks * sizeof(uint32_t), false, ctx))) return rc;
        if ((rc = bl_grow((void**)&sm->d_seeds, &sm->seeds_cap, (size_t)nk * sizeof(int2), false, ctx))) return rc;
    }
    smw_head* hd = (smw_head*)sm->staging;
    hd->hlog = h; hd->nbx = nbx; hd->nby = nby; hd->exhaustive = exhaustive ? 1 : 0;
    hd->candidates = candidates;
    if ((rc = sm_upload_and_raster(sm, sizeof(smw_head), nk, rays, f))) return rc;
    if (!exhaustive) {
        hipLaunchKernelGGL(k_smw_pool_rows, dim3((unsigned)(((long long)mw * f.height + 255) / 256)), dim3(256), 0, ctx->stream,
                           map->cells, f.width, f.height, B, mw, sm->d_pool_rows);
        hipLaunchKernelGGL(k_smw_pool_cols, dim3((unsigned)(((long long)mw * mh + 255) / 256)), dim3(256), 0, ctx->stream,
                           sm->d_pool_rows, f.height, B, mw, mh, sm->d_pool);
        const long long waves = (long long)nk * nby * ((nbx + 63) >> 6);
        hipLaunchKernelGGL(k_smw_bounds, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, ctx->stream, sm->d_head, sm->d_pool, mw, mh,
                           sm->d_ends, sm->d_bounds);
        hipLaunchKernelGGL(k_smw_seed, dim3(nk), dim3(256), 0, ctx->stream, sm->d_head, map->cells, f, sm->d_ends, sm->d_bounds,
                           sm->d_seeds);
        hipLaunchKernelGGL(k_smw_compact, dim3((unsigned)((nblocks + 255) / 256)), dim3(256), 0, ctx->stream, sm->d_head, sm->d_seeds,
                           sm->d_bounds, nblocks, sm->d_list);
    }
    const uint32_t* list = exhaustive ? (const uint32_t*)nullptr : sm->d_list;
    if (staged)
        hipLaunchKernelGGL(k_smw_exact<true>, dim3(SMW_GROUPS), dim3(SMW_THREADS), (size_t)pitch * f.height, ctx->stream, sm->d_head,
                           map->cells, f, sm->d_ends, list, nblocks, pitch, sm->d_rec);
    else
        hipLaunchKernelGGL(k_smw_exact<false>, dim3(SMW_GROUPS), dim3(SMW_THREADS), 0, ctx->stream, sm->d_head, map->cells, f,
                           sm->d_ends, list, nblocks, pitch, sm->d_rec);
    hipLaunchKernelGGL(k_smw_final, dim3(1), dim3(256), 0, ctx->stream, sm->d_head, sm->d_rec, SMW_GROUPS,
                       exhaustive ? (const int2*)nullptr : sm->d_seeds, f);
    BL_HIP(hipGetLastError());
    BL_HIP(hipMemcpyAsync(hd, sm->d_head, sizeof(smw_head), hipMemcpyDeviceToHost, ctx->stream));
    BL_HIP(hipStreamSynchronize(ctx->stream));
    *result = hd->base.result;
    sm->wide_stats.candidates = candidates;
    sm->wide_stats.blocks = nblocks;
    sm->wide_stats.blocks_kept = exhaustive ? nblocks : (long long)hd->kept;
    sm->wide_stats.candidates_scored = (long long)hd->scored;
    sm->wide_stats.block_log2 = h;
    sm->wide_stats.path = staged ? 0 : 1;
    sm->wide_matched = true;
    return BL_OK;
}

extern "C" int bl_scanmatch_wide_stats(const bl_scanmatch* sm, bl_scan_match_wide_stats_t* out)
{
    BL_CHECK_ARG(sm != nullptr && out != nullptr);
    if (!sm->wide_matched) { bl_set_error("bl_scanmatch_wide_stats: no wide match yet"); return BL_ERR_STATE; }
    *out = sm->wide_stats;
    return BL_OK;
}
