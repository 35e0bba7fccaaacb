// bl_rbslam_match.h -- step 3b of a moved bl_rbslam_update with scan matching on: every particle matches the scan against ITS OWN map in
// a small window around the pose the action left, and moves to the best pose there.  Included by bl_rbslam.hip (the object's struct is
// private to that file), after rb_weigh_args.  The definition is botlab_hip.h's "correlative scan matching" word for
// word, one match per particle; tests/rb_slam_match_model.py is the same over tests/scan_match_model.py.
//
// k_rb_match: ONE launch, a workgroup per particle, no atomics, no host round trip.
//   prologue   ActionModel::applyAction of the particle (k_rb_weigh's own, which is then launched in its form without it)
//   window     the map cells any candidate can reach: the centre cell +- (reach + n + 1), reach = ceil(longest valid range *
//              cellsPerMeter), clipped to the grid.  STAGED: its positive part sits in LDS as uint8 (the host decides from the bound
//              of the window, BL_RBSLAM_MATCH_WINDOW_BYTES); otherwise the particle's map is read directly through L2.
//   headings   one at a time: the valid rays' endpoint cells, window-relative, go to LDS; thread t then scores candidate t % ncand
//              (lanes consecutive along di) over ray slice t / ncand, the slices' partial sums meet in LDS, and thread c < ncand folds
//              candidate c of this heading into its running 64-bit key, top score and tie count.  Two barriers per heading.
//   result     one workgroup maximum of the keys (order-independent), the sum of the tie counts, the pose.
#ifndef BL_RBSLAM_MATCH_H
#define BL_RBSLAM_MATCH_H

#include "bl_scanmatch_dev.h"                // the rules this match has in common with bl_scanmatch.hip's, each stated there once

#define RBM_THREADS 512
#define RBM_MAX_RAYS BL_RBSLAM_MATCH_MAX_RAYS
#define RBM_MAX_SLICES 64
#define RBM_WINDOW_BYTES BL_RBSLAM_MATCH_WINDOW_BYTES
#define RBM_WHOLE (1 << 20)                  // a half window of this many cells or more: the window is the whole grid
#define RBM_NONE (-(1 << 30))                // x of an endpoint without a cell: no shift brings it into a window

struct rb_match_args {
    int rays;                                // valid rays (sm_valid_rays)
    const float* ranges; const float* thetas;
    int nx, ny, ntheta; float dtheta; int min_score;
    int hx, hy;                              // half window in cells: reach + n + 1, or RBM_WHOLE
    int ends_bytes;                          // dynamic LDS: int2 ends[rays] | uint8 window[]
    int32_t* out;                            // di | dj | dk | score | score_centre | ties | accepted, P entries each
};

template <bool STAGED>
__global__ __launch_bounds__(RBM_THREADS) void k_rb_match(rb_weigh_args a, rb_match_args q)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    __shared__ int s_part[RBM_THREADS];
    __shared__ unsigned long long s_key[RBM_THREADS / 64];
    __shared__ uint32_t s_ties[RBM_THREADS / 64];
    const int tid = threadIdx.x, m = blockIdx.x;
    int2* s_ends = (int2*)s_raw;
    unsigned char* s_win = s_raw + q.ends_bytes;
    const bl_frame& f = a.frame;

    // ---- step 3, the same in every thread
    const float4 s = a.src[a.idx[m]];
    float px, py, pth;
    bl_pf_apply_action(a, m, m, s, px, py, pth);

    // ---- the window of this particle
    float sx, sy;
    bl_global_to_grid(px, py, f, &sx, &sy);
    const bool near = __builtin_fabsf(sx) < 0x1p29f && __builtin_fabsf(sy) < 0x1p29f;      // false for NaN
    const int cx = near ? (int)sx : 0, cy = near ? (int)sy : 0;
    int bx0 = 0, by0 = 0, bx1 = f.width - 1, by1 = f.height - 1;
    bool any = true;
    if (q.hx < RBM_WHOLE) { any = near; bx0 = cx - q.hx; bx1 = cx + q.hx; }
    if (q.hy < RBM_WHOLE) { any = any && near; by0 = cy - q.hy; by1 = cy + q.hy; }
    const sm_window win = sm_clip_window(bx0, by0, bx1, by1, any, f);
    const int x0 = win.x0, y0 = win.y0, w = win.w, h = win.h, pitch = win.pitch;
    const int8_t* cells = a.maps + (size_t)a.slot[m] * a.stride;
    if (STAGED) sm_stage_window(cells, f.width, win, s_win, tid, RBM_THREADS);

    // ---- thread t: candidate t % ncand over the rays slice, slice + S, ...; thread c < ncand owns candidate c
    const int cw = 2 * q.nx + 1, ncand = cw * (2 * q.ny + 1);           // <= 289
    int S = RBM_THREADS / ncand;
    if (S > RBM_MAX_SLICES) S = RBM_MAX_SLICES;
    const int cand = tid % ncand, slice = tid / ncand;
    const int jrow = cand / cw, di = cand - jrow * cw - q.nx, dj = jrow - q.ny;
    const bool scorer = slice < S;
    unsigned long long key = 0;
    int top = -1, centre = 0; uint32_t ties = 0;
    for (int dk = -q.ntheta; dk <= q.ntheta; ++dk) {
        const float theta_k = pth + (float)dk * q.dtheta;
        for (int r = tid; r < q.rays; r += RBM_THREADS) {
            int2 e = make_int2(RBM_NONE, RBM_NONE);
            int ix, iy;
            if (sm_endpoint(q.ranges[r], q.thetas[r], theta_k, sx, sy, f, &ix, &iy)) e = make_int2(ix - x0, iy - y0);
            s_ends[r] = e;
        }
        __syncthreads();                                                // the endpoints (and, the first time, the window) are in LDS
        if (scorer) {
            int acc = 0;
            for (int r = slice; r < q.rays; r += S) {
                const int2 e = s_ends[r];
                const unsigned ux = (unsigned)(e.x + di), uy = (unsigned)(e.y + dj);
                const bool in = ux < (unsigned)w && uy < (unsigned)h;   // never true for RBM_NONE
                if (STAGED) {
                    const int v = s_win[in ? uy * (unsigned)pitch + ux : 0u];                  // no branch: the reads of a thread overlap
                    acc += in ? v : 0;
                } else {
                    const int v = cells[in ? (size_t)(y0 + (int)uy) * f.width + (size_t)(x0 + (int)ux) : (size_t)0];
                    acc += (in && v > 0) ? v : 0;
                }
            }
            s_part[tid] = acc;
        }
        __syncthreads();
        if (tid < ncand) {
            int acc = 0;
            for (int k = 0; k < S; ++k) acc += s_part[k * ncand + tid];
            if (dk == 0 && di == 0 && dj == 0) centre = acc;
            const unsigned long long kc = sm_key(acc, di, dj, dk);
            key = kc > key ? kc : key;
            if (acc > top) { top = acc; ties = 1; } else if (acc == top) ++ties;
        }
    }
    // ---- the particle's best key, and how many candidates share its score
    const sm_best wg = sm_block_best_key(key, (uint32_t)top, ties, RBM_THREADS / 64, s_key, s_ties);      // ties is 0 from ncand on
    if (tid == q.ny * cw + q.nx) q.out[4 * a.P + m] = centre;           // the thread that owns (0, 0)
    if (tid == 0) {
        int score, bi, bj, bk;
        sm_key_decode(wg.key, &score, &bi, &bj, &bk);
        const int accepted = score >= q.min_score ? 1 : 0;
        // a particle that stays where the action left it keeps that pose bit for bit (its heading is not wrapped again)
        sm_result_pose(accepted && (bi != 0 || bj != 0 || bk != 0), px, py, pth, bi, bj, bk, f.mpc, q.dtheta, &px, &py, &pth);
        a.dst[m] = make_float4(px, py, pth, 0.0f);
        a.parent[m] = make_float4(s.x, s.y, s.z, 0.0f);
        q.out[m] = bi; q.out[a.P + m] = bj; q.out[2 * a.P + m] = bk; q.out[3 * a.P + m] = score;
        q.out[5 * a.P + m] = (int32_t)wg.ties; q.out[6 * a.P + m] = accepted;
    }
}

#endif  // BL_RBSLAM_MATCH_H
