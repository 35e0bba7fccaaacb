// bl_loopclose.hip -- the loop-closure front end (include/botlab_hip.h, "loop closure"): from a scan log the loop
// edges, every candidate in one sequence of launches.  The definition is the header's; the numpy restatement the tests compare with,
// bit for bit, is tests/loop_closure_model.py.
//
// One stream-ordered sequence per find on the ctx stream, its length independent of the number of candidates; grids are sized by the
// slots = min(queries, max_candidates), and a slot without a candidate leaves at once:
//   k_lc_pairs          a wave per query: the nearest older scan by (d2, j), one 64 + 32 bit key, the lowest j of the minimum.
//                       find_places puts k_pr_describe and k_pr_match (bl_place_dev.h) in its place: the partner by
//                       the scans' descriptors, and k_lc_number then centres the match on the partner's pose turned by the shift.
//   k_lc_number         one workgroup: the queries with a partner numbered in ascending q; M and whether it fits.  When it does not,
//                       every later kernel leaves and the handle's results stay as they were.
//   k_lc_prep           a workgroup per candidate: the match header; the valid rays of entry q compacted in scan order.
//   k_lc_rays           a workgroup per (scan of the window, candidate): the rays' cells in the submap's frame and their box.
//   k_lc_fold           a workgroup per (64 x 64 tile, candidate): the window's scans folded in order into one clamped add per cell
//                       in LDS (bl_scanlog_dev.h), eval(f, 0) written as the submap's cells -- every cell of the submap, every call.
//   k_lc_raster, k_lc_score, k_lc_final, k_lc_moments, k_lc_moments_final
//                       bl_scanmatch_match_prior's sequence with a candidate dimension (bl_scanmatch_seq_dev.h).
//   k_lc_records        a thread per candidate: the gate and the record.
// One read-back (M, the candidates, the records) and one synchronisation; the edges of the kept candidates are formed on the host in
// plain double (this file is compiled with -ffp-contract=off like every other).
#include <string.h>

#include "bl_internal.h"
#include "bl_scanlog_dev.h"
#include "bl_scanmatch_seq_dev.h"
#include "bl_place_dev.h"

#define LC_MAX_BYTES (1ull << 30)
#define LC_PI 3.141592653589793
#define LC_TWO_PI 6.283185307179586

struct lc_cand {
    int32_t q, j, first, count;
    float ox, oy;                       // the submap's origin
    uint32_t flags; int32_t valid;      // BL_LC_TOO_MANY_RAYS or 0; the valid rays of entry q
    bl_pose_xyt_t pq, pj;               // the centre of the match (pose mode: the recorded pose of q) and the recorded pose of j
};
struct lc_state { int32_t M, ok; };

struct lc_args {
    int n, Q, slots, maxc;
    int stride, min_gap, w, S, W2;      // W2 = 2 w: the scans of a window that are traced
    double r2; float half;
    int head, capacity, max_rays, ray_stride;
    float mpc, cpm, max_laser; int hit, miss;
    int nx, ny, ntheta; float dtheta, max_range; int min_score;
    sm_prior_k pr; uint32_t magic; int shift;
    int nk, ncand, nblocks, mom_groups, rp_max, lds_window;
    char* scans; const int* kept; const bl_pose_xyt_t* ring;
    int* partner;                       // per query: j or -1
    const bl_place_t* place;            // place mode: per query the best pair; NULL in pose mode
    lc_state* state; lc_cand* cand;
    int4* rays; int4* boxes; int8_t* sub;
    float* vr;                          // per slot: ranges[SM_MAX_RAYS] | thetas[SM_MAX_RAYS]
    sm_head* heads; int2* ends; sm_block_best* best; int32_t* volume;
    bl_scan_match_moments_t* mom; sm_partial* partial;
    bl_loopclose_candidate_t* rec;
};

struct bl_loopclose {
    bl_ctx* ctx;
    int maxc;
    lc_state* d_state; lc_cand* d_cand; sm_head* d_heads; bl_scan_match_moments_t* d_mom; bl_loopclose_candidate_t* d_rec;
    void* d_partner; size_t cap_partner;
    void* d_desc; size_t cap_desc;      // place mode: the descriptors, their counts and the per-query records of the last
    void* d_bits; size_t cap_bits;      // find_places that launched
    void* d_place; size_t cap_place;
    int place_n, place_Q; bool placed;
    void* d_rays; size_t cap_rays;
    void* d_boxes; size_t cap_boxes;
    void* d_sub; size_t cap_sub;
    void* d_vr; size_t cap_vr;
    void* d_ends; size_t cap_ends;
    void* d_best; size_t cap_best;
    void* d_volume; size_t cap_volume;
    void* d_partial; size_t cap_partial;
    char* staging;                      // pinned: lc_state | lc_cand[maxc] | bl_loopclose_candidate_t[maxc]
    hipEvent_t ev[5];
    bool timed;
    // the last find that was not refused
    int M, S;
    std::vector<lc_cand>* cands;
    std::vector<bl_loopclose_candidate_t>* recs;
};

__device__ __forceinline__ bl_frame lc_frame(const lc_args& a, const lc_cand& c)
{
    bl_frame f; f.width = a.S; f.height = a.S; f.mpc = a.mpc; f.cpm = a.cpm; f.ox = c.ox; f.oy = c.oy;
    return f;
}
__device__ __forceinline__ bool lc_live(const lc_args& a, int m) { return a.state->ok != 0 && m < a.state->M; }

// ---------------------------------------------------------------- pairs
// grid: queries; a wave each.  d2 in double, every operation rounded by itself; its bits order as the values do (d2 >= +0).
__global__ __launch_bounds__(64) void k_lc_pairs(lc_args a)
{
    const int qi = blockIdx.x, q = qi * a.stride, lane = threadIdx.x;
    const int last = q - a.min_gap - 1;
    unsigned long long bk = ~0ull;
    int bj = INT32_MAX;
    double bd = 0.0;
    if (last >= 0) {
        const bl_pose_xyt_t pq = a.ring[(a.head + q) % a.capacity];
        for (int j = lane; j <= last; j += 64) {                 // ascending j: a lane keeps the lowest j of its minimum
            const bl_pose_xyt_t pj = a.ring[(a.head + j) % a.capacity];
            const double dx = (double)pj.x - (double)pq.x, dy = (double)pj.y - (double)pq.y;
            const double d2 = dx * dx + dy * dy;
            const unsigned long long key = (unsigned long long)__double_as_longlong(d2);
            if (key < bk) { bk = key; bj = j; bd = d2; }
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long ok = __shfl_xor(bk, off, 64);
        const int oj = __shfl_xor(bj, off, 64);
        const double od = __shfl_xor(bd, off, 64);
        if (ok < bk || (ok == bk && oj < bj)) { bk = ok; bj = oj; bd = od; }
    }
    if (lane == 0) a.partner[qi] = (bj != INT32_MAX && !(bd > a.r2)) ? bj : -1;
}

// one workgroup of 1024: M, then (when M fits) the candidates in ascending q
__global__ __launch_bounds__(1024) void k_lc_number(lc_args a)
{
    __shared__ int s_w[16];
    __shared__ int s_base, s_total;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) { s_base = 0; s_total = 0; }
    __syncthreads();
    int mine = 0;
    for (int t = tid; t < a.Q; t += 1024) mine += a.partner[t] >= 0 ? 1 : 0;
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off, 64);
    if (lane == 0 && mine) atomicAdd(&s_total, mine);
    __syncthreads();
    const int M = s_total;
    const bool ok = M <= a.maxc;
    if (tid == 0) { a.state->M = M; a.state->ok = ok ? 1 : 0; }
    if (!ok) return;                                            // uniform
    for (int t0 = 0; t0 < a.Q; t0 += 1024) {
        const int t = t0 + tid;
        const int j = t < a.Q ? a.partner[t] : -1;
        const int v = j >= 0 ? 1 : 0;
        int incl = v;
        for (int off = 1; off < 64; off <<= 1) { const int o = __shfl_up(incl, off, 64); if (lane >= off) incl += o; }
        if (lane == 63) s_w[wv] = incl;
        __syncthreads();
        int base = s_base;
        for (int k = 0; k < wv; ++k) base += s_w[k];
        if (v) {
            const int m = base + incl - 1;                      // < M <= maxc
            lc_cand c;
            c.q = t * a.stride; c.j = j;
            c.first = max(j - a.w, 0);
            c.count = min(j + a.w, a.n - 1) - c.first + 1;
            c.pq = a.ring[(a.head + c.q) % a.capacity];
            c.pj = a.ring[(a.head + j) % a.capacity];
            if (a.place) {                                      // the partner's pose turned by the shift; utime stays q's
                const int s = a.place[t].shift, ss = s < 32 ? s : s - 64;
                c.pq.x = c.pj.x; c.pq.y = c.pj.y;
                c.pq.theta = __fadd_rn(c.pj.theta, __fmul_rn((float)ss, PR_STEP));
            }
            c.ox = c.pj.x - a.half; c.oy = c.pj.y - a.half;
            c.flags = 0; c.valid = 0;
            a.cand[m] = c;
        }
        __syncthreads();
        if (tid == 1023) s_base = base + incl;
        __syncthreads();
    }
}

// ---------------------------------------------------------------- per candidate: the match header and the valid rays
// grid: slots.  The rays that count (sm_ray_valid), in scan order, packed as bl_scanmatch_match packs them on the host.
__global__ __launch_bounds__(256) void k_lc_prep(lc_args a)
{
    __shared__ int s_wc[4];
    const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (!lc_live(a, m)) return;
    const lc_cand c = a.cand[m];
    const int slot = (a.head + c.q) % a.capacity;
    const int kept = min(a.kept[slot], a.max_rays);
    const rl_slot s = rl_slot_of(a.scans, a.max_rays, slot);
    float* ranges = a.vr + (size_t)m * 2 * SM_MAX_RAYS;
    float* thetas = ranges + SM_MAX_RAYS;
    int base = 0;
    for (int r0 = 0; r0 < kept; r0 += 256) {
        const int r = r0 + tid;
        const float rng = r < kept ? s.ranges[r] : 0.0f;
        const bool valid = r < kept && sm_ray_valid(rng, a.max_range);
        const unsigned long long b = __ballot(valid);
        if (lane == 0) s_wc[wv] = __popcll(b);
        __syncthreads();
        int at = base + __popcll(b & ((1ull << lane) - 1ull));
        for (int k = 0; k < wv; ++k) at += s_wc[k];
        if (valid && at < SM_MAX_RAYS) { ranges[at] = rng; thetas[at] = s.thetas[r]; }
        base += s_wc[0] + s_wc[1] + s_wc[2] + s_wc[3];
        __syncthreads();
    }
    if (tid == 0) {
        const bool too_many = base > SM_MAX_RAYS;
        a.cand[m].valid = base;
        a.cand[m].flags = too_many ? (uint32_t)BL_LC_TOO_MANY_RAYS : 0u;
        sm_head h;
        memset(&h, 0, sizeof(h));
        h.cx = c.pq.x; h.cy = c.pq.y; h.ctheta = c.pq.theta; h.dtheta = a.dtheta;
        h.utime = c.pq.utime;
        h.nx = a.nx; h.ny = a.ny; h.ntheta = a.ntheta; h.rays = too_many ? 0 : base;
        h.min_score = a.min_score;
        h.bbox[0] = INT32_MAX; h.bbox[1] = INT32_MAX; h.bbox[2] = INT32_MIN; h.bbox[3] = INT32_MIN;
        a.heads[m] = h;
    }
}

// ---------------------------------------------------------------- the submaps
// grid: (traced scans of a window, slots).  Scan i of candidate m is entry first + 1 + i, traced from its predecessor's pose.
__global__ __launch_bounds__(RL_THREADS) void k_lc_rays(lc_args a)
{
    __shared__ int s_box[4];
    const int i = blockIdx.x, m = blockIdx.y;
    if (!lc_live(a, m)) return;
    const lc_cand c = a.cand[m];
    if (i >= c.count - 1) return;
    const int e = c.first + 1 + i;                              // 1 .. n - 1
    const int slot = (a.head + e) % a.capacity;
    const size_t at = (size_t)m * a.W2 + i;
    rl_scan_rays(lc_frame(a, c), a.max_laser, rl_slot_of(a.scans, a.max_rays, slot), min(a.kept[slot], a.ray_stride),
                 a.ring[(a.head + e - 1) % a.capacity], a.ring[slot], a.rays + at * a.ray_stride, &a.boxes[at], s_box);
}

// grid: (tiles of a submap, slots).  k_rl_fold's LDS layout, the whole window in one workgroup (at most 62 scans), the cells written
// directly: eval(f, 0).  A tile no ray meets keeps the identity and reads zero.
__global__ __launch_bounds__(RL_THREADS) void k_lc_fold(lc_args a)
{
    __shared__ unsigned int s_fn[RL_TILE_CELLS];
    __shared__ unsigned int s_cnt[RL_TILE_CELLS];
    const int tid = threadIdx.x, t = blockIdx.x, m = blockIdx.y;
    if (!lc_live(a, m)) return;
    const lc_cand c = a.cand[m];
    const int ntx = (a.S + RL_TILE - 1) / RL_TILE;
    const int ty = t / ntx, tx = t - ty * ntx;
    const int tx0 = tx * RL_TILE, ty0 = ty * RL_TILE;
    const int tx1 = min(tx0 + RL_TILE, a.S) - 1, ty1 = min(ty0 + RL_TILE, a.S) - 1;
    for (int i = tid; i < RL_TILE_CELLS; i += RL_THREADS) { s_fn[i] = RL_IDENTITY; s_cnt[i] = 0u; }
    __syncthreads();
    for (int i = 0; i < c.count - 1; ++i) {
        const size_t at = (size_t)m * a.W2 + i;
        if (!rl_meets(a.boxes[at], tx0, ty0, tx1, ty1)) continue;              // uniform over the workgroup
        const int slot = (a.head + c.first + 1 + i) % a.capacity;
        rl_fold_scan(s_fn, s_cnt, a.rays + at * a.ray_stride, min(a.kept[slot], a.ray_stride), tx0, ty0, tx1, ty1, a.hit, a.miss);
    }
    int8_t* sub = a.sub + (size_t)m * a.S * a.S;
    for (int j = tid; j < RL_TILE_CELLS; j += RL_THREADS) {
        const int x = tx0 + (j & (RL_TILE - 1)), y = ty0 + j / RL_TILE;
        if (x < a.S && y < a.S) sub[(size_t)y * a.S + x] = (int8_t)rl_eval(s_fn[j], 0);
    }
}

// ---------------------------------------------------------------- the matches: bl_scanmatch_match_prior's sequence per candidate
__device__ __forceinline__ const float* lc_ranges(const lc_args& a, int m) { return a.vr + (size_t)m * 2 * SM_MAX_RAYS; }
__device__ __forceinline__ int2* lc_ends(const lc_args& a, int m) { return a.ends + (size_t)m * a.nk * a.rp_max; }
__device__ __forceinline__ int32_t* lc_volume(const lc_args& a, int m) { return a.volume + (size_t)m * a.nk * a.ncand; }

// grid: (blocks over headings x the longest padded row, slots)
__global__ __launch_bounds__(256) void k_lc_raster(lc_args a)
{
    const int m = blockIdx.y;
    if (!lc_live(a, m)) return;
    if (a.heads[m].rays == 0) return;                           // as the single match: no launch without rays
    sm_raster_body(a.heads + m, lc_ranges(a, m), lc_ranges(a, m) + SM_MAX_RAYS, lc_frame(a, a.cand[m]), lc_ends(a, m), blockIdx.x);
}

// grid: (slices, headings, slots).  Dynamic LDS: the window.
__global__ __launch_bounds__(1024) void k_lc_score(lc_args a)
{
    const int m = blockIdx.z;
    if (!lc_live(a, m)) return;
    sm_score_body<true>(a.heads + m, a.sub + (size_t)m * a.S * a.S, lc_frame(a, a.cand[m]), lc_ends(a, m), a.lds_window,
                        a.best + (size_t)m * a.nblocks, lc_volume(a, m), a.pr);
}

// grid: slots
__global__ __launch_bounds__(256) void k_lc_final(lc_args a)
{
    const int m = blockIdx.x;
    if (!lc_live(a, m)) return;
    sm_final_body<true>(a.heads + m, a.best + (size_t)m * a.nblocks, a.nblocks, lc_frame(a, a.cand[m]), a.pr, a.mom + m);
}

// grid: (groups of the moments pass, slots)
__global__ __launch_bounds__(SM_MOM_THREADS) void k_lc_moments(lc_args a)
{
    const int m = blockIdx.y;
    if (!lc_live(a, m)) return;
    sm_moments_body(a.heads + m, lc_volume(a, m), a.mom + m, a.magic, a.shift, a.partial + (size_t)m * a.mom_groups);
}

// grid: slots
__global__ __launch_bounds__(256) void k_lc_moments_final(lc_args a)
{
    const int m = blockIdx.x;
    if (!lc_live(a, m)) return;
    sm_moments_final_body(a.heads + m, lc_volume(a, m), a.partial + (size_t)m * a.mom_groups, a.mom_groups, a.mom + m);
}

// a thread per slot: the gate and the record (the edge is the host's)
__global__ __launch_bounds__(256) void k_lc_records(lc_args a)
{
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= a.slots || !lc_live(a, m)) return;
    const lc_cand c = a.cand[m];
    bl_loopclose_candidate_t r;
    memset(&r, 0, sizeof(r));
    r.q = c.q; r.j = c.j; r.first = c.first; r.count = c.count;
    if (c.flags & BL_LC_TOO_MANY_RAYS) {
        r.flags = BL_LC_TOO_MANY_RAYS;
    } else {
        r.result = a.heads[m].result;
        r.moments = a.mom[m];
        uint32_t fl = 0;
        if (!r.result.accepted) fl |= BL_LC_NOT_ACCEPTED;
        if (r.result.ties != 1) fl |= BL_LC_TIED;
        if (!(abs(r.result.di) < a.nx && abs(r.result.dj) < a.ny && abs(r.result.dk) < a.ntheta)) fl |= BL_LC_ON_EDGE;
        r.flags = fl;
    }
    a.rec[m] = r;
}

// ---------------------------------------------------------------- the edge of a kept candidate, plain double, no fused operation
static double lc_wrap(double d)
{
    if (d > LC_PI) d = d - LC_TWO_PI;
    else if (d < -LC_PI) d = d + LC_TWO_PI;
    return d;
}
static void lc_mul3(const double a[3][3], const double b[3][3], double out[3][3])
{
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) out[r][c] = (a[r][0] * b[0][c] + a[r][1] * b[1][c]) + a[r][2] * b[2][c];
}
static void lc_edge(bl_loopclose_candidate_t* r, const lc_cand& cd, double mpc, double dtheta)
{
    bl_pose_xyt_t p;
    double mean[3], cov[6];
    bl_scanmatch_refined_pose(&r->result, &r->moments, &cd.pq, mpc, dtheta, &p);
    bl_scanmatch_covariance(&r->moments, mpc, dtheta, mean, cov);
    float sf, cf;
    bl_sincosf(cd.pj.theta, &sf, &cf);
    const double s = (double)sf, c = (double)cf;
    const double dx = (double)p.x - (double)cd.pj.x, dy = (double)p.y - (double)cd.pj.y;
    bl_posegraph_edge_t e;
    memset(&e, 0, sizeof(e));
    e.i = cd.j; e.j = cd.q;
    e.z[0] = c * dx + s * dy;
    e.z[1] = c * dy - s * dx;
    e.z[2] = lc_wrap((double)p.theta - (double)cd.pj.theta);
    const double Sg[3][3] = {{cov[0], cov[1], cov[3]}, {cov[1], cov[2], cov[4]}, {cov[3], cov[4], cov[5]}};
    const double Rt[3][3] = {{c, s, 0.0}, {-s, c, 0.0}, {0.0, 0.0, 1.0}};
    const double R[3][3] = {{c, -s, 0.0}, {s, c, 0.0}, {0.0, 0.0, 1.0}};
    double A[3][3], S[3][3];
    lc_mul3(Rt, Sg, A);
    lc_mul3(A, R, S);
    S[0][0] = S[0][0] + mpc * mpc / 12.0;
    S[1][1] = S[1][1] + mpc * mpc / 12.0;
    S[2][2] = S[2][2] + dtheta * dtheta / 12.0;
    double C[3][3];
    C[0][0] = S[1][1] * S[2][2] - S[1][2] * S[2][1];
    C[0][1] = S[1][2] * S[2][0] - S[1][0] * S[2][2];
    C[0][2] = S[1][0] * S[2][1] - S[1][1] * S[2][0];
    C[1][0] = S[0][2] * S[2][1] - S[0][1] * S[2][2];
    C[1][1] = S[0][0] * S[2][2] - S[0][2] * S[2][0];
    C[1][2] = S[0][1] * S[2][0] - S[0][0] * S[2][1];
    C[2][0] = S[0][1] * S[1][2] - S[0][2] * S[1][1];
    C[2][1] = S[0][2] * S[1][0] - S[0][0] * S[1][2];
    C[2][2] = S[0][0] * S[1][1] - S[0][1] * S[1][0];
    const double det = (S[0][0] * C[0][0] + S[0][1] * C[0][1]) + S[0][2] * C[0][2];
    double I[3][3];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) I[a][b] = C[b][a] / det;
    e.info[0] = 0.5 * (I[0][0] + I[0][0]); e.info[1] = 0.5 * (I[0][1] + I[1][0]); e.info[2] = 0.5 * (I[1][1] + I[1][1]);
    e.info[3] = 0.5 * (I[0][2] + I[2][0]); e.info[4] = 0.5 * (I[1][2] + I[2][1]); e.info[5] = 0.5 * (I[2][2] + I[2][2]);
    r->edge = e;
}

// ---------------------------------------------------------------- host
extern "C" int bl_loopclose_create(bl_ctx* ctx, int max_candidates, bl_loopclose** out)
{
    BL_CHECK_ARG(ctx != nullptr && out != nullptr);
    BL_CHECK_ARG(max_candidates >= 1 && max_candidates <= BL_LC_MAX_CANDIDATES);
    BL_HIP(hipSetDevice(ctx->device));
    BL_HIP(hipFuncSetAttribute((const void*)k_lc_score, hipFuncAttributeMaxDynamicSharedMemorySize, SM_LDS_MAX));
    bl_loopclose* lc = new bl_loopclose();
    memset(lc, 0, sizeof(*lc));
    lc->ctx = ctx; lc->maxc = max_candidates;
    lc->cands = new std::vector<lc_cand>();
    lc->recs = new std::vector<bl_loopclose_candidate_t>();
    const size_t n = (size_t)max_candidates;
    hipError_t e = hipMalloc((void**)&lc->d_state, sizeof(lc_state));
    if (e == hipSuccess) e = hipMalloc((void**)&lc->d_cand, n * sizeof(lc_cand));
    if (e == hipSuccess) e = hipMalloc((void**)&lc->d_heads, n * sizeof(sm_head));
    if (e == hipSuccess) e = hipMalloc((void**)&lc->d_mom, n * sizeof(bl_scan_match_moments_t));
    if (e == hipSuccess) e = hipMalloc((void**)&lc->d_rec, n * sizeof(bl_loopclose_candidate_t));
    if (e == hipSuccess) e = hipHostMalloc((void**)&lc->staging, sizeof(lc_state) + n * (sizeof(lc_cand) + sizeof(bl_loopclose_candidate_t)), hipHostMallocDefault);
    for (int i = 0; i < 5 && e == hipSuccess; ++i) e = hipEventCreate(&lc->ev[i]);
    if (e != hipSuccess) { bl_set_error("bl_loopclose_create: %s", hipGetErrorString(e)); bl_loopclose_destroy(lc); return BL_ERR_HIP; }
    *out = lc;
    return BL_OK;
}

extern "C" void bl_loopclose_destroy(bl_loopclose* lc)
{
    if (!lc) return;
    (void)hipStreamSynchronize(lc->ctx->stream);
    void* bufs[] = {lc->d_state, lc->d_cand, lc->d_heads, lc->d_mom, lc->d_rec, lc->d_partner, lc->d_rays, lc->d_boxes, lc->d_sub,
                    lc->d_vr, lc->d_ends, lc->d_best, lc->d_volume, lc->d_partial, lc->d_desc, lc->d_bits, lc->d_place};
    for (void* b : bufs) if (b) (void)hipFree(b);
    if (lc->staging) (void)hipHostFree(lc->staging);
    for (int i = 0; i < 5; ++i) if (lc->ev[i]) (void)hipEventDestroy(lc->ev[i]);
    delete lc->cands; delete lc->recs;
    delete lc;
}

// the submaps' buffer grown with its contents kept: a find that is refused for its count of partners leaves the last submaps readable
static int lc_grow_keep(void** p, size_t* cap, size_t want, bl_ctx* ctx)
{
    if (want <= *cap) return BL_OK;
    void* q = nullptr;
    BL_HIP(hipMalloc(&q, want));
    if (*p) {
        BL_HIP(hipMemcpyAsync(q, *p, *cap, hipMemcpyDeviceToDevice, ctx->stream));
        BL_HIP(hipStreamSynchronize(ctx->stream));
        BL_HIP(hipFree(*p));
    }
    *p = q; *cap = want;
    return BL_OK;
}

// find (place == NULL: partners by the recorded poses) and find_places (partners by the descriptors)
static int lc_find(bl_loopclose* lc, bl_scanlog* log, const bl_grid* like, const bl_loopclose_params_t* prm, const bl_place_params_t* place,
                   int* n_candidates)
{
    BL_CHECK_ARG(log->ctx == lc->ctx);
    BL_CHECK_ARG(prm->stride >= 1 && prm->min_gap >= 0);
    if (!place) BL_CHECK_ARG(prm->radius > 0.0f);                // false for NaN
    if (place) {
        BL_CHECK_ARG(place->bins_per_meter > 0.0f && place->bins_per_meter <= 1000.0f);       // false for NaN
        BL_CHECK_ARG(place->max_range > SM_MIN_RANGE && place->max_range <= 1000.0f);
        BL_CHECK_ARG(place->dilate == 0 || place->dilate == 1);
        BL_CHECK_ARG(place->min_key >= 0 && place->min_key <= 65536);
        BL_CHECK_ARG(place->min_bits >= 0 && place->min_bits <= PR_SECTORS * PR_BINS);
    }
    BL_CHECK_ARG(prm->w >= 0 && prm->w <= BL_LC_MAX_W);
    BL_CHECK_ARG(prm->submap_cells >= BL_LC_MIN_SUBMAP && prm->submap_cells <= BL_LC_MAX_SUBMAP);
    BL_CHECK_ARG(prm->hit >= 0 && prm->hit <= 127 && prm->miss >= 0 && prm->miss <= 127);
    const bl_scan_match_params_t& mp = prm->match;
    BL_CHECK_ARG(mp.nx >= 0 && mp.nx <= SM_MAX_N && mp.ny >= 0 && mp.ny <= SM_MAX_N);
    BL_CHECK_ARG(mp.ntheta >= 0 && mp.ntheta <= SM_MAX_NTHETA);
    BL_CHECK_ARG(mp.dtheta > 0.0f);
    BL_CHECK_ARG(mp.keep_volume == 0);
    BL_CHECK_ARG(sm_prior_ok(&prm->prior));
    BL_CHECK_ARG(prm->prior.half_life >= 1 && prm->prior.half_life <= BL_SM_MAX_HALF_LIFE);
    bl_ctx* ctx = lc->ctx;
    BL_HIP(hipSetDevice(ctx->device));

    const int n = log->size;
    if (n < 2) {
        lc->M = 0; lc->S = prm->submap_cells; lc->cands->clear(); lc->recs->clear();
        *n_candidates = 0;
        return BL_OK;
    }
    lc_args a;
    memset(&a, 0, sizeof(a));
    a.n = n; a.stride = prm->stride; a.min_gap = prm->min_gap; a.w = prm->w; a.S = prm->submap_cells; a.W2 = 2 * prm->w;
    a.Q = (int)(((long long)n + prm->stride - 1) / prm->stride);
    a.maxc = lc->maxc;
    a.slots = a.Q < lc->maxc ? a.Q : lc->maxc;
    a.r2 = (double)prm->radius * (double)prm->radius;
    a.mpc = like->frame.mpc; a.cpm = like->frame.cpm;
    a.half = (float)((double)a.S * (double)a.mpc / 2.0);
    a.head = log->head; a.capacity = log->capacity; a.max_rays = log->max_rays;
    int ray_stride = 1;
    for (int i = 0; i < n; ++i) { const int k = log->h_kept[(log->head + i) % log->capacity]; if (k > ray_stride) ray_stride = k; }
    a.ray_stride = ray_stride;
    a.max_laser = prm->max_laser; a.hit = prm->hit; a.miss = prm->miss;
    a.nx = mp.nx; a.ny = mp.ny; a.ntheta = mp.ntheta; a.dtheta = mp.dtheta; a.max_range = mp.max_range; a.min_score = mp.min_score;
    a.pr.a_xx = prm->prior.a_xx; a.pr.a_xy = prm->prior.a_xy; a.pr.a_yy = prm->prior.a_yy; a.pr.a_tt = prm->prior.a_tt;
    sm_weight_magic(prm->prior.half_life, &a.magic, &a.shift);
    a.nk = 2 * mp.ntheta + 1;
    const int ch = 2 * mp.ny + 1;
    a.ncand = (2 * mp.nx + 1) * ch;
    // the slots share the device: as many slices of a heading's candidates as give about 1024 workgroups in all
    int threads = 0;
    const int slices = sm_score_slices(a.ncand, a.nk, (1024 + a.slots - 1) / a.slots, &threads);
    a.nblocks = slices * a.nk;
    a.mom_groups = sm_moment_groups(a.nk * ch);
    a.rp_max = ((ray_stride < SM_MAX_RAYS ? ray_stride : SM_MAX_RAYS) + 63) & ~63;
    // LDS for a window: the bound of the longest range the matcher lets through; a bound that does not fit still lets every
    // candidate whose own window does be staged (the device compares what it needs with what it is given)
    bl_frame f; f.width = a.S; f.height = a.S; f.mpc = a.mpc; f.cpm = a.cpm; f.ox = 0.0f; f.oy = 0.0f;
    a.lds_window = sm_window_lds(mp.max_range, f, mp.nx, mp.ny);
    if (a.lds_window == 0) a.lds_window = SM_LDS_MAX;
    const size_t lds_bytes = (size_t)(a.lds_window > 16 ? a.lds_window : 16);

    const unsigned long long slots = (unsigned long long)a.slots, cells = (unsigned long long)a.S * a.S;
    const unsigned long long b_sub = slots * cells, b_vol = slots * a.nk * a.ncand * sizeof(int32_t);
    const unsigned long long b_rays = slots * a.W2 * ray_stride * sizeof(int4), b_ends = slots * a.nk * a.rp_max * sizeof(int2);
    BL_CHECK_ARG(b_sub + b_vol + b_rays + b_ends <= LC_MAX_BYTES);

    int rc = bl_grow(&lc->d_partner, &lc->cap_partner, (size_t)a.Q * sizeof(int), false, ctx);
    if (!rc && place) rc = bl_grow(&lc->d_desc, &lc->cap_desc, (size_t)n * PR_SECTORS * sizeof(uint32_t), false, ctx);
    if (!rc && place) rc = bl_grow(&lc->d_bits, &lc->cap_bits, (size_t)n * sizeof(int32_t), false, ctx);
    if (!rc && place) rc = bl_grow(&lc->d_place, &lc->cap_place, (size_t)a.Q * sizeof(bl_place_t), false, ctx);
    if (!rc) rc = bl_grow(&lc->d_rays, &lc->cap_rays, (size_t)b_rays, false, ctx);
    if (!rc) rc = bl_grow(&lc->d_boxes, &lc->cap_boxes, (size_t)(slots * (a.W2 > 0 ? a.W2 : 1)) * sizeof(int4), false, ctx);
    if (!rc) rc = lc_grow_keep(&lc->d_sub, &lc->cap_sub, (size_t)b_sub, ctx);
    if (!rc) rc = bl_grow(&lc->d_vr, &lc->cap_vr, (size_t)slots * 2 * SM_MAX_RAYS * sizeof(float), false, ctx);
    if (!rc) rc = bl_grow(&lc->d_ends, &lc->cap_ends, (size_t)b_ends, false, ctx);
    if (!rc) rc = bl_grow(&lc->d_best, &lc->cap_best, (size_t)slots * a.nblocks * sizeof(sm_block_best), false, ctx);
    if (!rc) rc = bl_grow(&lc->d_volume, &lc->cap_volume, (size_t)b_vol, false, ctx);
    if (!rc) rc = bl_grow(&lc->d_partial, &lc->cap_partial, (size_t)slots * a.mom_groups * sizeof(sm_partial), false, ctx);
    if (rc) return rc;
    a.scans = log->d_scans; a.kept = log->d_kept; a.ring = log->d_poses;
    a.partner = (int*)lc->d_partner; a.state = lc->d_state; a.cand = lc->d_cand;
    a.rays = (int4*)lc->d_rays; a.boxes = (int4*)lc->d_boxes; a.sub = (int8_t*)lc->d_sub; a.vr = (float*)lc->d_vr;
    a.heads = lc->d_heads; a.ends = (int2*)lc->d_ends; a.best = (sm_block_best*)lc->d_best; a.volume = (int32_t*)lc->d_volume;
    a.mom = lc->d_mom; a.partial = (sm_partial*)lc->d_partial; a.rec = lc->d_rec;

    hipStream_t st = ctx->stream;
    const unsigned ntiles = (unsigned)(((a.S + RL_TILE - 1) / RL_TILE) * ((a.S + RL_TILE - 1) / RL_TILE));
    BL_HIP(hipEventRecord(lc->ev[0], st));
    if (place) {
        pr_args p;
        memset(&p, 0, sizeof(p));
        p.n = n; p.Q = a.Q; p.stride = a.stride; p.min_gap = a.min_gap;
        p.head = a.head; p.capacity = a.capacity; p.max_rays = a.max_rays;
        p.bins_per_meter = place->bins_per_meter; p.max_range = place->max_range;
        p.dilate = place->dilate; p.min_key = place->min_key; p.min_bits = place->min_bits;
        p.scans = a.scans; p.kept = a.kept;
        p.desc = (uint32_t*)lc->d_desc; p.bits = (int32_t*)lc->d_bits; p.place = (bl_place_t*)lc->d_place; p.partner = a.partner;
        a.place = p.place;
        lc->place_n = n; lc->place_Q = a.Q; lc->placed = true;
        hipLaunchKernelGGL(k_pr_describe, dim3(n), dim3(256), 0, st, p);
        hipLaunchKernelGGL(k_pr_match, dim3(a.Q), dim3(64 * PR_WAVES), 0, st, p);
    } else {
        hipLaunchKernelGGL(k_lc_pairs, dim3(a.Q), dim3(64), 0, st, a);
    }
    hipLaunchKernelGGL(k_lc_number, dim3(1), dim3(1024), 0, st, a);
    BL_HIP(hipEventRecord(lc->ev[1], st));
    hipLaunchKernelGGL(k_lc_prep, dim3(a.slots), dim3(256), 0, st, a);
    if (a.W2 > 0) hipLaunchKernelGGL(k_lc_rays, dim3(a.W2, a.slots), dim3(RL_THREADS), 0, st, a);
    hipLaunchKernelGGL(k_lc_fold, dim3(ntiles, a.slots), dim3(RL_THREADS), 0, st, a);
    BL_HIP(hipEventRecord(lc->ev[2], st));
    hipLaunchKernelGGL(k_lc_raster, dim3((unsigned)(((long long)a.nk * a.rp_max + 255) / 256), a.slots), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_lc_score, dim3(slices, a.nk, a.slots), dim3(threads), lds_bytes, st, a);
    hipLaunchKernelGGL(k_lc_final, dim3(a.slots), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_lc_moments, dim3(a.mom_groups, a.slots), dim3(SM_MOM_THREADS), 0, st, a);
    hipLaunchKernelGGL(k_lc_moments_final, dim3(a.slots), dim3(256), 0, st, a);
    BL_HIP(hipEventRecord(lc->ev[3], st));
    hipLaunchKernelGGL(k_lc_records, dim3((a.slots + 255) / 256), dim3(256), 0, st, a);
    BL_HIP(hipGetLastError());
    BL_HIP(hipEventRecord(lc->ev[4], st));
    lc->timed = true;
    // the one read-back: M, the candidates and the records of every slot (a slot beyond M holds what an earlier find left)
    lc_state* h_state = (lc_state*)lc->staging;
    lc_cand* h_cand = (lc_cand*)(h_state + 1);
    bl_loopclose_candidate_t* h_rec = (bl_loopclose_candidate_t*)(h_cand + lc->maxc);
    BL_HIP(hipMemcpyAsync(h_state, lc->d_state, sizeof(lc_state), hipMemcpyDeviceToHost, st));
    BL_HIP(hipMemcpyAsync(h_cand, lc->d_cand, (size_t)a.slots * sizeof(lc_cand), hipMemcpyDeviceToHost, st));
    BL_HIP(hipMemcpyAsync(h_rec, lc->d_rec, (size_t)a.slots * sizeof(bl_loopclose_candidate_t), hipMemcpyDeviceToHost, st));
    BL_HIP(hipStreamSynchronize(st));
    if (!h_state->ok) {
        bl_set_error("%s: %d queries have a partner, the handle holds %d", place ? "bl_loopclose_find_places" : "bl_loopclose_find", h_state->M, lc->maxc);
        return BL_ERR_ARG;
    }
    const int M = h_state->M;
    lc->M = M; lc->S = a.S;
    lc->cands->assign(h_cand, h_cand + M);
    lc->recs->assign(h_rec, h_rec + M);
    for (int m = 0; m < M; ++m)
        if ((*lc->recs)[m].flags == 0) lc_edge(&(*lc->recs)[m], (*lc->cands)[m], (double)a.mpc, (double)a.dtheta);
    *n_candidates = M;
    return BL_OK;
}

extern "C" int bl_loopclose_find(bl_loopclose* lc, bl_scanlog* log, const bl_grid* like, const bl_loopclose_params_t* prm, int* n_candidates)
{
    BL_CHECK_ARG(lc != nullptr && log != nullptr && like != nullptr && prm != nullptr && n_candidates != nullptr);
    return lc_find(lc, log, like, prm, nullptr, n_candidates);
}

extern "C" int bl_loopclose_find_places(bl_loopclose* lc, bl_scanlog* log, const bl_grid* like, const bl_loopclose_params_t* prm,
                                        const bl_place_params_t* place, int* n_candidates)
{
    BL_CHECK_ARG(lc != nullptr && log != nullptr && like != nullptr && prm != nullptr && place != nullptr && n_candidates != nullptr);
    return lc_find(lc, log, like, prm, place, n_candidates);
}

// diagnostics of the last find_places that launched
extern "C" int bl_loopclose_places(bl_loopclose* lc, int* n_queries, bl_place_t* out)
{
    BL_CHECK_ARG(lc != nullptr && n_queries != nullptr);
    if (!lc->placed) { bl_set_error("bl_loopclose_places: no find_places yet"); return BL_ERR_STATE; }
    if (out) {
        BL_HIP(hipSetDevice(lc->ctx->device));
        BL_HIP(hipMemcpyAsync(out, lc->d_place, (size_t)lc->place_Q * sizeof(bl_place_t), hipMemcpyDeviceToHost, lc->ctx->stream));
        BL_HIP(hipStreamSynchronize(lc->ctx->stream));
    }
    *n_queries = lc->place_Q;
    return BL_OK;
}

extern "C" int bl_loopclose_descriptors(bl_loopclose* lc, int* n_entries, uint32_t* words, int32_t* bits)
{
    BL_CHECK_ARG(lc != nullptr && n_entries != nullptr);
    if (!lc->placed) { bl_set_error("bl_loopclose_descriptors: no find_places yet"); return BL_ERR_STATE; }
    BL_HIP(hipSetDevice(lc->ctx->device));
    const size_t n = (size_t)lc->place_n;
    if (words) BL_HIP(hipMemcpyAsync(words, lc->d_desc, n * PR_SECTORS * sizeof(uint32_t), hipMemcpyDeviceToHost, lc->ctx->stream));
    if (bits) BL_HIP(hipMemcpyAsync(bits, lc->d_bits, n * sizeof(int32_t), hipMemcpyDeviceToHost, lc->ctx->stream));
    BL_HIP(hipStreamSynchronize(lc->ctx->stream));
    *n_entries = lc->place_n;
    return BL_OK;
}

extern "C" int bl_loopclose_candidates(bl_loopclose* lc, bl_loopclose_candidate_t* out)
{
    BL_CHECK_ARG(lc != nullptr && (out != nullptr || lc->M == 0));
    if (lc->M > 0) memcpy(out, lc->recs->data(), (size_t)lc->M * sizeof(bl_loopclose_candidate_t));
    return BL_OK;
}

extern "C" int bl_loopclose_edges(bl_loopclose* lc, int* n, bl_posegraph_edge_t* out)
{
    BL_CHECK_ARG(lc != nullptr && n != nullptr);
    int k = 0;
    for (int m = 0; m < lc->M; ++m) {
        if ((*lc->recs)[m].flags != 0) continue;
        if (out) out[k] = (*lc->recs)[m].edge;
        ++k;
    }
    *n = k;
    return BL_OK;
}

extern "C" int bl_loopclose_submap(bl_loopclose* lc, int m, int8_t* cells, float* origin_xy)
{
    BL_CHECK_ARG(lc != nullptr && m >= 0 && m < lc->M);
    if (origin_xy) { origin_xy[0] = (*lc->cands)[m].ox; origin_xy[1] = (*lc->cands)[m].oy; }
    if (cells) {
        BL_HIP(hipSetDevice(lc->ctx->device));
        const size_t bytes = (size_t)lc->S * lc->S;
        BL_HIP(hipMemcpyAsync(cells, (const int8_t*)lc->d_sub + (size_t)m * bytes, bytes, hipMemcpyDeviceToHost, lc->ctx->stream));
        BL_HIP(hipStreamSynchronize(lc->ctx->stream));
    }
    return BL_OK;
}

extern "C" int bl_loopclose_last_device_ms(bl_loopclose* lc, float* ms, float* ms4)
{
    BL_CHECK_ARG(lc != nullptr && ms != nullptr);
    if (!lc->timed) { bl_set_error("bl_loopclose_last_device_ms: no find yet"); return BL_ERR_STATE; }
    BL_HIP(hipSetDevice(lc->ctx->device));
    BL_HIP(hipEventSynchronize(lc->ev[4]));
    BL_HIP(hipEventElapsedTime(ms, lc->ev[0], lc->ev[4]));
    if (ms4)
        for (int i = 0; i < 4; ++i) BL_HIP(hipEventElapsedTime(&ms4[i], lc->ev[i], lc->ev[i + 1]));
    return BL_OK;
}
