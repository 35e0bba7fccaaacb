// bl_scanmatch_seq_dev.h -- the match sequence of bl_scanmatch_match / bl_scanmatch_match_prior as device bodies: bl_scanmatch.hip
// launches them for one match, bl_loopclose.hip (the loop-closure front end) for a batch of matches with one more grid
// dimension, each match with its own header, map, endpoints, partial results and volume.  Each body is what its kernel was, statement
// for statement; a body reads blockIdx.x / blockIdx.y / gridDim.x as its kernel did (k_sm_raster's block index is a parameter).
//   device  the match header; the rasteriser; the map window of a match; the prior's penalty; the scoring loop; the result; the
//           moments pass (the weight, the streaming sums, their reduction and the sub-cell fractions)
//   host    which priors are accepted; the weight's reciprocal
#ifndef BL_SCANMATCH_SEQ_DEV_H
#define BL_SCANMATCH_SEQ_DEV_H

#include "bl_scanmatch_dev.h"

#define SM_MAX_NTHETA 180
#define SM_MAX_RAYS 4096
#define SM_LDS_MAX (152 * 1024)        // dynamic LDS a workgroup of k_sm_score may ask for (a CU has 160 KiB)

// device header of a match: parameters in, bounding box and result out
struct sm_head {
    float cx, cy, ctheta, dtheta;
    int64_t utime;
    int32_t nx, ny, ntheta, rays;
    int32_t min_score, pad;
    int32_t bbox[4];                   // x0, y0 (atomic min), x1, y1 (atomic max) of the endpoints that count
    int32_t score_centre, path;
    bl_scan_match_result_t result;
};

struct sm_block_best { unsigned long long key; uint32_t ties; uint32_t pad; };

// ---------------------------------------------------------------------------------------------------------------- rasteriser
// workgroup `block` of 256 threads, one thread per (heading, ray)
__device__ __forceinline__ void sm_raster_body(sm_head* __restrict__ head, const float* __restrict__ ranges,
                                               const float* __restrict__ thetas, const bl_frame& f, int2* __restrict__ ends, int block)
{
    const int rays = head->rays, nt = head->ntheta, nx = head->nx, ny = head->ny;
    const int rp = (rays + 63) & ~63;                                   // rows padded to whole waves of k_sm_score, sentinels in the pad
    const int total = (2 * nt + 1) * rp;
    const int t = block * 256 + threadIdx.x;
    int ex = SM_NONE, ey = SM_NONE;
    const int k = t / rp, r = t - k * rp;
    if (t < total && r < rays) {
        const float theta_k = head->ctheta + (float)(k - nt) * head->dtheta;
        float sx, sy;
        int ix, iy;
        bl_global_to_grid(head->cx, head->cy, f, &sx, &sy);
        if (sm_endpoint(ranges[r], thetas[r], theta_k, sx, sy, f, &ix, &iy) && ix >= -nx && ix < f.width + nx && iy >= -ny &&
            iy < f.height + ny) {
            ex = ix; ey = iy;
        }
    }
    if (t < total) ends[t] = make_int2(ex, ey);
    const bool on = ex != SM_NONE;
    int x0 = on ? ex : INT32_MAX, y0 = on ? ey : INT32_MAX, x1 = on ? ex : INT32_MIN, y1 = on ? ey : INT32_MIN;
    for (int off = 32; off > 0; off >>= 1) {
        x0 = min(x0, __shfl_xor(x0, off, 64)); y0 = min(y0, __shfl_xor(y0, off, 64));
        x1 = max(x1, __shfl_xor(x1, off, 64)); y1 = max(y1, __shfl_xor(y1, off, 64));
    }
    if ((threadIdx.x & 63) == 0 && x1 >= x0) {
        atomicMin(&head->bbox[0], x0); atomicMin(&head->bbox[1], y0);
        atomicMax(&head->bbox[2], x1); atomicMax(&head->bbox[3], y1);
    }
}

// ---------------------------------------------------------------------------------------------------------------- scoring
// the map window of a match: the endpoints' bounding box widened by the shifts, clipped to the grid
__device__ __forceinline__ sm_window sm_make_window(const sm_head* head, const bl_frame& f)
{
    const int bx0 = head->bbox[0], by0 = head->bbox[1], bx1 = head->bbox[2], by1 = head->bbox[3];
    return sm_clip_window(bx0 - head->nx, by0 - head->ny, bx1 + head->nx, by1 + head->ny, bx1 >= bx0, f);
}

// The prior of bl_scanmatch_match_prior as the kernels take it, and the objective's offset in the key's high word.
struct sm_prior_k { int32_t a_xx, a_xy, a_yy, a_tt; };
#define SM_OBJ_BIAS (1 << 23)
__device__ __forceinline__ int sm_pen(const sm_prior_k& p, int di, int dj, int dk)
{
    const long long q = (long long)p.a_xx * (di * di) + 2ll * p.a_xy * (di * dj) + (long long)p.a_yy * (dj * dj) +
                        (long long)p.a_tt * (dk * dk);               // 0 <= q < 2^31 within the limits
    return (int)(q >> 8);
}

// The scoring loop of both forms.  PRIOR = false is bl_scanmatch_match's kernel, statement for statement; PRIOR = true takes the
// penalty off once per candidate, behind the ray loop, and keys, stores and counts ties on the objective.
// grid: (slices, headings).  Dynamic LDS: uint8 window[lds_window_bytes].
template <bool PRIOR>
__device__ __forceinline__ void sm_score_body(sm_head* __restrict__ head, const int8_t* __restrict__ cells, const bl_frame& f,
                                              const int2* __restrict__ ends, int lds_window_bytes,
                                              sm_block_best* __restrict__ best, int32_t* __restrict__ volume, const sm_prior_k& pr)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    __shared__ unsigned long long s_key[16];
    __shared__ uint32_t s_ties[16];
    const int rays = head->rays, nt = head->ntheta, nx = head->nx, ny = head->ny;
    const int k = blockIdx.y, dk = k - nt;
    const int tid = threadIdx.x, nthreads = blockDim.x;
    unsigned char* s_win = s_raw;
    const int rp = (rays + 63) & ~63;                                   // a heading's row of endpoints, padded with sentinels
    const int2* __restrict__ k_ends = ends + (size_t)k * rp;
    const int lane = tid & 63;

    const sm_window win = sm_make_window(head, f);
    const bool staged = (long long)win.pitch * win.h <= (long long)lds_window_bytes;          // uniform over the whole launch
    if (staged && win.any) sm_stage_window(cells, f.width, win, s_win, tid, nthreads);
    __syncthreads();

    const int cw = 2 * nx + 1, ncand = cw * (2 * ny + 1);
    const int per = (ncand + gridDim.x - 1) / gridDim.x;                // candidates of this slice
    const int c_begin = blockIdx.x * per, c_end = min(ncand, c_begin + per);
    unsigned long long key = 0;
    int top = PRIOR ? INT32_MIN : -1; uint32_t ties = 0;                    // an objective is above -2^23
    for (int cb = c_begin + (tid & ~63); cb < c_end; cb += nthreads) {       // wave-uniform trip count: the broadcasts need every lane
        const int c = cb + lane;
        const int jrow = c / cw;
        const int di = c - jrow * cw - nx, dj = jrow - ny;
        int acc = staged ? sm_lookup_sum<false>(k_ends, rp, lane, (unsigned)(di - win.x0), (unsigned)(dj - win.y0), s_win, (unsigned)win.w,
                                                (unsigned)win.h, (unsigned)win.pitch)
                         : sm_lookup_sum<true>(k_ends, rp, lane, (unsigned)di, (unsigned)dj, (const unsigned char*)cells, (unsigned)f.width,
                                               (unsigned)f.height, (unsigned)f.width);
        if (c >= c_end) continue;
        if (PRIOR) acc -= sm_pen(pr, di, dj, dk);                            // from here on the objective; the centre's pen is 0
        if (volume) volume[(size_t)k * ncand + c] = acc;
        if (dk == 0 && di == 0 && dj == 0) head->score_centre = acc;
        const unsigned long long kc = sm_key(PRIOR ? acc + SM_OBJ_BIAS : acc, di, dj, dk);
        key = kc > key ? kc : key;
        if (acc > top) { top = acc; ties = 1; } else if (acc == top) ++ties;
    }
    // a thread without candidates has ties 0, whatever its top
    const sm_best wg = sm_block_best_key(key, (uint32_t)(PRIOR ? top + SM_OBJ_BIAS : top), ties, nthreads >> 6, s_key, s_ties);
    if (tid == 0) {
        sm_block_best b; b.key = wg.key; b.ties = (c_end > c_begin) ? wg.ties : 0; b.pad = 0;
        best[blockIdx.y * gridDim.x + blockIdx.x] = b;
        if (blockIdx.x == 0 && blockIdx.y == 0) head->path = staged ? 0 : 1;
    }
}

// ---------------------------------------------------------------------------------------------------------------- result
// the result struct of the plain, the prior and the wide match, from the winner and the header; one thread
__device__ __forceinline__ void sm_write_result(sm_head* __restrict__ head, const bl_frame& f, int di, int dj, int dk, int score,
                                                int32_t ties)
{
    bl_scan_match_result_t r;
    r.di = di; r.dj = dj; r.dk = dk;
    r.score = score;
    r.score_centre = head->score_centre;
    r.ties = ties;
    r.rays_used = head->rays;
    r.accepted = score >= head->min_score ? 1 : 0;
    r.pose.utime = head->utime;
    sm_result_pose(r.accepted != 0, head->cx, head->cy, head->ctheta, di, dj, dk, f.mpc, head->dtheta, &r.pose.x, &r.pose.y, &r.pose.theta);
    head->result = r;
}

// one workgroup of 256 threads
template <bool PRIOR>
__device__ __forceinline__ void sm_final_body(sm_head* __restrict__ head, const sm_block_best* __restrict__ best, int nblocks,
                                              const bl_frame& f, const sm_prior_k& pr, bl_scan_match_moments_t* __restrict__ mom)
{
    __shared__ unsigned long long s_key[4];
    __shared__ uint32_t s_ties[4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    unsigned long long key = 0;
    for (int i = tid; i < nblocks; i += 256) { const unsigned long long b = best[i].key; key = b > key ? b : key; }
    key = sm_wave_max(key);
    if (lane == 0) s_key[wave] = key;
    __syncthreads();
    key = 0;
    for (int w = 0; w < 4; ++w) key = s_key[w] > key ? s_key[w] : key;
    uint32_t n = 0;
    for (int i = tid; i < nblocks; i += 256) {
        const sm_block_best b = best[i];
        if (b.ties && (uint32_t)(b.key >> 32) == (uint32_t)(key >> 32)) n += b.ties;
    }
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, 64);
    if (lane == 0) s_ties[wave] = n;
    __syncthreads();
    if (tid == 0) {
        int score, di, dj, dk;
        sm_key_decode(key, &score, &di, &dj, &dk);
        if (PRIOR) {                                                         // the high word held obj + 2^23; the score is the raw one
            const int obj = score - SM_OBJ_BIAS, pen = sm_pen(pr, di, dj, dk);
            mom->best_obj = obj; mom->pen_best = pen;
            score = obj + pen;
        }
        sm_write_result(head, f, di, dj, dk, score, (int32_t)(s_ties[0] + s_ties[1] + s_ties[2] + s_ties[3]));
    }
}

// ---------------------------------------------------------------------------------------------------------------- moments
#define SM_MOM_THREADS 256
#define SM_MOM_MAX_GROUPS 1024
#define SM_MOM_BATCH 4                  // rows a wave has in flight
struct sm_partial { long long s[10]; };
static __constant__ int32_t c_sm_exp2[64] = { BL_SM_EXP2_VALUES };

__device__ __forceinline__ long long sm_wave_sum(long long v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// The weight of a candidate d >= 0 below the best objective.  t = floor(64 d / half_life) = 64 e + i (d = e half_life + f and
// 64 f / half_life < 64), taken as (64 d * magic) >> shift with shift = 30 + L, 2^L >= half_life, magic = ceil(2^shift / half_life)
// <= 2^30: for n = 64 d < 2^30 (d < 2^23 + 2^19) the product is n / half_life + n r / (half_life 2^shift) with 0 <= r < half_life,
// and the second term is below 2^-L <= 1 / half_life, so the floor is that of n / half_life.  The product is below 2^61.
__device__ __forceinline__ int sm_weight(int d, uint32_t magic, int shift, const int32_t* tab)
{
    const unsigned long long t = ((unsigned long long)((uint32_t)d << 6) * magic) >> shift;
    const uint32_t e = (uint32_t)(t >> 6), i = (uint32_t)t & 63u;
    return e >= 21u ? 0 : (tab[i] >> e);
}
// magic and shift of sm_weight for a half_life within 1 .. 2^20
static inline void sm_weight_magic(int half_life, uint32_t* magic, int* shift)
{
    int L = 0;
    while ((1 << L) < half_life) ++L;
    *shift = 30 + L;
    const unsigned long long hl = (unsigned long long)half_life;
    *magic = (uint32_t)(((1ull << *shift) + hl - 1) / hl);
}
// workgroups of the moments pass: a wave per SM_MOM_BATCH rows of the volume, at most SM_MOM_MAX_GROUPS
static inline int sm_moment_groups(int rows)
{
    const int g = (rows + SM_MOM_BATCH * (SM_MOM_THREADS / 64) - 1) / (SM_MOM_BATCH * (SM_MOM_THREADS / 64));
    return g > SM_MOM_MAX_GROUPS ? SM_MOM_MAX_GROUPS : g;
}

// grid: up to SM_MOM_MAX_GROUPS workgroups of four waves.  A row is the 2 nx + 1 objectives of one (dk, dj); wave g of G takes rows
// g, g + G, ..., SM_MOM_BATCH of them at a time, its lanes along di in chunks of 64, so a lane's di is fixed for a whole chunk pass
// and the row's dj, dk are wave-uniform: six running sums per lane (w, w dj, w dk, w dj dj, w dj dk, w dk dk) are folded into the
// ten moments with di once per chunk.  (dk, dj) of the next row come from adding the stride's quotient and remainder: no division
// per element or per row.
__device__ __forceinline__ void sm_moments_body(const sm_head* __restrict__ head, const int32_t* __restrict__ volume,
                                                const bl_scan_match_moments_t* __restrict__ mom, uint32_t magic, int shift,
                                                sm_partial* __restrict__ partial)
{
    __shared__ int32_t s_tab[64];
    __shared__ long long s_part[SM_MOM_THREADS / 64][10];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (tid < 64) s_tab[tid] = c_sm_exp2[tid];
    __syncthreads();
    const int nt = head->ntheta, nx = head->nx, ny = head->ny;
    const int cw = 2 * nx + 1, ch = 2 * ny + 1, rows = (2 * nt + 1) * ch;
    const int best = mom->best_obj;
    const int nwaves = (int)gridDim.x * (SM_MOM_THREADS / 64);
    const int g = __builtin_amdgcn_readfirstlane((int)blockIdx.x * (SM_MOM_THREADS / 64) + wave);
    const int step_k = nwaves / ch, step_j = nwaves - step_k * ch;          // the stride from a row to the wave's next one
    long long m[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) m[i] = 0;
    for (int x0 = 0; x0 < cw; x0 += 64) {                                    // at most three chunks (cw <= 129)
        const int xi = x0 + lane;
        const bool on = xi < cw;
        const int di = xi - nx;
        long long a = 0, b = 0, c = 0, d2 = 0, e2 = 0, f2 = 0;
        int k = g / ch, j = g - k * ch;                                      // of row r; once per chunk
        for (int r = g; r < rows; r += SM_MOM_BATCH * nwaves) {              // wave-uniform
            int v[SM_MOM_BATCH];
#pragma unroll
            for (int u = 0; u < SM_MOM_BATCH; ++u) {
                const long long ru = (long long)r + (long long)u * nwaves;
                v[u] = (on && ru < rows) ? volume[(size_t)ru * cw + xi] : best;           // ru < rows, xi < cw: below rows * cw
            }
#pragma unroll
            for (int u = 0; u < SM_MOM_BATCH; ++u) {
                const long long ru = (long long)r + (long long)u * nwaves;
                const int dj = j - ny, dk = k - nt;
                int w = sm_weight(best - v[u], magic, shift, s_tab);
                w = (on && ru < rows) ? w : 0;
                a += w;
                b += (long long)w * dj;
                c += (long long)w * dk;
                d2 += (long long)w * (dj * dj);
                e2 += (long long)w * (dj * dk);
                f2 += (long long)w * (dk * dk);
                k += step_k; j += step_j;
                if (j >= ch) { j -= ch; ++k; }
            }
        }
        m[0] += a; m[1] += a * di; m[2] += b; m[3] += c; m[4] += a * (di * di);
        m[5] += b * di; m[6] += d2; m[7] += c * di; m[8] += e2; m[9] += f2;
    }
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const long long t = sm_wave_sum(m[i]);
        if (lane == 0) s_part[wave][i] = t;
    }
    __syncthreads();
    if (tid < 10) {
        long long t = 0;
        for (int w = 0; w < SM_MOM_THREADS / 64; ++w) t += s_part[w][tid];
        partial[blockIdx.x].s[tid] = t;
    }
}

// one workgroup of 256 threads: the sum of the records; the sub-cell fractions from the winner's neighbours along each axis, read
// only behind the edge test (the neighbours of a candidate inside the window are inside the volume)
__device__ __forceinline__ void sm_moments_final_body(const sm_head* __restrict__ head, const int32_t* __restrict__ volume,
                                                      const sm_partial* __restrict__ partial, int nparts,
                                                      bl_scan_match_moments_t* __restrict__ mom)
{
    __shared__ long long s_part[4][10];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    long long m[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) m[i] = 0;
    for (int p = tid; p < nparts; p += 256) {
#pragma unroll
        for (int i = 0; i < 10; ++i) m[i] += partial[p].s[i];
    }
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const long long t = sm_wave_sum(m[i]);
        if (lane == 0) s_part[wave][i] = t;
    }
    __syncthreads();
    if (tid == 0) {
        long long t[10];
        for (int i = 0; i < 10; ++i) t[i] = s_part[0][i] + s_part[1][i] + s_part[2][i] + s_part[3][i];
        mom->s0 = t[0]; mom->sx = t[1]; mom->sy = t[2]; mom->st = t[3]; mom->sxx = t[4];
        mom->sxy = t[5]; mom->syy = t[6]; mom->sxt = t[7]; mom->syt = t[8]; mom->stt = t[9];
        const int nt = head->ntheta, nx = head->nx, ny = head->ny, cw = 2 * nx + 1, ch = 2 * ny + 1;
        const int di = head->result.di, dj = head->result.dj, dk = head->result.dk;
        const size_t at = ((size_t)(dk + nt) * ch + (size_t)(dj + ny)) * cw + (size_t)(di + nx);
        const int o0 = mom->best_obj;
        const int half[3] = { nx, ny, nt }, pos[3] = { di, dj, dk };
        const size_t stride[3] = { (size_t)1, (size_t)cw, (size_t)cw * ch };
        for (int ax = 0; ax < 3; ++ax) {
            int num = 0, den = 1;
            if (half[ax] >= 1 && pos[ax] > -half[ax] && pos[ax] < half[ax]) {
                const int om = volume[at - stride[ax]], op = volume[at + stride[ax]];
                den = 2 * (2 * o0 - om - op); num = op - om;
                if (den == 0) { num = 0; den = 1; }
            }
            mom->sub_num[ax] = num; mom->sub_den[ax] = den;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- host
static inline bool sm_prior_ok(const bl_scan_match_prior_t* p)
{
    const int m = BL_SM_MAX_COEFF;
    if (p->a_xx < 0 || p->a_xx > m || p->a_yy < 0 || p->a_yy > m || p->a_tt < 0 || p->a_tt > m || p->a_xy < -m || p->a_xy > m) return false;
    return (long long)p->a_xy * p->a_xy <= (long long)p->a_xx * p->a_yy;
}

// Slices of a heading's candidates for k_sm_score: enough workgroups (`want` over all headings) to fill the device, none with less
// than a workgroup of candidates.  *threads: the workgroup size.
static inline int sm_score_slices(int ncand, int nk, int want, int* threads)
{
    *threads = ncand >= 4096 ? 1024 : 256;
    int slices = (want + nk - 1) / nk;
    const int max_slices = (ncand + *threads - 1) / *threads;
    if (slices > max_slices) slices = max_slices;
    if (slices < 1) slices = 1;
    return slices;
}

// LDS for the window of a match whose valid rays reach at most rmax metres: an upper bound of what the device will find (every
// endpoint lies within the longest range, a cell of slack for each rounding, of the centre; the window is that box widened by the
// shifts, clipped to the grid).  The device compares the window it really needs with what it was given, so an optimistic bound could
// only cost the staging.  0: no staging.
static inline int sm_window_lds(float rmax, const bl_frame& f, int nx, int ny)
{
    const double reach = (double)rmax * (double)f.cpm + 3.0;
    double bw = 2.0 * reach + 1.0 + 2.0 * nx + 4.0, bh = 2.0 * reach + 1.0 + 2.0 * ny;
    if (!(bw < (double)f.width)) bw = (double)f.width;                  // also catches NaN
    if (!(bh < (double)f.height)) bh = (double)f.height;
    const size_t win_bytes = (size_t)(((int)bw + 3) & ~3) * (size_t)(int)bh;
    return win_bytes <= (size_t)SM_LDS_MAX ? (int)win_bytes : 0;
}

#endif  // BL_SCANMATCH_SEQ_DEV_H
