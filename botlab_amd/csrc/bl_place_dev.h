// bl_place_dev.h -- place recognition for the loop-closure front end (include/botlab_hip.h, "loop closure by place recognition";
// DESIGN.md 4.34): a descriptor per logged scan, and per query the older scan and the circular shift at which the descriptors
// overlap most.  Integer work throughout; the numpy restatement, bit for bit, is tests/place_model.py.
//   k_pr_describe   a workgroup per log entry: 64 words of LDS set by atomicOr, stored by one wave, which also sums the popcounts.
//   k_pr_match      a workgroup per query: lane = shift, a wave takes PR_GROUP partners per read of the query's words from LDS.
#ifndef BL_PLACE_DEV_H
#define BL_PLACE_DEV_H

#include "bl_internal.h"
#include "bl_scanlog_dev.h"
#include "bl_scanmatch_dev.h"

#define PR_SECTORS BL_PLACE_SECTORS
#define PR_BINS BL_PLACE_BINS
#define PR_K 10.185916f                      // the float nearest 32 / pi
#define PR_STEP 0.09817477f                  // the float nearest 2 pi / 64
#define PR_MAX_THETA 1024.0f
// Partners per LDS read of a wave, and waves of a workgroup.  Measured (describe + match, 1024 scans, stride 4 /
// stride 1, ms): 4 waves x 4: 0.237 / 0.261; 8 x 4: 0.136 / 0.217; 8 x 2: 0.147 / 0.232; 16 x 4: 0.098 / 0.226; 16 x 2: 0.103 / 0.238;
// 16 x 1: 0.117 / 0.247.  Groups of four are the fastest at every wave count; sixteen waves shorten the longest query's chain.
#define PR_GROUP 4
#define PR_WAVES 16

struct pr_args {
    int n, Q, stride, min_gap;
    int head, capacity, max_rays;
    float bins_per_meter, max_range;
    int dilate, min_key, min_bits;
    char* scans; const int* kept;
    uint32_t* desc;                          // n x 64
    int32_t* bits;                           // n
    bl_place_t* place;                       // Q
    int* partner;                            // Q
};

// ---------------------------------------------------------------- descriptors
// grid: n.  Rays beyond 256 take further trips.
__global__ __launch_bounds__(256) void k_pr_describe(pr_args a)
{
    __shared__ unsigned int s_d[PR_SECTORS];
    const int e = blockIdx.x, tid = threadIdx.x;
    if (tid < PR_SECTORS) s_d[tid] = 0u;
    __syncthreads();
    const int slot = (a.head + e) % a.capacity;
    const int kept = min(a.kept[slot], a.max_rays);
    const rl_slot s = rl_slot_of(a.scans, a.max_rays, slot);
    for (int r = tid; r < kept; r += 256) {
        const float rng = s.ranges[r], th = s.thetas[r];
        if (!sm_ray_valid(rng, a.max_range) || !(fabsf(th) <= PR_MAX_THETA)) continue;
        const int sec = (int)floorf(th * PR_K) & (PR_SECTORS - 1);
        const int bin = min((int)(rng * a.bins_per_meter), PR_BINS - 1);
        atomicOr(&s_d[sec], 1u << bin);
    }
    __syncthreads();
    if (tid < PR_SECTORS) {                                     // wave 0
        const unsigned int w = s_d[tid];
        a.desc[(size_t)e * PR_SECTORS + tid] = w;
        int c = __popc(w);
        for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
        if (tid == 0) a.bits[e] = c;
    }
}

// ---------------------------------------------------------------- best pairs
// (key descending, j ascending, s ascending) as one 64-bit order: greater is better, 0 is "none" (a best has j < 2^31)
__device__ __forceinline__ unsigned long long pr_order(int key, int j, int s)
{
    return ((unsigned long long)(unsigned)key << 38) | ((unsigned long long)(0xffffffffu - (unsigned)j) << 6) | (unsigned long long)(63 - s);
}

// grid: Q.  Group g of PR_GROUP partners is wave g % PR_WAVES' on its trip g / PR_WAVES: j = 4 g .. 4 g + 3.
__global__ __launch_bounds__(64 * PR_WAVES) void k_pr_match(pr_args a)
{
    __shared__ unsigned int s_q2[2 * PR_SECTORS];               // D'q twice in a row: lane s reads word a + s with no mask
    __shared__ int s_bits;
    __shared__ unsigned long long s_ord[PR_WAVES];
    __shared__ int s_ov[PR_WAVES];
    const int qi = blockIdx.x, q = qi * a.stride, tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int last = q - a.min_gap - 1;
    const int bits_q = a.bits[q];
    if (tid < PR_SECTORS) {
        unsigned int w = a.desc[(size_t)q * PR_SECTORS + tid];
        if (a.dilate) w = w | (w << 1) | (w >> 1);
        s_q2[tid] = w; s_q2[tid + PR_SECTORS] = w;
        int c = __popc(w);
        for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
        if (tid == 0) s_bits = c;
    }
    __syncthreads();
    const unsigned int bits_dq = (unsigned int)s_bits;
    unsigned long long best = 0ull;
    int best_ov = 0;
    if (bits_q >= a.min_bits) {
        for (int j0 = wv * PR_GROUP; j0 <= last; j0 += PR_WAVES * PR_GROUP) {      // uniform over the wave, ascending j
            // a partner of the group beyond `last` reads entry `last` again and is dropped below: no read beyond the n entries
            const uint32_t* dj[PR_GROUP];
#pragma unroll
            for (int g = 0; g < PR_GROUP; ++g) dj[g] = a.desc + (size_t)min(j0 + g, last) * PR_SECTORS;
            unsigned int ov[PR_GROUP];
#pragma unroll
            for (int g = 0; g < PR_GROUP; ++g) ov[g] = 0u;
#pragma unroll 8
            for (int s = 0; s < PR_SECTORS; ++s) {
                const unsigned int w = s_q2[s + lane];
#pragma unroll
                for (int g = 0; g < PR_GROUP; ++g) ov[g] += __popc(w & dj[g][s]);
            }
#pragma unroll
            for (int g = 0; g < PR_GROUP; ++g) {
                const int j = j0 + g;
                if (j > last) break;                            // uniform
                const int bj = a.bits[j];
                if (bj < a.min_bits) continue;                  // uniform
                const unsigned int den = bits_dq + (unsigned int)bj - ov[g];
                const unsigned int key = den == 0u ? 0u : (ov[g] << 16) / den;
                const unsigned long long o = pr_order((int)key, j, lane);
                if ((o >> 38) > (best >> 38) || best == 0ull) { best = o; best_ov = (int)ov[g]; }   // a strict > on the key
            }
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long oo = __shfl_xor(best, off, 64);
        const int ov = __shfl_xor(best_ov, off, 64);
        if (oo > best) { best = oo; best_ov = ov; }
    }
    if (lane == 0) { s_ord[wv] = best; s_ov[wv] = best_ov; }
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < PR_WAVES; ++k)
            if (s_ord[k] > best) { best = s_ord[k]; best_ov = s_ov[k]; }
        bl_place_t p;
        p.q = q; p.bits_q = bits_q;
        if (best == 0ull) {
            p.j = -1; p.shift = 0; p.key = 0; p.overlap = 0; p.bits_j = 0; p.partner = -1;
        } else {
            p.key = (int)(best >> 38);
            p.j = (int)(0xffffffffu - (unsigned)((best >> 6) & 0xffffffffull));
            p.shift = 63 - (int)(best & 63ull);
            p.overlap = best_ov;
            p.bits_j = a.bits[p.j];
            p.partner = p.key >= a.min_key ? p.j : -1;
        }
        a.place[qi] = p;
        a.partner[qi] = p.partner;
    }
}

#endif
