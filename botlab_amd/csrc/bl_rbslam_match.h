// bl_rbslam_match.h -- step 3b of a moved bl_rbslam_update with scan matching on: every particle matches the scan against ITS OWN map in
// a small window around the pose the action left, and moves to the best pose there.  Included by bl_rbslam.hip (the object's struct is
// private to that file), after rb_weigh_args and rb_action.  The definition is botlab_hip.h's "correlative scan matching" word for
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

#define RBM_THREADS 512
#define RBM_MAX_RAYS BL_RBSLAM_MATCH_MAX_RAYS
#define RBM_MAX_SLICES 64
#define RBM_WINDOW_BYTES BL_RBSLAM_MATCH_WINDOW_BYTES
#define RBM_WHOLE (1 << 20)                  // a half window of this many cells or more: the window is the whole grid
#define RBM_NONE (-(1 << 30))                // x of an endpoint without a cell: no shift brings it into a window
#define RBM_MIN_RANGE 0.15f                  // moving_laser_scan.cpp:24

struct rb_match_args {
    int rays;                                // valid rays: 0.15f < range < max_range
    const float* ranges; const float* thetas;
    int nx, ny, ntheta; float dtheta; int min_score;
    int hx, hy;                              // half window in cells: reach + n + 1, or RBM_WHOLE
    int ends_bytes;                          // dynamic LDS: int2 ends[rays] | uint8 window[]
    int32_t* out;                            // di | dj | dk | score | score_centre | ties | accepted, P entries each
};

// The candidate order of the definition as one unsigned key (bl_scanmatch.hip's sm_key): score, then small di*di + dj*dj, small |dk|,
// small dk, small dj, small di.  Given d2 and dj, di is known up to its sign, and given |dk|, dk likewise: one bit each.
__device__ __forceinline__ unsigned long long rbm_key(int score, int di, int dj, int dk)
{
    const uint32_t d2 = (uint32_t)(di * di + dj * dj);                 // <= 128
    const uint32_t adk = (uint32_t)(dk < 0 ? -dk : dk);                // <= 16
    const uint32_t lo = ((16383u - d2) << 18) | ((255u - adk) << 10) | ((dk <= 0 ? 1u : 0u) << 9) | ((uint32_t)(64 - dj) << 1) |
                        (di <= 0 ? 1u : 0u);
    return ((unsigned long long)(uint32_t)score << 32) | lo;
}
__device__ __forceinline__ void rbm_key_decode(unsigned long long key, int* score, int* di, int* dj, int* dk)
{
    const uint32_t lo = (uint32_t)key;
    const int d2 = 16383 - (int)(lo >> 18);
    const int adk = 255 - (int)((lo >> 10) & 255u);
    *dk = (lo & 512u) ? -adk : adk;
    *dj = 64 - (int)((lo >> 1) & 255u);
    int a = 0;
    while ((a + 1) * (a + 1) <= d2 - *dj * *dj) ++a;                    // at most 8 steps, once per particle
    *di = (lo & 1u) ? -a : a;
    *score = (int)(uint32_t)(key >> 32);
}

__device__ __forceinline__ uint32_t rbm_positive_bytes(uint32_t v)     // max(0, b) of four signed bytes
{
    const uint32_t neg = (v >> 7) & 0x01010101u;
    return v & ~(neg * 0xffu);
}

template <bool STAGED>
__global__ __launch_bounds__(RBM_THREADS) void k_rb_match(rb_weigh_args a, rb_match_args q)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    __shared__ int s_part[RBM_THREADS];
    __shared__ unsigned long long s_key[RBM_THREADS / 64];
    __shared__ uint32_t s_ties[RBM_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, m = blockIdx.x;
    int2* s_ends = (int2*)s_raw;
    unsigned char* s_win = s_raw + q.ends_bytes;
    const bl_frame& f = a.frame;

    // ---- step 3, the same in every thread
    const float4 s = a.src[a.idx[m]];
    float px, py, pth;
    rb_action(a, m, s, &px, &py, &pth);

    // ---- the window of this particle
    float sx, sy;
    bl_global_to_grid(px, py, f, &sx, &sy);
    const bool near = __builtin_fabsf(sx) < 0x1p29f && __builtin_fabsf(sy) < 0x1p29f;      // false for NaN
    const int cx = near ? (int)sx : 0, cy = near ? (int)sy : 0;
    int x0 = 0, y0 = 0, x1 = f.width - 1, y1 = f.height - 1;
    bool any = true;
    if (q.hx < RBM_WHOLE) { any = near; x0 = max(cx - q.hx, 0); x1 = min(cx + q.hx, f.width - 1); }
    if (q.hy < RBM_WHOLE) { any = any && near; y0 = max(cy - q.hy, 0); y1 = min(cy + q.hy, f.height - 1); }
    const bool dwords = (f.width & 3) == 0;
    if (dwords) x0 &= ~3;
    any = any && x1 >= x0 && y1 >= y0;
    const int w = any ? x1 - x0 + 1 : 0, h = any ? y1 - y0 + 1 : 0;
    const int pitch = (w + 3) & ~3;
    const int8_t* cells = a.maps + (size_t)a.slot[m] * a.stride;
    if (STAGED) {
        if (dwords) {
            const int qw = pitch >> 2;                                  // x0 and the grid width are multiples of four: whole dwords lie inside the row
            for (int i = tid; i < qw * h; i += RBM_THREADS) {
                const int row = i / qw, c4 = i - row * qw;
                const uint32_t v = *(const uint32_t*)(cells + (size_t)(y0 + row) * f.width + x0 + 4 * c4);
                *(uint32_t*)(s_win + row * pitch + 4 * c4) = rbm_positive_bytes(v);
            }
        } else {
            for (int i = tid; i < pitch * h; i += RBM_THREADS) {
                const int row = i / pitch, col = i - row * pitch;
                int v = 0;
                if (col < w) v = cells[(size_t)(y0 + row) * f.width + x0 + col];
                s_win[i] = (unsigned char)(v > 0 ? v : 0);
            }
        }
    }

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
            const float ang = bl_wrap_to_pi(theta_k - q.thetas[r]);   // moving_laser_scan.cpp:33
            float sn, cs;
            bl_sincosf_cells(ang, &sn, &cs);
            const float range = q.ranges[r];
            const float fx = range * cs * f.cpm + sx;                   // sensor_model.cpp:34-35
            const float fy = range * sn * f.cpm + sy;
            int2 e = make_int2(RBM_NONE, RBM_NONE);
            // beyond +-2^30 (or NaN) the endpoint is nowhere near a grid: it counts nothing, and the conversion is never asked for it
            if (__builtin_fabsf(fx) < 0x1p30f && __builtin_fabsf(fy) < 0x1p30f) e = make_int2((int)fx - x0, (int)fy - y0);
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
            const unsigned long long kc = rbm_key(acc, di, dj, dk);
            key = kc > key ? kc : key;
            if (acc > top) { top = acc; ties = 1; } else if (acc == top) ++ties;
        }
    }
    // ---- the particle's best key, and how many candidates share its score
    unsigned long long wkey = key;
    for (int off = 32; off > 0; off >>= 1) { const unsigned long long o = __shfl_xor(wkey, off, 64); wkey = o > wkey ? o : wkey; }
    if (lane == 0) s_key[wave] = wkey;
    __syncthreads();
    unsigned long long bkey = 0;
    for (int k = 0; k < RBM_THREADS / 64; ++k) bkey = s_key[k] > bkey ? s_key[k] : bkey;
    uint32_t n = (tid < ncand && (uint32_t)top == (uint32_t)(bkey >> 32)) ? ties : 0;
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, 64);
    if (lane == 0) s_ties[wave] = n;
    __syncthreads();
    if (tid == q.ny * cw + q.nx) q.out[4 * a.P + m] = centre;           // the thread that owns (0, 0)
    if (tid == 0) {
        uint32_t total = 0;
        for (int k = 0; k < RBM_THREADS / 64; ++k) total += s_ties[k];
        int score, bi, bj, bk;
        rbm_key_decode(bkey, &score, &bi, &bj, &bk);
        const int accepted = score >= q.min_score ? 1 : 0;
        if (accepted && (bi != 0 || bj != 0 || bk != 0)) {
            px = (float)((double)px + (double)bi * (double)f.mpc);
            py = (float)((double)py + (double)bj * (double)f.mpc);
            pth = bl_wrap_to_pi(pth + (float)bk * q.dtheta);
        }
        a.dst[m] = make_float4(px, py, pth, 0.0f);
        a.parent[m] = make_float4(s.x, s.y, s.z, 0.0f);
        q.out[m] = bi; q.out[a.P + m] = bj; q.out[2 * a.P + m] = bk; q.out[3 * a.P + m] = score;
        q.out[5 * a.P + m] = (int32_t)total; q.out[6 * a.P + m] = accepted;
    }
}

#endif  // BL_RBSLAM_MATCH_H
