// bl_obstracks.hip -- the obstacle tracks (include/botlab_hip.h, "obstacle tracks"): the obstacle layer's live cells grouped into
// blobs, the blobs followed from update to update, and a composed grid that also holds where the moving ones are heading.  No
// reference counterpart; the definition in the header is the contract and tests/obstacle_tracks_model.py restates it.
//
// An update is the layer's own three list launches (obs_live_list_enqueue, bl_obslayer_dev.h) and five of this file, all on the ctx
// stream.  The host never learns the number of live cells, so every per-cell launch of an update has the shape of the largest list
// (OBT_BLOCKS x OBT_WG) and the threads behind the list leave at once.
//   k_obt_init     parent[c] = c for the cells of the list, the blob records emptied.  The parent array has an entry per cell of the
//                  grid, but only the entries of this update's live cells are written or read: it is never cleared.
//   k_obt_link     a thread per live cell probes E, SW, S, SE in the layer's state and unites: k_pfc_link's lock-free union-find
//                  (the larger root hooked under the smaller by one CAS, path halving; every walk is strictly decreasing).  A
//                  component's root ends up as its least flat index: the representative.
//   k_obt_rank     one workgroup: the roots counted along the list (which is in flat-index order), so a root's prefix count is its
//                  blob's rank.
//   k_obt_fold     a thread per live cell: its root's rank is its label; area, sums and box go to the blob's record with integer
//                  atomics (exact, so the order is free).  A wave whose cells share one blob adds once.
//   k_obt_assoc    one workgroup of 1024: centroids, rounds of mutual best between free tracks and free blobs, the transition on a
//                  copy of the slots in LDS, births in rank order by one wave, and only then -- unless the id limit refuses the
//                  update -- the slots written back.
//   k_obt_sweep    (compose, after the layer's own k_obs_compose) a thread per (live cell, sub-step), in strides: the cell's stamp.
//   k_obt_static   (compose_static, after the layer's own k_obs_compose) a thread per live cell: a confirmed moving track's cell takes
//                  the map's value back.
// Integers only; no result depends on the launch shape or on the order in which anything arrives.
#include <limits.h>
#include <string.h>

#include "bl_internal.h"
#include "bl_obslayer_dev.h"

#define OBT_WG 256
#define OBT_BLOCKS (BL_OBSTRACKS_MAX_CELLS / OBT_WG)
#define OBT_ASSOC_WG 1024
#define OBT_SWEEP_BLOCKS 64                // of k_obt_sweep: 16384 threads in strides
#define OBT_SAT 65535
#define OBT_VMAX 1023
#define OBT_POS_MAX (1 << 30)

// the device's counters (int32 each): what bl_obstracks_stats reports, and what the next launch needs of the last
enum { OBT_L = 0, OBT_BLOBS, OBT_KEPT, OBT_ELIGIBLE, OBT_MATCHED, OBT_BORN, OBT_DELETED, OBT_UNBORN, OBT_TRACKS, OBT_CONFIRMED, OBT_REFUSED,
       OBT_ROUNDS, OBT_NEXT_ID, OBT_HDR_WORDS = 16 };

__device__ __forceinline__ unsigned int obt_ld(const unsigned int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// root of x; parent[i] <= i, so every step goes down and the walk is bounded by the number of cells
__device__ __forceinline__ unsigned int obt_find(unsigned int* parent, unsigned int x, unsigned int bound, bool halve)
{
    for (unsigned int step = 0; step < bound; ++step) {
        const unsigned int p = obt_ld(parent + x);
        if (p == x) return x;
        const unsigned int g = obt_ld(parent + p);
        if (halve && g != p) __hip_atomic_store(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = g;
    }
    return x;
}

// a failed CAS means that another thread hooked the root this one held, which then finds a smaller one
__device__ __forceinline__ void obt_unite(unsigned int* parent, unsigned int a, unsigned int b, unsigned int bound)
{
    for (unsigned int round = 0; round <= bound; ++round) {
        a = obt_find(parent, a, bound, true);
        b = obt_find(parent, b, bound, true);
        if (a == b) return;
        if (a < b) { const unsigned int t = a; a = b; b = t; }
        if (atomicCAS(parent + a, a, b) == a) return;
    }
}

__global__ __launch_bounds__(OBT_WG) void k_obt_init(const int* __restrict__ totals, int* __restrict__ hdr, const int32_t* __restrict__ xy,
                                                     unsigned int* __restrict__ parent, bl_obsblob_t* __restrict__ blobs, int W)
{
    const int L = totals[0];
    const int i = (int)blockIdx.x * OBT_WG + (int)threadIdx.x;
    if (i == 0) { hdr[OBT_L] = L; hdr[OBT_BLOBS] = 0; hdr[OBT_KEPT] = 0; }
    if (i < BL_OBSTRACKS_MAX_BLOBS) {
        bl_obsblob_t b;
        b.sum_x = 0; b.sum_y = 0; b.area = 0; b.x0 = INT_MAX; b.y0 = INT_MAX; b.x1 = -1; b.y1 = -1; b.cx = 0; b.cy = 0; b.eligible = 0;
        b.track = -1; b.rep = -1;
        blobs[i] = b;
    }
    if (L > BL_OBSTRACKS_MAX_CELLS || i >= L) return;
    const unsigned int c = (unsigned int)xy[2 * i + 1] * (unsigned int)W + (unsigned int)xy[2 * i];
    parent[c] = c;
}

__global__ __launch_bounds__(OBT_WG) void k_obt_link(const int* __restrict__ hdr, const int32_t* __restrict__ xy, unsigned int* parent,
                                                     const uint8_t* __restrict__ count, const uint32_t* __restrict__ last, int W, int H,
                                                     obs_live_rule q)
{
    const int L = hdr[OBT_L];
    const int i = (int)blockIdx.x * OBT_WG + (int)threadIdx.x;
    if (L > BL_OBSTRACKS_MAX_CELLS || i >= L) return;
    const int x = xy[2 * i], y = xy[2 * i + 1];
    const unsigned int bound = (unsigned int)W * (unsigned int)H;
    const unsigned int c = (unsigned int)y * (unsigned int)W + (unsigned int)x;
    const int dxs[4] = {1, -1, 0, 1}, dys[4] = {0, 1, 1, 1};            // E, SW, S, SE: the other four are some other cell's
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int nx = x + dxs[k], ny = y + dys[k];
        if (nx < 0 || nx >= W || ny >= H) continue;                     // nothing outside the grid is read
        const size_t ni = (size_t)ny * W + nx;
        const uint32_t cnt = count[ni];
        if (cnt >= q.min_hits && obs_live(q, cnt, last[ni])) obt_unite(parent, c, (unsigned int)ni, bound);
    }
}

// one workgroup.  The list is in flat-index order and a blob's root is its least cell, so the number of roots before a root in the
// list is the blob's rank.
__global__ __launch_bounds__(OBT_ASSOC_WG) void k_obt_rank(int* __restrict__ hdr, const int32_t* __restrict__ xy, const unsigned int* __restrict__ parent,
                                                           int* __restrict__ cellrank, bl_obsblob_t* __restrict__ blobs, int W)
{
    __shared__ int s_n[OBT_ASSOC_WG];
    const int L = hdr[OBT_L];
    if (L > BL_OBSTRACKS_MAX_CELLS) return;                             // (uniform)
    const int t = threadIdx.x;
    const int per = (L + OBT_ASSOC_WG - 1) / OBT_ASSOC_WG;
    const int i0 = min(t * per, L), i1 = min(i0 + per, L);
    int roots = 0;
    for (int i = i0; i < i1; ++i) {
        const unsigned int c = (unsigned int)xy[2 * i + 1] * (unsigned int)W + (unsigned int)xy[2 * i];
        roots += parent[c] == c ? 1 : 0;
    }
    s_n[t] = roots;
    __syncthreads();
    for (int off = 1; off < OBT_ASSOC_WG; off <<= 1) {                  // inclusive scan
        const int a = t >= off ? s_n[t - off] : 0;
        __syncthreads();
        s_n[t] += a;
        __syncthreads();
    }
    int rank = s_n[t] - roots;
    for (int i = i0; i < i1; ++i) {
        const unsigned int c = (unsigned int)xy[2 * i + 1] * (unsigned int)W + (unsigned int)xy[2 * i];
        if (parent[c] == c) {
            cellrank[c] = rank;
            if (rank < BL_OBSTRACKS_MAX_BLOBS) blobs[rank].rep = (int32_t)c;
            ++rank;
        }
    }
    if (t == OBT_ASSOC_WG - 1) { hdr[OBT_BLOBS] = s_n[t]; hdr[OBT_KEPT] = min(s_n[t], BL_OBSTRACKS_MAX_BLOBS); }
}

__global__ __launch_bounds__(OBT_WG) void k_obt_fold(const int* __restrict__ hdr, const int32_t* __restrict__ xy, unsigned int* parent,
                                                     const int* __restrict__ cellrank, bl_obsblob_t* blobs, int32_t* __restrict__ label, int W, int H)
{
    const int L = hdr[OBT_L];
    if (L > BL_OBSTRACKS_MAX_CELLS) return;                             // (uniform)
    const int i = (int)blockIdx.x * OBT_WG + (int)threadIdx.x;
    int rank = -1, x = 0, y = 0;
    if (i < L) {
        x = xy[2 * i]; y = xy[2 * i + 1];
        const unsigned int r = obt_find(parent, (unsigned int)y * (unsigned int)W + (unsigned int)x, (unsigned int)W * (unsigned int)H, false);
        const int rk = cellrank[r];
        rank = rk < BL_OBSTRACKS_MAX_BLOBS ? rk : -1;
        label[i] = rank;
    }
    // every lane of the wave is here
    const unsigned long long m = __ballot(rank >= 0);
    if (m == 0ull) return;
    const int first = __shfl(rank, __ffsll((long long)m) - 1, 64);
    if (__all(rank < 0 || rank == first)) {                             // one blob in this wave: one lane adds for all
        const bool on = rank >= 0;
        int a = on ? 1 : 0, x0 = on ? x : INT_MAX, y0 = on ? y : INT_MAX, x1 = on ? x : -1, y1 = on ? y : -1;
        unsigned long long sx = on ? (unsigned long long)x : 0ull, sy = on ? (unsigned long long)y : 0ull;
        for (int off = 32; off > 0; off >>= 1) {
            a += __shfl_xor(a, off, 64);
            sx += __shfl_xor(sx, off, 64); sy += __shfl_xor(sy, off, 64);
            x0 = min(x0, __shfl_xor(x0, off, 64)); y0 = min(y0, __shfl_xor(y0, off, 64));
            x1 = max(x1, __shfl_xor(x1, off, 64)); y1 = max(y1, __shfl_xor(y1, off, 64));
        }
        if ((threadIdx.x & 63) == 0) {
            bl_obsblob_t* b = blobs + first;
            atomicAdd((unsigned long long*)&b->sum_x, sx); atomicAdd((unsigned long long*)&b->sum_y, sy);
            atomicAdd(&b->area, a);
            atomicMin(&b->x0, x0); atomicMin(&b->y0, y0); atomicMax(&b->x1, x1); atomicMax(&b->y1, y1);
        }
    } else if (rank >= 0) {
        bl_obsblob_t* b = blobs + rank;
        atomicAdd((unsigned long long*)&b->sum_x, (unsigned long long)x); atomicAdd((unsigned long long*)&b->sum_y, (unsigned long long)y);
        atomicAdd(&b->area, 1);
        atomicMin(&b->x0, x); atomicMin(&b->y0, y); atomicMax(&b->x1, x); atomicMax(&b->y1, y);
    }
}

// d2 of a track's prediction and a blob's centroid when it is within the gate (g = 256 * gate_cells), else -1.  Both differences are
// checked against g first, so the squares stay below 2^29 whatever the positions are.
__device__ __forceinline__ long long obt_d2(int2 p, int2 c, long long g)
{
    const long long dx = (long long)c.x - (long long)p.x, dy = (long long)c.y - (long long)p.y;
    if (dx > g || dx < -g || dy > g || dy < -g) return -1ll;
    const long long d2 = dx * dx + dy * dy;
    return d2 <= g * g ? d2 : -1ll;
}

__device__ __forceinline__ int obt_clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

__global__ __launch_bounds__(OBT_ASSOC_WG) void k_obt_assoc(int* __restrict__ hdr, bl_obsblob_t* __restrict__ blobs, bl_obstrack_t* __restrict__ tracks,
                                                            int32_t* __restrict__ label, bl_obstracks_params_t p)
{
    __shared__ bl_obstrack_t s_tr[BL_OBSTRACKS_MAX_TRACKS];            // 14 KB: the slots, worked on here and written back at the end
    __shared__ int2 s_c[BL_OBSTRACKS_MAX_BLOBS];                       // 8 KB: centroids
    __shared__ int2 s_pred[BL_OBSTRACKS_MAX_TRACKS];                   // 2 KB: predictions
    __shared__ int s_bfree[BL_OBSTRACKS_MAX_BLOBS], s_bbest[BL_OBSTRACKS_MAX_BLOBS], s_btrack[BL_OBSTRACKS_MAX_BLOBS];
    __shared__ int s_tfree[BL_OBSTRACKS_MAX_TRACKS], s_tbest[BL_OBSTRACKS_MAX_TRACKS], s_tmatch[BL_OBSTRACKS_MAX_TRACKS];
    __shared__ int s_slot_of[BL_OBSTRACKS_MAX_TRACKS];
    __shared__ int s_acc, s_matched, s_deleted, s_eligible, s_ntracks, s_nconf, s_nb, s_unborn, s_refused;
    const int t = threadIdx.x, lane = t & 63;
    const int L = hdr[OBT_L];
    const bool too_many = L > BL_OBSTRACKS_MAX_CELLS;
    const int kept = too_many ? 0 : hdr[OBT_KEPT];
    const long long g = 256ll * (long long)p.gate_cells;
    if (t == 0) { s_acc = 0; s_matched = 0; s_deleted = 0; s_eligible = 0; s_ntracks = 0; s_nconf = 0; s_nb = 0; s_unborn = 0; s_refused = too_many ? BL_OBSTRACKS_REFUSED_CELLS : 0; }
    if (t < BL_OBSTRACKS_MAX_TRACKS) {
        const bl_obstrack_t tr = tracks[t];
        s_tr[t] = tr;
        s_pred[t] = make_int2(tr.px + tr.vx, tr.py + tr.vy);
        s_tfree[t] = tr.id != 0u ? 1 : 0;
        s_tmatch[t] = -1;
    }
    __syncthreads();
    {   // a blob per thread: centroid and eligibility
        int el = 0;
        if (t < kept) {
            const bl_obsblob_t b = blobs[t];
            const long long A = (long long)b.area;
            s_c[t] = make_int2((int)((256ll * b.sum_x) / A) + 128, (int)((256ll * b.sum_y) / A) + 128);   // the sums are >= 0
            el = (b.area >= p.min_cells && b.area <= p.max_cells) ? 1 : 0;
            if (el) atomicAdd(&s_eligible, 1);
        }
        s_bfree[t] = el;
        s_btrack[t] = -1;
    }
    __syncthreads();
    // ---- rounds of mutual best.  (d2, i, j) is a strict total order of the pairs, so the least pair among the free ends is both its
    // track's best and its blob's best: every round with a candidate left accepts at least that one, and what a round accepts is what
    // the sorted greedy walk accepts.
    int rounds = 0;
    for (;;) {
        {   // a free track's least (d2, j): four lanes per track, blobs j = sub, sub + 4, ...
            const int i = t >> 2, sub = t & 3;
            long long bd = LLONG_MAX; int bj = INT_MAX;
            if (s_tfree[i]) {
                const int2 pr = s_pred[i];
                for (int j = sub; j < kept; j += 4) {
                    if (!s_bfree[j]) continue;
                    const long long d2 = obt_d2(pr, s_c[j], g);
                    if (d2 >= 0 && (d2 < bd || (d2 == bd && j < bj))) { bd = d2; bj = j; }
                }
            }
            for (int off = 1; off <= 2; off <<= 1) {
                const long long od = __shfl_xor(bd, off, 64); const int oj = __shfl_xor(bj, off, 64);
                if (od < bd || (od == bd && oj < bj)) { bd = od; bj = oj; }
            }
            if (sub == 0) s_tbest[i] = bj == INT_MAX ? -1 : bj;
        }
        {   // a free blob's least (d2, i)
            int bi = -1;
            if (t < kept && s_bfree[t]) {
                long long bd = LLONG_MAX;
                const int2 c = s_c[t];
                for (int i = 0; i < BL_OBSTRACKS_MAX_TRACKS; ++i) {
                    if (!s_tfree[i]) continue;
                    const long long d2 = obt_d2(s_pred[i], c, g);
                    if (d2 >= 0 && d2 < bd) { bd = d2; bi = i; }       // ascending i: the first of equals stays
                }
            }
            s_bbest[t] = bi;
        }
        __syncthreads();
        if (t < BL_OBSTRACKS_MAX_TRACKS) {
            const int j = s_tbest[t];
            if (j >= 0 && s_bbest[j] == t) {
                s_tmatch[t] = j; s_tfree[t] = 0; s_bfree[j] = 0; s_btrack[j] = t;
                atomicAdd(&s_matched, 1);
                s_acc = 1;
            }
        }
        __syncthreads();
        const int acc = s_acc;
        __syncthreads();
        if (!acc) break;
        if (t == 0) s_acc = 0;
        ++rounds;
        __syncthreads();
    }
    // ---- the transition of the occupied slots
    if (t < BL_OBSTRACKS_MAX_TRACKS && s_tr[t].id != 0u) {
        bl_obstrack_t tr = s_tr[t];
        const int2 pr = s_pred[t];
        const int j = s_tmatch[t];
        if (j >= 0) {
            const bl_obsblob_t b = blobs[j];
            const int rx = s_c[j].x - pr.x, ry = s_c[j].y - pr.y;       // within the gate: |r| <= 16384
            tr.px = pr.x + ((p.alpha * rx) >> 8); tr.py = pr.y + ((p.alpha * ry) >> 8);   // >> of a negative int: floor
            tr.vx = obt_clampi(tr.vx + ((p.beta * rx) >> 8), -OBT_VMAX, OBT_VMAX);
            tr.vy = obt_clampi(tr.vy + ((p.beta * ry) >> 8), -OBT_VMAX, OBT_VMAX);
            tr.hits = min(tr.hits + 1, OBT_SAT); tr.missed = 0;
            tr.area = b.area; tr.x0 = b.x0; tr.y0 = b.y0; tr.x1 = b.x1; tr.y1 = b.y1;
            tr.flags = BL_OBSTRACK_MATCHED;
        } else {
            tr.px = pr.x; tr.py = pr.y;
            tr.missed = min(tr.missed + 1, OBT_SAT);
            tr.flags = 0;
            if (tr.missed > p.max_missed) { memset(&tr, 0, sizeof(tr)); atomicAdd(&s_deleted, 1); }
        }
        s_tr[t] = tr;
    }
    __syncthreads();
    // ---- births, one wave: the k-th unmatched eligible blob by rank takes the k-th free slot
    if (t < 64) {
        int nfree = 0;
        for (int base = 0; base < BL_OBSTRACKS_MAX_TRACKS; base += 64) {
            const bool fr = s_tr[base + lane].id == 0u;
            const unsigned long long m = __ballot(fr);
            if (fr) s_slot_of[nfree + __popcll(m & ((1ull << lane) - 1ull))] = base + lane;
            nfree += __popcll(m);
        }
        int wanted = 0;
        for (int base = 0; base < kept; base += 64) {
            const int j = base + lane;
            const bool w = j < kept && s_bfree[j] != 0;
            const unsigned long long m = __ballot(w);
            if (w) s_bbest[j] = wanted + __popcll(m & ((1ull << lane) - 1ull));   // the blob's place among the births
            wanted += __popcll(m);
        }
        if (lane == 0) {
            const int nb = min(wanted, nfree);
            const unsigned long long next_id = (unsigned long long)(unsigned int)hdr[OBT_NEXT_ID];
            s_nb = nb; s_unborn = wanted - nb;
            if (!too_many && nb > 0 && next_id + (unsigned long long)nb - 1ull >= 0xffffffffull) s_refused = BL_OBSTRACKS_REFUSED_IDS;
        }
    }
    __syncthreads();
    const int refused = s_refused;
    if (refused) {                                                      // the slots and the id counter stay; no blobs, no labels
        if (t < BL_OBSTRACKS_MAX_TRACKS) {
            const bl_obstrack_t tr = tracks[t];
            if (tr.id != 0u) { atomicAdd(&s_ntracks, 1); if (tr.flags & BL_OBSTRACK_CONFIRMED) atomicAdd(&s_nconf, 1); }
        }
        for (int i = t; i < min(L, BL_OBSTRACKS_MAX_CELLS); i += OBT_ASSOC_WG) label[i] = -1;
        __syncthreads();
        if (t == 0) {
            hdr[OBT_BLOBS] = 0; hdr[OBT_KEPT] = 0; hdr[OBT_ELIGIBLE] = 0; hdr[OBT_MATCHED] = 0; hdr[OBT_BORN] = 0; hdr[OBT_DELETED] = 0;
            hdr[OBT_UNBORN] = 0; hdr[OBT_TRACKS] = s_ntracks; hdr[OBT_CONFIRMED] = s_nconf; hdr[OBT_REFUSED] = refused; hdr[OBT_ROUNDS] = 0;
        }
        return;
    }
    const int nb = s_nb;
    const unsigned int next_id = (unsigned int)hdr[OBT_NEXT_ID];
    if (t < kept && s_bfree[t] && s_bbest[t] < nb) {
        const int k = s_bbest[t], slot = s_slot_of[k];
        const bl_obsblob_t b = blobs[t];
        bl_obstrack_t tr;
        tr.id = next_id + (unsigned int)k;
        tr.px = s_c[t].x; tr.py = s_c[t].y; tr.vx = 0; tr.vy = 0; tr.hits = 1; tr.missed = 0;
        tr.area = b.area; tr.x0 = b.x0; tr.y0 = b.y0; tr.x1 = b.x1; tr.y1 = b.y1;
        tr.flags = BL_OBSTRACK_BORN; tr.slot = slot;
        s_tr[slot] = tr;
        s_btrack[t] = slot;
    }
    __syncthreads();
    if (t < BL_OBSTRACKS_MAX_TRACKS) {
        bl_obstrack_t tr = s_tr[t];
        tr.slot = t;
        if (tr.id != 0u) {
            if (tr.hits >= p.confirm_hits) tr.flags |= BL_OBSTRACK_CONFIRMED;
            if (tr.vx * tr.vx + tr.vy * tr.vy >= p.min_speed * p.min_speed) tr.flags |= BL_OBSTRACK_MOVING;
            atomicAdd(&s_ntracks, 1);
            if (tr.flags & BL_OBSTRACK_CONFIRMED) atomicAdd(&s_nconf, 1);
        }
        tracks[t] = tr;
    }
    if (t < kept) {
        bl_obsblob_t* b = blobs + t;
        b->cx = s_c[t].x; b->cy = s_c[t].y;
        b->eligible = (b->area >= p.min_cells && b->area <= p.max_cells) ? 1 : 0;
        b->track = s_btrack[t];
    }
    __syncthreads();
    if (t == 0) {
        hdr[OBT_ELIGIBLE] = s_eligible; hdr[OBT_MATCHED] = s_matched; hdr[OBT_BORN] = nb; hdr[OBT_DELETED] = s_deleted; hdr[OBT_UNBORN] = s_unborn;
        hdr[OBT_TRACKS] = s_ntracks; hdr[OBT_CONFIRMED] = s_nconf; hdr[OBT_REFUSED] = 0; hdr[OBT_ROUNDS] = rounds;
        hdr[OBT_NEXT_ID] = (int)(next_id + (unsigned int)nb);
    }
}

// a thread per (live cell, sub-step), taken in strides by a grid of OBT_SWEEP_BLOCKS workgroups whatever the list's length is (the
// host does not know it): item k is sub-step k / L + 1 of live cell k % L, so neighbouring lanes read neighbouring cells
__global__ __launch_bounds__(OBT_WG) void k_obt_sweep(const int* __restrict__ hdr, const int32_t* __restrict__ xy, const int32_t* __restrict__ label,
                                                      const bl_obsblob_t* __restrict__ blobs, const bl_obstrack_t* __restrict__ tracks,
                                                      int8_t* __restrict__ out, int W, int H, bl_obstracks_compose_t cc)
{
    const int L = hdr[OBT_L];
    if (hdr[OBT_KEPT] == 0 || L > BL_OBSTRACKS_MAX_CELLS) return;
    const int items = L * 4 * cc.horizon;                               // <= 65536 * 256
    for (int k = (int)blockIdx.x * OBT_WG + (int)threadIdx.x; k < items; k += OBT_SWEEP_BLOCKS * OBT_WG) {
        const int s = k / L + 1, i = k - (s - 1) * L;                   // s <= 256, |v| <= 1023: s * v fits easily
        const int rk = label[i];
        if (rk < 0) continue;
        const int slot = blobs[rk].track;
        if (slot < 0) continue;
        const bl_obstrack_t tr = tracks[slot];
        if ((tr.flags & (BL_OBSTRACK_CONFIRMED | BL_OBSTRACK_MOVING)) != (BL_OBSTRACK_CONFIRMED | BL_OBSTRACK_MOVING)) continue;
        const int sx = xy[2 * i] + ((s * tr.vx + 512) >> 10), sy = xy[2 * i + 1] + ((s * tr.vy + 512) >> 10);
        if (sx < 0 || sx >= W || sy < 0 || sy >= H) continue;
        if (cc.keep_clear >= 0 && abs(sx - cc.robot_x) <= cc.keep_clear && abs(sy - cc.robot_y) <= cc.keep_clear) continue;   // (no overflow: see the host)
        out[(size_t)sy * W + sx] = (int8_t)127;
    }
}

// (compose_static, after the layer's own k_obs_compose) a thread per live cell of the last update: where its blob is a confirmed moving
// track's -- k_obt_sweep's predicate -- the cell takes the map's value back
__global__ __launch_bounds__(OBT_WG) void k_obt_static(const int* __restrict__ hdr, const int32_t* __restrict__ xy, const int32_t* __restrict__ label,
                                                       const bl_obsblob_t* __restrict__ blobs, const bl_obstrack_t* __restrict__ tracks,
                                                       const int8_t* __restrict__ map, int8_t* __restrict__ out, int W)
{
    const int L = hdr[OBT_L];
    const int i = (int)blockIdx.x * OBT_WG + (int)threadIdx.x;
    if (hdr[OBT_KEPT] == 0 || L > BL_OBSTRACKS_MAX_CELLS || i >= L) return;
    const int rk = label[i];
    if (rk < 0) return;
    const int slot = blobs[rk].track;
    if (slot < 0) return;
    if ((tracks[slot].flags & (BL_OBSTRACK_CONFIRMED | BL_OBSTRACK_MOVING)) != (BL_OBSTRACK_CONFIRMED | BL_OBSTRACK_MOVING)) return;
    const size_t c = (size_t)xy[2 * i + 1] * W + xy[2 * i];
    out[c] = map[c];
}

// ---------------------------------------------------------------------------------------------------------------- host
struct bl_obstracks {
    bl_ctx* ctx;
    int W, H;
    bl_obstracks_params_t params; bool have_params;
    uint32_t last_n; bool fresh;
    int* d_hdr;
    int32_t* d_xy; int32_t* d_label;
    unsigned int* d_parent; int* d_cellrank;
    bl_obsblob_t* d_blobs; bl_obstrack_t* d_tracks;
    bool updated, composed;
    hipEvent_t ev_ua, ev_ub, ev_ca, ev_cb;
};

// no tracks, no blobs, ids from next_id (on the stream)
static int obt_clear(bl_obstracks* tr, uint32_t next_id)
{
    int hdr[OBT_HDR_WORDS];
    memset(hdr, 0, sizeof(hdr));
    hdr[OBT_NEXT_ID] = (int)next_id;
    BL_HIP(hipMemsetAsync(tr->d_tracks, 0, BL_OBSTRACKS_MAX_TRACKS * sizeof(bl_obstrack_t), tr->ctx->stream));
    BL_HIP(hipMemcpyAsync(tr->d_hdr, hdr, sizeof(hdr), hipMemcpyHostToDevice, tr->ctx->stream));
    BL_HIP(hipStreamSynchronize(tr->ctx->stream));                      // hdr is this frame's
    return BL_OK;
}

extern "C" int bl_obstracks_create(bl_ctx* ctx, int width, int height, bl_obstracks** out)
{
    BL_CHECK_ARG(ctx != nullptr && out != nullptr);
    BL_CHECK_ARG(width >= 1 && height >= 1 && (long long)width * height < (1ll << 31));
    BL_HIP(hipSetDevice(ctx->device));
    bl_obstracks* tr = new bl_obstracks();
    memset((void*)tr, 0, sizeof(*tr));
    tr->ctx = ctx; tr->W = width; tr->H = height; tr->fresh = true;
    const size_t cells = (size_t)width * height;
    hipError_t e = hipMalloc((void**)&tr->d_hdr, OBT_HDR_WORDS * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void**)&tr->d_xy, 2 * (size_t)BL_OBSTRACKS_MAX_CELLS * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&tr->d_label, (size_t)BL_OBSTRACKS_MAX_CELLS * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&tr->d_parent, cells * sizeof(unsigned int));
    if (e == hipSuccess) e = hipMalloc((void**)&tr->d_cellrank, cells * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void**)&tr->d_blobs, BL_OBSTRACKS_MAX_BLOBS * sizeof(bl_obsblob_t));
    if (e == hipSuccess) e = hipMalloc((void**)&tr->d_tracks, BL_OBSTRACKS_MAX_TRACKS * sizeof(bl_obstrack_t));
    if (e == hipSuccess) e = hipEventCreate(&tr->ev_ua);
    if (e == hipSuccess) e = hipEventCreate(&tr->ev_ub);
    if (e == hipSuccess) e = hipEventCreate(&tr->ev_ca);
    if (e == hipSuccess) e = hipEventCreate(&tr->ev_cb);
    if (e != hipSuccess) {
        bl_set_error("bl_obstracks_create: %s", hipGetErrorString(e));
        bl_obstracks_destroy(tr);
        return BL_ERR_HIP;
    }
    const int rc = obt_clear(tr, 1u);
    if (rc) { bl_obstracks_destroy(tr); return rc; }
    *out = tr;
    return BL_OK;
}

extern "C" void bl_obstracks_destroy(bl_obstracks* tr)
{
    if (!tr) return;
    (void)hipSetDevice(tr->ctx->device);
    (void)hipStreamSynchronize(tr->ctx->stream);
    if (tr->d_hdr) (void)hipFree(tr->d_hdr);
    if (tr->d_xy) (void)hipFree(tr->d_xy);
    if (tr->d_label) (void)hipFree(tr->d_label);
    if (tr->d_parent) (void)hipFree(tr->d_parent);
    if (tr->d_cellrank) (void)hipFree(tr->d_cellrank);
    if (tr->d_blobs) (void)hipFree(tr->d_blobs);
    if (tr->d_tracks) (void)hipFree(tr->d_tracks);
    if (tr->ev_ua) (void)hipEventDestroy(tr->ev_ua);
    if (tr->ev_ub) (void)hipEventDestroy(tr->ev_ub);
    if (tr->ev_ca) (void)hipEventDestroy(tr->ev_ca);
    if (tr->ev_cb) (void)hipEventDestroy(tr->ev_cb);
    delete tr;
}

extern "C" int bl_obstracks_set_params(bl_obstracks* tr, const bl_obstracks_params_t* p)
{
    BL_CHECK_ARG(tr != nullptr && p != nullptr);
    BL_CHECK_ARG(p->min_cells >= 1 && p->min_cells <= BL_OBSTRACKS_MAX_CELLS);
    BL_CHECK_ARG(p->max_cells >= p->min_cells && p->max_cells <= BL_OBSTRACKS_MAX_CELLS);
    BL_CHECK_ARG(p->gate_cells >= 1 && p->gate_cells <= 64);
    BL_CHECK_ARG(p->alpha >= 0 && p->alpha <= 256 && p->beta >= 0 && p->beta <= 256);
    BL_CHECK_ARG(p->confirm_hits >= 1 && p->confirm_hits <= 255);
    BL_CHECK_ARG(p->max_missed >= 0 && p->max_missed <= 255);
    BL_CHECK_ARG(p->min_speed >= 0 && p->min_speed <= OBT_VMAX);
    tr->params = *p;
    tr->have_params = true;
    return BL_OK;
}

static int obt_need_params(const bl_obstracks* tr, const bl_obslayer* ol)
{
    if (tr->have_params && ol->have_params) return BL_OK;
    bl_set_error(tr->have_params ? "obstacle layer has no parameters (bl_obslayer_set_params first)"
                                 : "obstacle tracks have no parameters (bl_obstracks_set_params first)");
    return BL_ERR_STATE;
}

extern "C" int bl_obstracks_reset(bl_obstracks* tr)
{
    BL_CHECK_ARG(tr != nullptr);
    BL_HIP(hipSetDevice(tr->ctx->device));
    const int rc = obt_clear(tr, 1u);
    if (rc) return rc;
    tr->last_n = 0; tr->fresh = true;
    return BL_OK;
}

extern "C" int bl_obstracks_update(bl_obstracks* tr, bl_obslayer* ol)
{
    BL_CHECK_ARG(tr != nullptr && ol != nullptr);
    BL_CHECK_ARG(ol->ctx == tr->ctx && ol->W == tr->W && ol->H == tr->H);
    int rc = obt_need_params(tr, ol);
    if (rc) return rc;
    if (!tr->fresh && ol->n != tr->last_n + 1u) {
        bl_set_error("bl_obstracks_update: the layer is at update %u, the tracks at %u (one bl_obstracks_update after each bl_obslayer_update; "
                     "bl_obstracks_reset after the layer's reset or upload)", ol->n, tr->last_n);
        return BL_ERR_STATE;
    }
    bl_ctx* ctx = tr->ctx;
    BL_HIP(hipSetDevice(ctx->device));
    obs_live_rule q;
    q.n = ol->n; q.ttl = (uint32_t)ol->params.ttl_scans; q.min_hits = (uint32_t)ol->params.min_hits;
    tr->updated = false;                                                // (the events pair up again once all of this is enqueued)
    BL_HIP(hipEventRecord(tr->ev_ua, ctx->stream));
    rc = obs_live_list_enqueue(ol, tr->d_xy, BL_OBSTRACKS_MAX_CELLS);
    if (rc) return rc;
    hipLaunchKernelGGL(k_obt_init, dim3(OBT_BLOCKS), dim3(OBT_WG), 0, ctx->stream, (const int*)ol->d_totals, tr->d_hdr, (const int32_t*)tr->d_xy,
                       tr->d_parent, tr->d_blobs, tr->W);
    hipLaunchKernelGGL(k_obt_link, dim3(OBT_BLOCKS), dim3(OBT_WG), 0, ctx->stream, (const int*)tr->d_hdr, (const int32_t*)tr->d_xy, tr->d_parent,
                       (const uint8_t*)ol->d_count, (const uint32_t*)ol->d_last, tr->W, tr->H, q);
    hipLaunchKernelGGL(k_obt_rank, dim3(1), dim3(OBT_ASSOC_WG), 0, ctx->stream, tr->d_hdr, (const int32_t*)tr->d_xy, (const unsigned int*)tr->d_parent,
                       tr->d_cellrank, tr->d_blobs, tr->W);
    hipLaunchKernelGGL(k_obt_fold, dim3(OBT_BLOCKS), dim3(OBT_WG), 0, ctx->stream, (const int*)tr->d_hdr, (const int32_t*)tr->d_xy, tr->d_parent,
                       (const int*)tr->d_cellrank, tr->d_blobs, tr->d_label, tr->W, tr->H);
    hipLaunchKernelGGL(k_obt_assoc, dim3(1), dim3(OBT_ASSOC_WG), 0, ctx->stream, tr->d_hdr, tr->d_blobs, tr->d_tracks, tr->d_label, tr->params);
    BL_HIP(hipGetLastError());
    BL_HIP(hipEventRecord(tr->ev_ub, ctx->stream));
    tr->last_n = ol->n; tr->fresh = false; tr->updated = true;          // enqueued: only now is the update accepted
    return BL_OK;
}

extern "C" int bl_obstracks_compose(bl_obstracks* tr, bl_obslayer* ol, const bl_grid* map, bl_grid* out, const bl_obstracks_compose_t* c)
{
    BL_CHECK_ARG(tr != nullptr && ol != nullptr && c != nullptr);
    BL_CHECK_ARG(ol->ctx == tr->ctx && ol->W == tr->W && ol->H == tr->H);
    BL_CHECK_ARG(c->horizon >= 0 && c->horizon <= BL_OBSTRACKS_MAX_HORIZON);
    BL_CHECK_ARG(c->keep_clear >= -1 && c->keep_clear <= BL_OBSTRACKS_MAX_KEEP_CLEAR);
    int rc = obt_need_params(tr, ol);
    if (rc) return rc;
    if (c->horizon > 0 && !tr->fresh && ol->n != tr->last_n) {
        bl_set_error("bl_obstracks_compose: the layer is at update %u, the tracks at %u", ol->n, tr->last_n);
        return BL_ERR_STATE;
    }
    bl_ctx* ctx = tr->ctx;
    BL_HIP(hipSetDevice(ctx->device));
    tr->composed = false;                                               // (as in the update: a start without its end is not read)
    BL_HIP(hipEventRecord(tr->ev_ca, ctx->stream));
    rc = bl_obslayer_compose(ol, map, out);                             // the checks of map and out, the lineage, the mirror, the copy
    if (rc) return rc;
    if (c->horizon > 0) {
        bl_obstracks_compose_t cc = *c;
        // a robot cell far outside the grid clears nothing; brought near, so that the kernel's differences cannot overflow
        if (cc.keep_clear >= 0 && (cc.robot_x < -1024 || cc.robot_x > tr->W + 1024 || cc.robot_y < -1024 || cc.robot_y > tr->H + 1024)) cc.keep_clear = -1;
        hipLaunchKernelGGL(k_obt_sweep, dim3(OBT_SWEEP_BLOCKS), dim3(OBT_WG), 0, ctx->stream, (const int*)tr->d_hdr,
                           (const int32_t*)tr->d_xy, (const int32_t*)tr->d_label, (const bl_obsblob_t*)tr->d_blobs, (const bl_obstrack_t*)tr->d_tracks,
                           out->cells, tr->W, tr->H, cc);
        BL_HIP(hipGetLastError());
    }
    BL_HIP(hipEventRecord(tr->ev_cb, ctx->stream));
    tr->composed = true;
    return BL_OK;
}

extern "C" int bl_obstracks_compose_static(bl_obstracks* tr, bl_obslayer* ol, const bl_grid* map, bl_grid* out)
{
    BL_CHECK_ARG(tr != nullptr && ol != nullptr);
    BL_CHECK_ARG(ol->ctx == tr->ctx && ol->W == tr->W && ol->H == tr->H);
    int rc = obt_need_params(tr, ol);
    if (rc) return rc;
    if (!tr->fresh && ol->n != tr->last_n) {
        bl_set_error("bl_obstracks_compose_static: the layer is at update %u, the tracks at %u", ol->n, tr->last_n);
        return BL_ERR_STATE;
    }
    bl_ctx* ctx = tr->ctx;
    BL_HIP(hipSetDevice(ctx->device));
    tr->composed = false;
    BL_HIP(hipEventRecord(tr->ev_ca, ctx->stream));
    rc = bl_obslayer_compose(ol, map, out);                             // the checks of map and out, the lineage, the mirror, the copy
    if (rc) return rc;
    hipLaunchKernelGGL(k_obt_static, dim3(OBT_BLOCKS), dim3(OBT_WG), 0, ctx->stream, (const int*)tr->d_hdr, (const int32_t*)tr->d_xy,
                       (const int32_t*)tr->d_label, (const bl_obsblob_t*)tr->d_blobs, (const bl_obstrack_t*)tr->d_tracks, (const int8_t*)map->cells,
                       out->cells, tr->W);
    BL_HIP(hipGetLastError());
    BL_HIP(hipEventRecord(tr->ev_cb, ctx->stream));
    tr->composed = true;
    return BL_OK;
}

void bl_obstracks_view_host(const bl_obstracks* tr, bl_obstracks_view* out)
{
    out->ctx = tr->ctx; out->W = tr->W; out->H = tr->H; out->have_params = tr->have_params; out->d_slots = tr->d_tracks;
}

static int obt_hdr(bl_obstracks* tr, int hdr[OBT_HDR_WORDS])
{
    BL_HIP(hipSetDevice(tr->ctx->device));
    BL_HIP(hipMemcpyAsync(hdr, tr->d_hdr, OBT_HDR_WORDS * sizeof(int), hipMemcpyDeviceToHost, tr->ctx->stream));
    BL_HIP(hipStreamSynchronize(tr->ctx->stream));
    return BL_OK;
}

extern "C" int bl_obstracks_tracks(bl_obstracks* tr, bl_obstrack_t* out, int cap, int* count)
{
    BL_CHECK_ARG(tr != nullptr && count != nullptr && cap >= 0 && (cap == 0 || out != nullptr));
    BL_HIP(hipSetDevice(tr->ctx->device));
    std::vector<bl_obstrack_t> all(BL_OBSTRACKS_MAX_TRACKS);
    BL_HIP(hipMemcpyAsync(all.data(), tr->d_tracks, all.size() * sizeof(bl_obstrack_t), hipMemcpyDeviceToHost, tr->ctx->stream));
    BL_HIP(hipStreamSynchronize(tr->ctx->stream));
    int m = 0;
    for (int i = 0; i < BL_OBSTRACKS_MAX_TRACKS; ++i) {
        if (all[(size_t)i].id == 0u) continue;
        if (m < cap) { out[m] = all[(size_t)i]; out[m].slot = i; }
        ++m;
    }
    *count = m;
    return BL_OK;
}

extern "C" int bl_obstracks_blobs(bl_obstracks* tr, bl_obsblob_t* out, int cap, int* count)
{
    BL_CHECK_ARG(tr != nullptr && count != nullptr && cap >= 0 && (cap == 0 || out != nullptr));
    int hdr[OBT_HDR_WORDS];
    const int rc = obt_hdr(tr, hdr);
    if (rc) return rc;
    *count = hdr[OBT_KEPT];
    const int m = hdr[OBT_KEPT] < cap ? hdr[OBT_KEPT] : cap;
    if (m <= 0) return BL_OK;
    BL_HIP(hipMemcpyAsync(out, tr->d_blobs, (size_t)m * sizeof(bl_obsblob_t), hipMemcpyDeviceToHost, tr->ctx->stream));
    BL_HIP(hipStreamSynchronize(tr->ctx->stream));
    return BL_OK;
}

extern "C" int bl_obstracks_labels(bl_obstracks* tr, int32_t* out, int cap, int* count)
{
    BL_CHECK_ARG(tr != nullptr && count != nullptr && cap >= 0 && (cap == 0 || out != nullptr));
    int hdr[OBT_HDR_WORDS];
    const int rc = obt_hdr(tr, hdr);
    if (rc) return rc;
    const int L = hdr[OBT_L] < BL_OBSTRACKS_MAX_CELLS ? hdr[OBT_L] : BL_OBSTRACKS_MAX_CELLS;
    *count = L;
    const int m = L < cap ? L : cap;
    if (m <= 0) return BL_OK;
    BL_HIP(hipMemcpyAsync(out, tr->d_label, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, tr->ctx->stream));
    BL_HIP(hipStreamSynchronize(tr->ctx->stream));
    return BL_OK;
}

extern "C" int bl_obstracks_stats(bl_obstracks* tr, bl_obstracks_stats_t* out)
{
    BL_CHECK_ARG(tr != nullptr && out != nullptr);
    int hdr[OBT_HDR_WORDS];
    const int rc = obt_hdr(tr, hdr);
    if (rc) return rc;
    memset(out, 0, sizeof(*out));
    out->n = tr->last_n; out->next_id = (uint32_t)hdr[OBT_NEXT_ID];
    out->live_cells = hdr[OBT_L];
    out->blobs = hdr[OBT_BLOBS]; out->eligible = hdr[OBT_ELIGIBLE]; out->dropped = hdr[OBT_BLOBS] - hdr[OBT_KEPT];
    out->matched = hdr[OBT_MATCHED]; out->born = hdr[OBT_BORN]; out->deleted = hdr[OBT_DELETED]; out->unborn = hdr[OBT_UNBORN];
    out->tracks = hdr[OBT_TRACKS]; out->confirmed = hdr[OBT_CONFIRMED]; out->refused = hdr[OBT_REFUSED]; out->rounds = hdr[OBT_ROUNDS];
    return BL_OK;
}

extern "C" int bl_obstracks_download(bl_obstracks* tr, bl_obstrack_t* slots, bl_obstracks_state_t* state)
{
    BL_CHECK_ARG(tr != nullptr);
    int hdr[OBT_HDR_WORDS];
    const int rc = obt_hdr(tr, hdr);
    if (rc) return rc;
    if (slots) {
        BL_HIP(hipMemcpyAsync(slots, tr->d_tracks, BL_OBSTRACKS_MAX_TRACKS * sizeof(bl_obstrack_t), hipMemcpyDeviceToHost, tr->ctx->stream));
        BL_HIP(hipStreamSynchronize(tr->ctx->stream));
    }
    if (state) { state->n = tr->last_n; state->next_id = (uint32_t)hdr[OBT_NEXT_ID]; state->fresh = tr->fresh ? 1 : 0; state->reserved = 0; }
    return BL_OK;
}

extern "C" int bl_obstracks_upload(bl_obstracks* tr, const bl_obstrack_t* slots, const bl_obstracks_state_t* state)
{
    BL_CHECK_ARG(tr != nullptr && slots != nullptr && state != nullptr);
    BL_CHECK_ARG(state->next_id >= 1u);
    std::vector<bl_obstrack_t> all(BL_OBSTRACKS_MAX_TRACKS);
    int ntracks = 0, nconf = 0;
    for (int i = 0; i < BL_OBSTRACKS_MAX_TRACKS; ++i) {
        bl_obstrack_t t = slots[i];
        if (t.id == 0u) memset(&t, 0, sizeof(t));
        else {
            BL_CHECK_ARG(t.id < state->next_id);
            for (int k = 0; k < i; ++k) BL_CHECK_ARG(slots[k].id != t.id);
            BL_CHECK_ARG(t.vx >= -OBT_VMAX && t.vx <= OBT_VMAX && t.vy >= -OBT_VMAX && t.vy <= OBT_VMAX);
            BL_CHECK_ARG(t.px >= -OBT_POS_MAX && t.px <= OBT_POS_MAX && t.py >= -OBT_POS_MAX && t.py <= OBT_POS_MAX);
            BL_CHECK_ARG(t.hits >= 1 && t.hits <= OBT_SAT && t.missed >= 0 && t.missed <= 255);
            ++ntracks; nconf += (t.flags & BL_OBSTRACK_CONFIRMED) ? 1 : 0;
        }
        t.slot = i;
        all[(size_t)i] = t;
    }
    BL_HIP(hipSetDevice(tr->ctx->device));
    int hdr[OBT_HDR_WORDS];
    memset(hdr, 0, sizeof(hdr));
    hdr[OBT_NEXT_ID] = (int)state->next_id; hdr[OBT_TRACKS] = ntracks; hdr[OBT_CONFIRMED] = nconf;
    BL_HIP(hipMemcpyAsync(tr->d_tracks, all.data(), all.size() * sizeof(bl_obstrack_t), hipMemcpyHostToDevice, tr->ctx->stream));
    BL_HIP(hipMemcpyAsync(tr->d_hdr, hdr, sizeof(hdr), hipMemcpyHostToDevice, tr->ctx->stream));
    BL_HIP(hipStreamSynchronize(tr->ctx->stream));
    tr->last_n = state->n; tr->fresh = state->fresh != 0;
    return BL_OK;
}

extern "C" int bl_obstracks_last_device_ms(const bl_obstracks* tr, float* update_ms, float* compose_ms)
{
    BL_CHECK_ARG(tr != nullptr);
    if ((update_ms && !tr->updated) || (compose_ms && !tr->composed)) {
        bl_set_error("bl_obstracks_last_device_ms: no %s yet", (update_ms && !tr->updated) ? "bl_obstracks_update" : "bl_obstracks_compose");
        return BL_ERR_STATE;
    }
    if (update_ms) {
        BL_HIP(hipEventSynchronize(tr->ev_ub));
        BL_HIP(hipEventElapsedTime(update_ms, tr->ev_ua, tr->ev_ub));
    }
    if (compose_ms) {
        BL_HIP(hipEventSynchronize(tr->ev_cb));
        BL_HIP(hipEventElapsedTime(compose_ms, tr->ev_ca, tr->ev_cb));
    }
    return BL_OK;
}
