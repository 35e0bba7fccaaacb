// Pose hypotheses of the particle cloud: bl_pf_clusters (definition: include/botlab_hip.h).  Included by bl_mcl.hip.
//
// The launches of one call, all on the ctx stream, nothing between them but the stream's order:
//   memset           the key table (twice as many slots as particles, a power of two) and the two counters
//   k_pfc_bins<0>    every workgroup removes the duplicate bins of its PFC_PER_WG particles in an LDS table (k_kld_count's pattern and
//                    63-bit key) and inserts its distinct keys into the global open-addressing table; the thread whose CAS claimed a
//                    slot takes the next dense bin id and writes that bin's record (key, zero sums, parent = itself)
//   k_pfc_bins<1>    the same LDS table again, now with 64-bit LDS accumulators per distinct bin (512 terms below 2^52 each cannot
//                    pass 2^62), relative to the bin's corner; one 128-bit atomic add per sum and distinct bin goes to the bin's
//                    record, whose dense id every slot now shows (the launch boundary lies between a slot's first writer and its readers)
//   k_pfc_link       one thread per bin probes its 13 forward neighbours in the table and unites: lock-free union-find that hooks
//                    the larger root under the smaller with one CAS (parent[i] <= i always: every walk is strictly decreasing and
//                    so bounded by the bin count), path halving on the way
//   k_pfc_roots      every bin walks to its root and notes it; its sums are shifted from the bin's corner to absolute fine
//                    coordinates, in place; a root takes the next cluster number
//   k_pfc_fold       every bin that is not a root adds its sums to its root's record (128-bit atomic adds; a wave whose bins share a
//                    root adds once) and lowers the root's key to its own with an atomic min: the anchor is the smallest KEY of the
//                    cluster, whichever bin ended up as the root
//   k_pfc_select     one workgroup: K rounds of "the best cluster after the one before" over the cluster list (U descending, anchor
//                    ascending is a total order, so a round needs no marks), the total of the units, and the result record
//   k_pfc_labels     (only when asked for) particle -> bin -> root -> cluster -> rank
// Every integer sum is order-free (wrapping 128-bit adds of terms whose total fits), so the result is the same for any
// arrival order; no loop waits for another workgroup.
#pragma once

#define PFC_WG 256
#define PFC_PER_THREAD 2
#define PFC_PER_WG (PFC_WG * PFC_PER_THREAD)
#define PFC_LDS_SLOTS (2 * PFC_PER_WG)
#define PFC_SEL_WG 1024
#define PFC_OFF 1048576ll                        // 2^20: offset of a position bin index inside the key
#define PFC_NONE 0xffffffffu

// a bin, and after k_pfc_fold (roots only) a cluster: s[] = x, y, xx, yy, xy, cos, sin as (lo, hi)
struct pfc_bin {
    unsigned long long key;                      // packed (ix, iy, it) + 1; a root's: lowered to the cluster's smallest by k_pfc_fold
    unsigned long long count, units;
    unsigned long long s[7][2];
};                                               // 136 bytes

struct pfc_dev {
    unsigned long long* table;                   // [mask + 1]: bin keys (0: empty)
    unsigned int* slot_id;                       // [mask + 1]: dense bin id of an occupied slot
    pfc_bin* bins;                               // [particles]
    unsigned int* parent;                        // [particles] union-find over bin ids
    unsigned int* root;                          // [particles] a bin's root (k_pfc_roots)
    unsigned int* clid;                          // [particles] a root bin's cluster number
    unsigned int* clist;                         // [particles] cluster number -> root bin
    int* rank;                                   // [particles] cluster number -> rank, -1 beyond K
    unsigned int* counters;                      // [0] bins, [1] clusters
    unsigned int mask;
};

struct pfc_part { long long px, py; int it; long long si, ci; unsigned int u; };

__device__ __forceinline__ long long pfc_clamp_floor(double v, double lim)
{
    const double q = floor(v);
    if (!(q >= -lim)) return (long long)-lim;                               // (NaN too)
    if (q > lim - 1.0) return (long long)(lim - 1.0);
    return (long long)q;
}

__device__ __forceinline__ pfc_part pfc_particle(const float4 r, double xy_scale, double th_scale, int T)
{
    pfc_part p;
    p.px = pfc_clamp_floor((double)r.x * xy_scale, 1073741824.0);
    p.py = pfc_clamp_floor((double)r.y * xy_scale, 1073741824.0);
    const long long q = pfc_clamp_floor((double)r.z * th_scale, 1099511627776.0);
    long long it = q % (long long)T;
    if (it < 0) it += T;
    p.it = (int)it;
    float sn = 0.0f, cs = 0.0f;
    if (fabsf(r.z) < 100.0f) bl_sincosf(r.z, &sn, &cs);                     // (false for NaN and the infinities)
    p.si = (long long)rint((double)sn * 1048576.0);
    p.ci = (long long)rint((double)cs * 1048576.0);
    p.u = __float_as_uint(r.w);
    return p;
}

__device__ __forceinline__ unsigned long long pfc_key(long long ix, long long iy, int it)
{
    return (((unsigned long long)(ix + PFC_OFF) << 42) | ((unsigned long long)(iy + PFC_OFF) << 21) | (unsigned long long)it) + 1ull;
}

// slot of a key that the table holds; PFC_NONE if it does not
__device__ __forceinline__ unsigned int pfc_lookup(const pfc_dev& d, unsigned long long key)
{
    unsigned int h = (unsigned int)kld_mix(key) & d.mask;
    for (unsigned int probe = 0; probe <= d.mask; ++probe) {
        const unsigned long long k = d.table[h];
        if (k == key) return h;
        if (k == 0ull) return PFC_NONE;
        h = (h + 1) & d.mask;
    }
    return PFC_NONE;
}

// p[0..1] += v as a 128-bit integer; every carry out of the low limb is added to the high one exactly once, by whoever caused it
__device__ __forceinline__ void pfc_add128(unsigned long long* p, __int128 v)
{
    const unsigned long long lo = (unsigned long long)v;
    unsigned long long hi = (unsigned long long)(v >> 64);
    if (lo != 0ull) {
        const unsigned long long old = atomicAdd(&p[0], lo);
        if (old + lo < old) hi += 1ull;
    }
    if (hi != 0ull) atomicAdd(&p[1], hi);
}

template <int ACC>
__global__ __launch_bounds__(PFC_WG) void k_pfc_bins(const float4* __restrict__ rec, int n, double xy_scale, double th_scale, int T, pfc_dev d)
{
    __shared__ unsigned long long s_key[PFC_LDS_SLOTS];
    __shared__ unsigned int s_lid[ACC ? PFC_LDS_SLOTS : 1];
    __shared__ unsigned long long s_lkey[ACC ? PFC_PER_WG : 1];
    __shared__ unsigned long long s_acc[ACC ? PFC_PER_WG : 1][9];          // count, units, fx, fy, fxx, fyy, fxy, cos, sin
    __shared__ unsigned int s_n;
    const int tid = threadIdx.x;
    for (int i = tid; i < PFC_LDS_SLOTS; i += PFC_WG) s_key[i] = 0ull;
    if (tid == 0) s_n = 0u;
    __syncthreads();
    const int base = blockIdx.x * PFC_PER_WG;
    pfc_part part[PFC_PER_THREAD];
    unsigned int slot[PFC_PER_THREAD];
    for (int r = 0; r < PFC_PER_THREAD; ++r) {
        const int j = base + r * PFC_WG + tid;
        slot[r] = PFC_NONE;
        if (j >= n) continue;
        part[r] = pfc_particle(rec[j], xy_scale, th_scale, T);
        const unsigned long long key = pfc_key(part[r].px >> 10, part[r].py >> 10, part[r].it);
        unsigned int h = (unsigned int)kld_mix(key) & (PFC_LDS_SLOTS - 1);
        for (int probe = 0; probe < PFC_LDS_SLOTS; ++probe) {             // (at most PFC_PER_WG keys in twice as many slots)
            const unsigned long long prev = atomicCAS(&s_key[h], 0ull, key);
            if (prev == 0ull || prev == key) { slot[r] = h; break; }
            h = (h + 1) & (PFC_LDS_SLOTS - 1);
        }
    }
    __syncthreads();
    if constexpr (!ACC) {
        for (int i = tid; i < PFC_LDS_SLOTS; i += PFC_WG) {
            const unsigned long long key = s_key[i];
            if (key == 0ull) continue;
            unsigned int h = (unsigned int)kld_mix(key) & d.mask;
            for (unsigned int probe = 0; probe <= d.mask; ++probe) {
                const unsigned long long prev = atomicCAS(&d.table[h], 0ull, key);
                if (prev == 0ull) {                                         // this thread alone owns the new bin until the launch ends
                    const unsigned int id = atomicAdd(&d.counters[0], 1u);
                    d.slot_id[h] = id;
                    pfc_bin b;
                    memset(&b, 0, sizeof(b));
                    b.key = key;
                    d.bins[id] = b;
                    d.parent[id] = id;
                    break;
                }
                if (prev == key) break;
                h = (h + 1) & d.mask;
            }
        }
    } else {
    // dense local numbers for the distinct bins of this workgroup, their accumulators zeroed
    for (int i = tid; i < PFC_LDS_SLOTS; i += PFC_WG) {
        const unsigned long long key = s_key[i];
        if (key == 0ull) continue;
        const unsigned int lid = atomicAdd(&s_n, 1u);
        s_lid[i] = lid;
        s_lkey[lid] = key;
        for (int k = 0; k < 9; ++k) s_acc[lid][k] = 0ull;
    }
    __syncthreads();
    for (int r = 0; r < PFC_PER_THREAD; ++r) {
        if (slot[r] == PFC_NONE) continue;
        unsigned long long* a = s_acc[s_lid[slot[r]]];
        const pfc_part& p = part[r];
        const unsigned long long u = p.u, fx = (unsigned long long)(p.px & 1023), fy = (unsigned long long)(p.py & 1023);
        atomicAdd(&a[0], 1ull);
        if (u == 0ull) continue;
        atomicAdd(&a[1], u);
        atomicAdd(&a[2], u * fx); atomicAdd(&a[3], u * fy);
        atomicAdd(&a[4], u * fx * fx); atomicAdd(&a[5], u * fy * fy); atomicAdd(&a[6], u * fx * fy);
        atomicAdd(&a[7], (unsigned long long)((long long)u * p.ci)); atomicAdd(&a[8], (unsigned long long)((long long)u * p.si));
    }
    __syncthreads();
    const unsigned int nl = s_n;
    for (unsigned int lid = tid; lid < nl; lid += PFC_WG) {
        const unsigned int h = pfc_lookup(d, s_lkey[lid]);
        if (h == PFC_NONE) continue;                                        // (cannot happen: k_pfc_bins<0> inserted every key)
        pfc_bin* b = d.bins + d.slot_id[h];
        const unsigned long long* a = s_acc[lid];
        atomicAdd(&b->count, a[0]);
        if (a[1] == 0ull) continue;
        atomicAdd(&b->units, a[1]);
        for (int k = 0; k < 5; ++k) pfc_add128(b->s[k], (__int128)a[2 + k]);
        for (int k = 5; k < 7; ++k) pfc_add128(b->s[k], (__int128)(long long)a[2 + k]);
    }
    }
}

__device__ __forceinline__ unsigned int pfc_ld(const unsigned int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// root of x; parent[i] <= i, so the walk takes at most x steps.  Path halving: a bin that is not a root never becomes one again,
// and whatever is stored into its parent word is one of its ancestors.
__device__ __forceinline__ unsigned int pfc_find(unsigned int* parent, unsigned int x, unsigned int nbins, bool halve)
{
    for (unsigned int step = 0; step < nbins; ++step) {
        const unsigned int p = pfc_ld(parent + x);
        if (p == x) return x;
        const unsigned int g = pfc_ld(parent + p);
        if (halve && g != p) __hip_atomic_store(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = g;
    }
    return x;
}

// a failed CAS means that another thread hooked the root this one held, which then finds a smaller one: at most nbins rounds
__device__ __forceinline__ void pfc_unite(unsigned int* parent, unsigned int a, unsigned int b, unsigned int nbins)
{
    for (unsigned int round = 0; round <= nbins; ++round) {
        a = pfc_find(parent, a, nbins, true);
        b = pfc_find(parent, b, nbins, true);
        if (a == b) return;
        if (a < b) { const unsigned int t = a; a = b; b = t; }
        if (atomicCAS(parent + a, a, b) == a) return;
    }
}

__global__ __launch_bounds__(PFC_WG) void k_pfc_link(int T, pfc_dev d)
{
    const unsigned int nbins = d.counters[0];
    const unsigned int id = blockIdx.x * PFC_WG + threadIdx.x;
    if (id >= nbins) return;
    const unsigned long long k = d.bins[id].key - 1ull;
    const long long ix = (long long)(k >> 42) - PFC_OFF, iy = (long long)((k >> 21) & 0x1fffffull) - PFC_OFF;
    const int it = (int)(k & 0x1fffffull);
    // the heading steps that lead to different bins: T = 1 has one heading bin, T = 2 one neighbour on both sides
    const int dt_lo = T >= 3 ? -1 : 0, dt_hi = T >= 2 ? 1 : 0;
    for (int dx = 0; dx <= 1; ++dx)
        for (int dy = dx ? -1 : 0; dy <= 1; ++dy)
            for (int dt = (dx || dy) ? dt_lo : 1; dt <= dt_hi; ++dt) {
                const long long nx = ix + dx, ny = iy + dy;
                if (nx >= PFC_OFF || ny < -PFC_OFF || ny >= PFC_OFF) continue;
                int nt = it + dt;
                if (nt < 0) nt += T;
                if (nt >= T) nt -= T;
                const unsigned int h = pfc_lookup(d, pfc_key(nx, ny, nt));
                if (h != PFC_NONE) pfc_unite(d.parent, id, d.slot_id[h], nbins);
            }
}

__device__ __forceinline__ __int128 pfc_get128(const unsigned long long* p) { return (__int128)(((unsigned __int128)p[1] << 64) | p[0]); }
__device__ __forceinline__ void pfc_put128(unsigned long long* p, __int128 v) { p[0] = (unsigned long long)v; p[1] = (unsigned long long)(v >> 64); }

__global__ __launch_bounds__(PFC_WG) void k_pfc_roots(pfc_dev d)
{
    const unsigned int nbins = d.counters[0];
    const unsigned int id = blockIdx.x * PFC_WG + threadIdx.x;
    if (id >= nbins) return;
    const unsigned int r = pfc_find(d.parent, id, nbins, false);
    d.root[id] = r;
    if (r == id) {
        const unsigned int c = atomicAdd(&d.counters[1], 1u);
        d.clid[id] = c;
        d.clist[c] = id;
        d.rank[c] = -1;
    }
    // from the bin's corner (ax, ay) to absolute fine coordinates: px = ax + fx
    pfc_bin* b = d.bins + id;
    const unsigned long long k = b->key - 1ull;
    const __int128 ax = (__int128)(((long long)(k >> 42) - PFC_OFF) * 1024), ay = (__int128)(((long long)((k >> 21) & 0x1fffffull) - PFC_OFF) * 1024);
    const __int128 U = (__int128)b->units;
    const __int128 fx = pfc_get128(b->s[0]), fy = pfc_get128(b->s[1]), fxx = pfc_get128(b->s[2]), fyy = pfc_get128(b->s[3]), fxy = pfc_get128(b->s[4]);
    pfc_put128(b->s[0], fx + ax * U);
    pfc_put128(b->s[1], fy + ay * U);
    pfc_put128(b->s[2], fxx + 2 * ax * fx + ax * ax * U);
    pfc_put128(b->s[3], fyy + 2 * ay * fy + ay * ay * U);
    pfc_put128(b->s[4], fxy + ax * fy + ay * fx + ax * ay * U);
}

__device__ __forceinline__ unsigned long long pfc_wave_sum_u64(unsigned long long v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// sum of a 128-bit value over the wave (lane 0 holds it): the low limbs in two halves of 32 bits, so that no carry is lost
__device__ __forceinline__ __int128 pfc_wave_sum_128(__int128 v)
{
    const unsigned long long lo = (unsigned long long)v;
    const unsigned long long l0 = pfc_wave_sum_u64(lo & 0xffffffffull), l1 = pfc_wave_sum_u64(lo >> 32);
    const unsigned long long hi = pfc_wave_sum_u64((unsigned long long)(v >> 64));
    return (__int128)(((unsigned __int128)hi << 64) + ((unsigned __int128)l1 << 32) + (unsigned __int128)l0);
}

__global__ __launch_bounds__(PFC_WG) void k_pfc_fold(pfc_dev d)
{
    const unsigned int nbins = d.counters[0];
    const unsigned int id = blockIdx.x * PFC_WG + threadIdx.x;
    const bool live = id < nbins;
    const unsigned int r = live ? d.root[id] : PFC_NONE;
    const bool folds = live && r != id;                                     // (a root's own sums are in place already)
    // a wave whose 64 bins all fold into one root (the one big cluster of a spread-out cloud) adds once
    const unsigned int r0 = __shfl(r, 0, 64);
    const bool same = __builtin_amdgcn_ballot_w64(folds && r == r0) == ~0ull;
    if (same) {
        const pfc_bin* b = d.bins + id;
        pfc_bin* t = d.bins + r0;
        const unsigned long long cnt = pfc_wave_sum_u64(b->count), un = pfc_wave_sum_u64(b->units);
        unsigned long long kmin = b->key;
        for (int off = 32; off > 0; off >>= 1) { const unsigned long long o = __shfl_down(kmin, off, 64); kmin = o < kmin ? o : kmin; }
        __int128 s[7];
        for (int k = 0; k < 7; ++k) s[k] = pfc_wave_sum_128(pfc_get128(b->s[k]));
        if ((threadIdx.x & 63) == 0) {
            atomicAdd(&t->count, cnt);
            atomicAdd(&t->units, un);
            atomicMin(&t->key, kmin);
            for (int k = 0; k < 7; ++k) pfc_add128(t->s[k], s[k]);
        }
        return;
    }
    if (!folds) return;
    const pfc_bin* b = d.bins + id;
    pfc_bin* t = d.bins + r;
    atomicAdd(&t->count, b->count);
    if (b->units != 0ull) atomicAdd(&t->units, b->units);
    atomicMin(&t->key, b->key);
    for (int k = 0; k < 7; ++k) pfc_add128(t->s[k], pfc_get128(b->s[k]));
}

// a before b in the result's order: more units, then the smaller anchor
__device__ __forceinline__ bool pfc_before(unsigned long long ua, unsigned long long ka, unsigned long long ub, unsigned long long kb)
{
    return ua > ub || (ua == ub && ka < kb);
}

__global__ __launch_bounds__(PFC_SEL_WG) void k_pfc_select(int K, int active, pfc_dev d, bl_pf_clusters_t* out)
{
    __shared__ unsigned long long s_u[PFC_SEL_WG], s_k[PFC_SEL_WG];
    __shared__ unsigned int s_c[PFC_SEL_WG];
    const int tid = threadIdx.x;
    const unsigned int C = d.counters[1];
    unsigned long long* words = (unsigned long long*)out;
    for (int i = tid; i < (int)(sizeof(bl_pf_clusters_t) / 8); i += PFC_SEL_WG) words[i] = 0ull;
    // the total of the units
    unsigned long long sum = 0ull;
    for (unsigned int c = tid; c < C; c += PFC_SEL_WG) sum += d.bins[d.clist[c]].units;
    s_u[tid] = sum;
    __syncthreads();
    for (int h = PFC_SEL_WG / 2; h > 0; h >>= 1) {
        if (tid < h) s_u[tid] += s_u[tid + h];
        __syncthreads();
    }
    if (tid == 0) { out->num_clusters = C; out->units_sum = s_u[0]; out->active = active; }
    __syncthreads();
    unsigned long long prev_u = 0ull, prev_k = 0ull;
    const int rounds = (unsigned int)K < C ? K : (int)C;
    for (int round = 0; round < rounds; ++round) {
        unsigned long long bu = 0ull, bk = 0ull;
        unsigned int bc = PFC_NONE;
        for (unsigned int c = tid; c < C; c += PFC_SEL_WG) {
            const pfc_bin* b = d.bins + d.clist[c];
            const unsigned long long u = b->units, k = b->key;
            if (round > 0 && !pfc_before(prev_u, prev_k, u, k)) continue;           // (chosen in an earlier round)
            if (bc == PFC_NONE || pfc_before(u, k, bu, bk)) { bu = u; bk = k; bc = c; }
        }
        s_u[tid] = bu; s_k[tid] = bk; s_c[tid] = bc;
        __syncthreads();
        for (int h = PFC_SEL_WG / 2; h > 0; h >>= 1) {
            if (tid < h && s_c[tid + h] != PFC_NONE && (s_c[tid] == PFC_NONE || pfc_before(s_u[tid + h], s_k[tid + h], s_u[tid], s_k[tid]))) {
                s_u[tid] = s_u[tid + h]; s_k[tid] = s_k[tid + h]; s_c[tid] = s_c[tid + h];
            }
            __syncthreads();
        }
        prev_u = s_u[0]; prev_k = s_k[0];
        const unsigned int c = s_c[0];
        __syncthreads();                                                            // (s_* are rewritten by the next round)
        if (c == PFC_NONE) break;                                                   // (uniform; cannot happen for round < C)
        if (tid == 0) {
            const pfc_bin* b = d.bins + d.clist[c];
            bl_pf_cluster_t* o = out->clusters + round;
            o->count = b->count; o->units = b->units;
            bl_i128_t* sums = &o->sx;
            for (int k = 0; k < 7; ++k) { sums[k].lo = b->s[k][0]; sums[k].hi = (int64_t)b->s[k][1]; }
            const unsigned long long key = b->key - 1ull;
            o->anchor_ix = (int32_t)((long long)(key >> 42) - PFC_OFF);
            o->anchor_iy = (int32_t)((long long)((key >> 21) & 0x1fffffull) - PFC_OFF);
            o->anchor_it = (int32_t)(key & 0x1fffffull);
            d.rank[c] = round;
        }
    }
}

__global__ __launch_bounds__(PFC_WG) void k_pfc_labels(const float4* __restrict__ rec, int n, double xy_scale, double th_scale, int T, pfc_dev d,
                                                       int32_t* __restrict__ labels)
{
    const int j = blockIdx.x * PFC_WG + threadIdx.x;
    if (j >= n) return;
    const pfc_part p = pfc_particle(rec[j], xy_scale, th_scale, T);
    const unsigned int h = pfc_lookup(d, pfc_key(p.px >> 10, p.py >> 10, p.it));
    labels[j] = h == PFC_NONE ? -1 : d.rank[d.clid[d.root[d.slot_id[h]]]];
}
