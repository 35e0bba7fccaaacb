// bl_shortcut.hip -- path shortcutting (include/botlab_hip.h, "path shortcutting"): any-angle waypoints from grid paths.  No
// reference counterpart; the definition in the header is the contract and tests/path_shortcut_model.py restates it.
//
//   k_sc_visible  vis[path][j][bit j - i] = (i, j) is an edge.  A workgroup belongs to one path and stages the ok bits of the path's
//                 bounding box in LDS (STAGED), rows padded to 32 bits; its waves then take items (j, g): one j and the 64 spans
//                 s = 64 g .. 64 g + 63, lane l the pair (j - s, j).  Every lane of a wave starts on cell j, so the first reads are
//                 broadcasts, and the spans of a wave differ by less than 64, so the walks end together.  The 64 answers are one
//                 ballot, written by one lane: no two waves share a word, no atomics.
//   k_sc_dp       a workgroup per path: cost[] and pred[] in LDS, j serial, the threads take the i of the window; the least key
//                 (cost, i) by wave shuffles and one LDS hop; the last thread walks pred and writes the kept indices ascending.
#include <math.h>
#include <string.h>

#include "bl_internal.h"

#define SC_VIS_THREADS 256
#define SC_COST_NONE 0x7FFFFFFFFFFFFFFFll
#define SC_RED_BYTES 128               // k_sc_dp: per wave a key cost (8) and a key i (4), up to 4 waves; then the input cost's partial sums
#define SC_VIS_CAP_WORDS (32ull << 20) // 64-bit words of vis a launch pair may use (256 MiB): longer calls go in several batches of paths

struct sc_args {
    const uint16_t* l1; const uint8_t* oktab; int table_n;
    int W, H;
    const int2* xy;                    // all paths' cells
    const int32_t* offsets;            // [P + 1]
    const unsigned long long* voff;    // [P] first vis word of a path, relative to this batch's buffer
    const int4* bbox;                  // [P] x0, y0, bw, bh of a path's cells
    unsigned long long* vis;
    int max_span;
    int G;                             // 64-bit words per vis row: spans 0 .. 64 G - 1
    int bpp;                           // workgroups per path (k_sc_visible)
    int p0;                            // first path of this batch
    int waypoint_cost;
    int32_t* keep; int32_t* counts; long long* cost;
};

template <bool STAGED>
__device__ __forceinline__ bool sc_ok(const sc_args& a, const uint32_t* s_win, int x0, int y0, int pitch_w, int x, int y)
{
    if (STAGED) {
        const int ux = x - x0, uy = y - y0;
        return (s_win[uy * pitch_w + (ux >> 5)] >> (ux & 31)) & 1u;
    }
    const int n = a.l1[(size_t)y * a.W + x];
    return n != 0xFFFF && n < a.table_n && a.oktab[n] != 0;
}

// every cell of cover(a, b) is ok.  Major axis t = 0 .. A, minor w = 0 .. B (B <= A), both counted from a towards b: the cell (t, w)
// is covered iff 2 |t B - w A| <= A + B.  e = t B - w0 A is carried with 0 <= e < A (as Bresenham carries its error), and only
// w0 - 1, w0, w0 + 1 can pass; the bounding box is 0 <= w <= B.
template <bool STAGED>
__device__ __forceinline__ bool sc_walk(const sc_args& a, const uint32_t* s_win, int x0, int y0, int pitch_w, int xa, int ya, int xb, int yb)
{
    const int DX = xb - xa, DY = yb - ya;
    const int adx = abs(DX), ady = abs(DY);
    const bool xmajor = adx >= ady;
    const int A = xmajor ? adx : ady, B = xmajor ? ady : adx;
    const int sx = DX < 0 ? -1 : 1, sy = DY < 0 ? -1 : 1;
    const int st = xmajor ? sx : sy, sw = xmajor ? sy : sx;          // steps of the major and the minor coordinate
    int mt = xmajor ? xa : ya;                                       // major coordinate of the walk
    const int mw0 = xmajor ? ya : xa;
    const int lim = A + B;
    int e = 0, w0 = 0;
    for (int t = 0; t <= A; ++t) {
        for (int k = -1; k <= 1; ++k) {
            const int w = w0 + k;
            if (w < 0 || w > B) continue;
            if (2 * abs(e - k * A) > lim) continue;
            const int mw = mw0 + sw * w;
            if (!sc_ok<STAGED>(a, s_win, x0, y0, pitch_w, xmajor ? mt : mw, xmajor ? mw : mt)) return false;
        }
        mt += st;
        e += B;
        if (e >= A && A > 0) { e -= A; ++w0; }
    }
    return true;
}

template <bool STAGED>
__global__ __launch_bounds__(SC_VIS_THREADS) void k_sc_visible(sc_args a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    uint32_t* s_win = (uint32_t*)s_raw;
    const int p = a.p0 + blockIdx.x / a.bpp, blk = blockIdx.x % a.bpp;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int off = a.offsets[p], m = a.offsets[p + 1] - off;
    const int items = m * a.G;
    if (blk * (SC_VIS_THREADS / 64) >= items) return;                // uniform over the workgroup: nothing to do, nothing staged
    const int4 bb = a.bbox[p];
    const int pitch_w = (bb.z + 31) >> 5;
    if (STAGED) {
        // a thread per cell of the padded window, 64 cells of one row pair per ballot
        const int cells = pitch_w * 32 * bb.w;
        for (int base = 0; base < cells; base += SC_VIS_THREADS) {
            const int idx = base + tid;
            bool bit = false;
            if (idx < cells) {
                const int ux = idx % (pitch_w * 32), uy = idx / (pitch_w * 32);
                if (ux < bb.z) bit = sc_ok<false>(a, nullptr, 0, 0, 0, bb.x + ux, bb.y + uy);
            }
            const unsigned long long b = __ballot(bit);
            const int w = (base + (tid & ~63)) >> 5;                 // the wave's first word (even)
            if (lane == 0 && (w << 5) < cells) {
                s_win[w] = (uint32_t)b;
                if (((w + 1) << 5) < cells) s_win[w + 1] = (uint32_t)(b >> 32);
            }
        }
        __syncthreads();
    }
    const int2* xy = a.xy + off;
    unsigned long long* vis = a.vis + a.voff[p - a.p0];
    for (int item = blk * (SC_VIS_THREADS / 64) + wave; item < items; item += a.bpp * (SC_VIS_THREADS / 64)) {
        const int j = item / a.G, g = item - j * a.G;
        const int s = g * 64 + lane;
        bool edge = s >= 1 && s <= a.max_span && s <= j;
        if (edge && s > 1) {
            const int2 cj = xy[j], ci = xy[j - s];
            edge = sc_walk<STAGED>(a, s_win, bb.x, bb.y, pitch_w, cj.x, cj.y, ci.x, ci.y);
        }
        const unsigned long long b = __ballot(edge);
        if (lane == 0) vis[(size_t)j * a.G + g] = b;
    }
}

// floor(sqrt(2^20 (dx^2 + dy^2))): the double root of an exactly represented argument, put right by integer compares
__device__ __forceinline__ long long sc_length(int dx, int dy)
{
    const long long A = ((long long)dx * dx + (long long)dy * dy) << 20;
    long long r = (long long)sqrt((double)A);
    while (r * r > A) --r;
    while ((r + 1) * (r + 1) <= A) ++r;
    return r;
}

__device__ __forceinline__ bool sc_key_less(long long ca, int ia, long long cb, int ib) { return ca < cb || (ca == cb && ia < ib); }

__global__ __launch_bounds__(256) void k_sc_dp(sc_args a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    const int p = a.p0 + blockIdx.x;
    const int off = a.offsets[p], m = a.offsets[p + 1] - off;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, T = blockDim.x, nw = T >> 6;
    long long* s_rc = (long long*)s_raw;                             // [4] per-wave key cost
    int* s_ri = (int*)(s_raw + 32);                                  // [4] per-wave key i
    long long* s_sum = (long long*)(s_raw + 64);                     // [4] per-wave partial sums of the input cost
    long long* s_cost = (long long*)(s_raw + SC_RED_BYTES);          // [m]
    uint16_t* s_pred = (uint16_t*)(s_raw + SC_RED_BYTES + (size_t)((m + 1) & ~1) * 8);   // [m]
    if (m <= 1) {
        if (tid == 0) {
            a.counts[p] = m;
            if (m == 1) a.keep[off] = 0;
            a.cost[2 * (size_t)p] = 0; a.cost[2 * (size_t)p + 1] = 0;
        }
        return;
    }
    const int2* xy = a.xy + off;
    const unsigned long long* vis = a.vis + a.voff[p - a.p0];
    // the input path's own cost
    long long sum = 0;
    for (int i = tid; i + 1 < m; i += T) {
        const int2 c0 = xy[i], c1 = xy[i + 1];
        sum += sc_length(c1.x - c0.x, c1.y - c0.y) + a.waypoint_cost;
    }
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if (lane == 0) s_sum[wave] = sum;
    if (tid == 0) { s_cost[0] = 0; s_pred[0] = 0; }
    __syncthreads();
    for (int j = 1; j < m; ++j) {
        const int2 cj = xy[j];
        const int smax = min(a.max_span, j);
        long long best = SC_COST_NONE;
        int bi = 0x7FFFFFFF;
        for (int s = 1 + tid; s <= smax; s += T) {
            if (!((vis[(size_t)j * a.G + (s >> 6)] >> (s & 63)) & 1ull)) continue;
            const int i = j - s;
            const int2 ci = xy[i];
            const long long c = s_cost[i] + sc_length(cj.x - ci.x, cj.y - ci.y) + a.waypoint_cost;
            if (sc_key_less(c, i, best, bi)) { best = c; bi = i; }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const long long oc = __shfl_xor(best, o);
            const int oi = __shfl_xor(bi, o);
            if (sc_key_less(oc, oi, best, bi)) { best = oc; bi = oi; }
        }
        if (nw > 1) {
            if (lane == 0) { s_rc[wave] = best; s_ri[wave] = bi; }
            __syncthreads();
            if (tid == 0)
                for (int w = 1; w < nw; ++w)
                    if (sc_key_less(s_rc[w], s_ri[w], best, bi)) { best = s_rc[w]; bi = s_ri[w]; }
        }
        if (tid == 0) { s_cost[j] = best; s_pred[j] = (uint16_t)bi; }
        __syncthreads();
    }
    if (tid == T - 1) {
        int n = 1;
        for (int k = m - 1; k > 0; k = s_pred[k]) ++n;
        int32_t* keep = a.keep + off;
        int q = n - 1;
        for (int k = m - 1; k > 0; k = s_pred[k]) keep[q--] = k;
        keep[0] = 0;
        a.counts[p] = n;
        long long in_cost = 0;
        for (int w = 0; w < nw; ++w) in_cost += s_sum[w];
        a.cost[2 * (size_t)p] = s_cost[m - 1];
        a.cost[2 * (size_t)p + 1] = in_cost;
    }
}

// ---------------------------------------------------------------------------------------------------------------- host
struct bl_shortcut {
    bl_ctx* ctx;
    bl_shortcut_params_t params; bool have_params;
    void* d_in; size_t d_in_cap;                  // bounding boxes | cells | vis offsets | offsets | ok table
    void* h_in; size_t h_in_cap;                  // pinned
    void* d_out; size_t d_out_cap;                // costs | counts | kept indices
    void* h_out; size_t h_out_cap;                // pinned
    void* d_vis; size_t d_vis_cap;
    std::vector<hipEvent_t>* ev;                  // ev[0], then per batch: after k_sc_visible, after k_sc_dp
    int ev_used;
    int last_path; bool timed; float last_ms, last_ms_visible;
};

static int sc_event(bl_shortcut* sc, int k, hipEvent_t* out)
{
    while ((int)sc->ev->size() <= k) {
        hipEvent_t e;
        BL_HIP(hipEventCreate(&e));
        sc->ev->push_back(e);
    }
    *out = (*sc->ev)[(size_t)k];
    return BL_OK;
}

extern "C" int bl_shortcut_create(bl_ctx* ctx, bl_shortcut** out)
{
    BL_CHECK_ARG(ctx != nullptr && out != nullptr);
    BL_HIP(hipSetDevice(ctx->device));
    bl_shortcut* sc = new bl_shortcut();
    memset((void*)sc, 0, sizeof(*sc));
    sc->ctx = ctx;
    sc->last_path = -1;
    sc->ev = new std::vector<hipEvent_t>();
    *out = sc;
    return BL_OK;
}

extern "C" void bl_shortcut_destroy(bl_shortcut* sc)
{
    if (!sc) return;
    (void)hipSetDevice(sc->ctx->device);
    (void)hipStreamSynchronize(sc->ctx->stream);
    if (sc->d_in) (void)hipFree(sc->d_in);
    if (sc->d_out) (void)hipFree(sc->d_out);
    if (sc->d_vis) (void)hipFree(sc->d_vis);
    if (sc->h_in) (void)hipHostFree(sc->h_in);
    if (sc->h_out) (void)hipHostFree(sc->h_out);
    for (hipEvent_t e : *sc->ev) (void)hipEventDestroy(e);
    delete sc->ev;
    delete sc;
}

extern "C" int bl_shortcut_set_params(bl_shortcut* sc, const bl_shortcut_params_t* p)
{
    BL_CHECK_ARG(sc != nullptr && p != nullptr);
    BL_CHECK_ARG(isfinite(p->clearance));
    BL_CHECK_ARG(p->max_span >= 1 && p->max_span <= BL_SHORTCUT_MAX_POINTS);
    BL_CHECK_ARG(p->waypoint_cost >= 0 && p->waypoint_cost <= BL_SHORTCUT_MAX_WAYPOINT_COST);
    sc->params = *p;
    sc->have_params = true;
    return BL_OK;
}

// The launches of one call: the paths in batches whose vis fits SC_VIS_CAP_WORDS (one batch, unless the paths are very many and very
// long).  Results land in sc->h_out (costs | counts | kept indices) after the one synchronisation.  vis_out: the vis rows of the single
// path (bl_shortcut_debug_visible; k_sc_dp is not launched), *G_out words a row.
static int sc_run(bl_shortcut* sc, const bl_dist* dist, const int32_t* xy, const int32_t* offsets, int P, std::vector<unsigned long long>* vis_out,
                  int* G_out)
{
    BL_CHECK_ARG(sc != nullptr && dist != nullptr);
    if (!sc->have_params) { bl_set_error("path shortcut has no parameters (bl_shortcut_set_params first)"); return BL_ERR_STATE; }
    BL_CHECK_ARG(P >= 0 && P <= BL_SHORTCUT_MAX_PATHS && offsets != nullptr);
    BL_CHECK_ARG(offsets[0] == 0);
    for (int p = 0; p < P; ++p) BL_CHECK_ARG(offsets[p + 1] >= offsets[p] && offsets[p + 1] - offsets[p] <= BL_SHORTCUT_MAX_POINTS);
    const int N = offsets[P];
    BL_CHECK_ARG(N == 0 || xy != nullptr);
    bl_ctx* ctx = sc->ctx;
    bl_dist_host_view v;
    int rc = bl_dist_view_host(dist, &v);
    if (rc) return rc;
    BL_CHECK_ARG(v.ctx == ctx);
    const int W = v.frame.width, H = v.frame.height, ln = v.table_n;
    for (int k = 0; k < N; ++k) BL_CHECK_ARG(xy[2 * k] >= 0 && xy[2 * k] < W && xy[2 * k + 1] >= 0 && xy[2 * k + 1] < H);
    BL_HIP(hipSetDevice(ctx->device));

    int max_m = 0;
    for (int p = 0; p < P; ++p) max_m = offsets[p + 1] - offsets[p] > max_m ? offsets[p + 1] - offsets[p] : max_m;
    int S = sc->params.max_span < max_m - 1 ? sc->params.max_span : max_m - 1;
    if (S < 1) S = 1;
    const int G = S / 64 + 1;
    // the input block: bounding boxes | cells | vis offsets | offsets | ok table; the output block: costs | counts | kept indices
    const size_t o_xy = (size_t)P * 16, o_voff = o_xy + (size_t)N * 8, o_off = o_voff + (size_t)P * 8;
    const size_t o_ok = o_off + (((size_t)(P + 1) * 4 + 7) & ~(size_t)7);
    const size_t in_bytes = o_ok + (size_t)ln;
    const size_t o_counts = (size_t)P * 16, o_keep = o_counts + (((size_t)P * 4 + 7) & ~(size_t)7);
    const size_t out_bytes = o_keep + (size_t)N * 4;
    rc = bl_grow(&sc->d_in, &sc->d_in_cap, in_bytes, false, ctx);
    if (!rc) rc = bl_grow(&sc->h_in, &sc->h_in_cap, in_bytes, true, ctx);
    if (!rc) rc = bl_grow(&sc->d_out, &sc->d_out_cap, out_bytes + 8, false, ctx);
    if (!rc) rc = bl_grow(&sc->h_out, &sc->h_out_cap, out_bytes + 8, true, ctx);
    if (rc) return rc;
    char* h = (char*)sc->h_in;
    if (N) memcpy(h + o_xy, xy, (size_t)N * 8);
    memcpy(h + o_off, offsets, (size_t)(P + 1) * 4);
    unsigned long long* h_voff = (unsigned long long*)(h + o_voff);
    int32_t* h_bbox = (int32_t*)h;
    uint8_t* h_ok = (uint8_t*)(h + o_ok);
    for (int n = 0; n < ln; ++n) h_ok[n] = bl_search_traversable(v.lut_host[n], sc->params.clearance) ? 1 : 0;   // the field's rule, by the field's code
    // bounding boxes, the window rule, the batches
    bool staged = true;
    size_t win_bytes = 0;
    std::vector<int> batch_first(1, 0);
    unsigned long long words = 0, max_words = 0;
    int max_items = 0;
    for (int p = 0; p < P; ++p) {
        const int m = offsets[p + 1] - offsets[p];
        int x0 = 0, y0 = 0, x1 = -1, y1 = -1;
        for (int k = offsets[p]; k < offsets[p + 1]; ++k) {
            const int x = xy[2 * k], y = xy[2 * k + 1];
            if (k == offsets[p]) { x0 = x1 = x; y0 = y1 = y; }
            x0 = x < x0 ? x : x0; x1 = x > x1 ? x : x1; y0 = y < y0 ? y : y0; y1 = y > y1 ? y : y1;
        }
        const int bw = x1 - x0 + 1, bh = y1 - y0 + 1;
        h_bbox[4 * p] = x0; h_bbox[4 * p + 1] = y0; h_bbox[4 * p + 2] = bw; h_bbox[4 * p + 3] = bh;
        if (m > 0) {
            const size_t wb = (size_t)((bw + 31) / 32 * 4) * bh;
            if (wb > (size_t)BL_SHORTCUT_WINDOW_BYTES) staged = false;
            if (wb > win_bytes) win_bytes = wb;
        }
        const unsigned long long need = (unsigned long long)m * G;
        if (words + need > SC_VIS_CAP_WORDS && words > 0) { batch_first.push_back(p); words = 0; }
        h_voff[p] = words;
        words += need;
        if (words > max_words) max_words = words;
        if (m * G > max_items) max_items = m * G;
    }
    batch_first.push_back(P);
    rc = bl_grow(&sc->d_vis, &sc->d_vis_cap, (size_t)(max_words ? max_words : 1) * 8, false, ctx);
    if (rc) return rc;
    BL_HIP(hipMemcpyAsync(sc->d_in, sc->h_in, in_bytes, hipMemcpyHostToDevice, ctx->stream));

    sc_args a;
    memset((void*)&a, 0, sizeof(a));
    a.l1 = v.l1; a.oktab = (const uint8_t*)((char*)sc->d_in + o_ok); a.table_n = ln;
    a.W = W; a.H = H;
    a.xy = (const int2*)((char*)sc->d_in + o_xy);
    a.offsets = (const int32_t*)((char*)sc->d_in + o_off);
    a.bbox = (const int4*)sc->d_in;
    a.vis = (unsigned long long*)sc->d_vis;
    a.max_span = sc->params.max_span; a.G = G;
    a.waypoint_cost = sc->params.waypoint_cost;
    a.cost = (long long*)sc->d_out; a.counts = (int32_t*)((char*)sc->d_out + o_counts); a.keep = (int32_t*)((char*)sc->d_out + o_keep);
    int bpp = (max_items + 127) / 128;                               // about 128 items a wave at the most, 128 workgroups a path
    a.bpp = bpp < 1 ? 1 : bpp > 128 ? 128 : bpp;
    const size_t vis_lds = staged ? ((win_bytes + 15) & ~(size_t)15) : 0;
    const int dp_threads = S <= 64 ? 64 : 256;
    const size_t dp_lds = SC_RED_BYTES + (size_t)((max_m + 1) & ~1) * 8 + (((size_t)max_m * 2 + 15) & ~(size_t)15);
    if (staged) BL_DYN_LDS_ONCE_PER_DEVICE(k_sc_visible<true>, BL_SHORTCUT_WINDOW_BYTES, ctx);
    BL_DYN_LDS_ONCE_PER_DEVICE(k_sc_dp, SC_RED_BYTES + BL_SHORTCUT_MAX_POINTS * 10 + 16, ctx);

    hipEvent_t e;
    int nev = 0;
    rc = sc_event(sc, nev++, &e);
    if (rc) return rc;
    BL_HIP(hipEventRecord(e, ctx->stream));
    for (size_t b = 0; b + 1 < batch_first.size(); ++b) {
        const int p0 = batch_first[b], np = batch_first[b + 1] - p0;
        if (np == 0) continue;
        a.p0 = p0;
        a.voff = (const unsigned long long*)((char*)sc->d_in + o_voff) + p0;
        if (staged) hipLaunchKernelGGL(k_sc_visible<true>, dim3((unsigned int)(np * a.bpp)), dim3(SC_VIS_THREADS), vis_lds, ctx->stream, a);
        else hipLaunchKernelGGL(k_sc_visible<false>, dim3((unsigned int)(np * a.bpp)), dim3(SC_VIS_THREADS), 0, ctx->stream, a);
        BL_HIP(hipGetLastError());
        sc->last_path = staged ? 0 : 1;
        rc = sc_event(sc, nev++, &e);
        if (rc) return rc;
        BL_HIP(hipEventRecord(e, ctx->stream));
        if (!vis_out) {
            hipLaunchKernelGGL(k_sc_dp, dim3((unsigned int)np), dim3(dp_threads), dp_lds, ctx->stream, a);
            BL_HIP(hipGetLastError());
        }
        rc = sc_event(sc, nev++, &e);
        if (rc) return rc;
        BL_HIP(hipEventRecord(e, ctx->stream));
    }
    if (vis_out) {
        vis_out->assign((size_t)max_words, 0ull);
        if (max_words) BL_HIP(hipMemcpyAsync(vis_out->data(), sc->d_vis, (size_t)max_words * 8, hipMemcpyDeviceToHost, ctx->stream));
        *G_out = G;
    } else if (out_bytes) {
        BL_HIP(hipMemcpyAsync(sc->h_out, sc->d_out, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    }
    BL_HIP(hipStreamSynchronize(ctx->stream));
    if (!vis_out) {
        sc->last_ms = 0.0f; sc->last_ms_visible = 0.0f;
        if (nev > 1) {
            BL_HIP(hipEventElapsedTime(&sc->last_ms, (*sc->ev)[0], (*sc->ev)[(size_t)nev - 1]));
            for (int k = 1; k < nev; k += 2) {
                float ms = 0.0f;
                BL_HIP(hipEventElapsedTime(&ms, (*sc->ev)[(size_t)k - 1], (*sc->ev)[(size_t)k]));
                sc->last_ms_visible += ms;
            }
        }
        sc->timed = true;
    }
    return BL_OK;
}

extern "C" int bl_shortcut_cells(bl_shortcut* sc, const bl_dist* dist, const int32_t* xy, const int32_t* offsets, int P, int32_t* out_keep,
                                 int32_t* out_counts, int64_t* out_cost)
{
    BL_CHECK_ARG(P <= 0 || (out_keep != nullptr && out_counts != nullptr && out_cost != nullptr));
    int rc = sc_run(sc, dist, xy, offsets, P, nullptr, nullptr);
    if (rc) return rc;
    const size_t o_counts = (size_t)P * 16, o_keep = o_counts + (((size_t)P * 4 + 7) & ~(size_t)7);
    const char* h = (const char*)sc->h_out;
    const int32_t* counts = (const int32_t*)(h + o_counts);
    for (int p = 0; p < P; ++p) {
        out_counts[p] = counts[p];
        memcpy(out_keep + offsets[p], h + o_keep + (size_t)offsets[p] * 4, (size_t)counts[p] * 4);
    }
    if (P) memcpy(out_cost, h, (size_t)P * 16);
    return BL_OK;
}

extern "C" int bl_shortcut_poses(bl_shortcut* sc, const bl_dist* dist, const bl_pose_xyt_t* paths, int cap_each, const int* lens, int P,
                                 bl_pose_xyt_t* out_paths, int* out_lens, int64_t* out_cost)
{
    BL_CHECK_ARG(sc != nullptr && dist != nullptr);
    BL_CHECK_ARG(P >= 0 && P <= BL_SHORTCUT_MAX_PATHS && cap_each >= 0);
    BL_CHECK_ARG(P == 0 || (paths != nullptr && lens != nullptr && out_paths != nullptr && out_lens != nullptr));
    bl_dist_host_view v;
    int rc = bl_dist_view_host(dist, &v);
    if (rc) return rc;
    std::vector<int32_t> offsets((size_t)P + 1, 0), xy;
    for (int p = 0; p < P; ++p) {
        BL_CHECK_ARG(lens[p] >= 0 && lens[p] <= cap_each && lens[p] <= BL_SHORTCUT_MAX_POINTS);
        offsets[(size_t)p + 1] = offsets[(size_t)p] + lens[p];
        for (int k = 0; k < lens[p]; ++k) {
            const bl_pose_xyt_t& q = paths[(size_t)p * cap_each + k];
            // global_position_to_grid_cell, inside the grid by bl_navfield_paths' test of a start pose
            const double vx = ((double)q.x - (double)v.frame.ox) * (double)v.frame.cpm, vy = ((double)q.y - (double)v.frame.oy) * (double)v.frame.cpm;
            BL_CHECK_ARG(vx > -1.0 && vx < (double)v.frame.width && vy > -1.0 && vy < (double)v.frame.height);
            xy.push_back((int)vx); xy.push_back((int)vy);
        }
    }
    rc = sc_run(sc, dist, xy.data(), offsets.data(), P, nullptr, nullptr);
    if (rc) return rc;
    const size_t o_counts = (size_t)P * 16, o_keep = o_counts + (((size_t)P * 4 + 7) & ~(size_t)7);
    const char* h = (const char*)sc->h_out;
    const int32_t* keep = (const int32_t*)(h + o_keep);
    const int32_t* counts = (const int32_t*)(h + o_counts);
    for (int p = 0; p < P; ++p) {
        const int32_t* kp = keep + offsets[(size_t)p];
        const int32_t* cell = xy.data() + 2 * (size_t)offsets[(size_t)p];
        out_lens[p] = counts[p];
        for (int s = 0; s < counts[p]; ++s) {
            bl_pose_xyt_t q = paths[(size_t)p * cap_each + kp[s]];
            if (s >= 1) {
                const int dx = cell[2 * kp[s]] - cell[2 * kp[s - 1]], dy = cell[2 * kp[s] + 1] - cell[2 * kp[s - 1] + 1];
                if (dx != 0 || dy != 0) q.theta = (float)atan2((double)dy, (double)dx);
            }
            out_paths[(size_t)p * cap_each + s] = q;
        }
    }
    if (out_cost && P) memcpy(out_cost, h, (size_t)P * 16);
    return BL_OK;
}

extern "C" int bl_shortcut_debug_visible(bl_shortcut* sc, const bl_dist* dist, const int32_t* xy, int m, uint8_t* out)
{
    BL_CHECK_ARG(m >= 0 && m <= 512 && (m == 0 || out != nullptr));
    const int32_t offsets[2] = {0, m};
    std::vector<unsigned long long> vis;
    int G = 1;
    int rc = sc_run(sc, dist, xy, offsets, 1, &vis, &G);
    if (rc) return rc;
    for (int j = 0; j < m; ++j)
        for (int i = 0; i < m; ++i) {
            const int s = j - i;
            out[(size_t)j * m + i] = (s >= 1 && s < 64 * G && ((vis[(size_t)j * G + (s >> 6)] >> (s & 63)) & 1ull)) ? 1 : 0;
        }
    return BL_OK;
}

extern "C" int bl_shortcut_debug_path(const bl_shortcut* sc) { return sc ? sc->last_path : -1; }

extern "C" int bl_shortcut_last_device_ms(const bl_shortcut* sc, float* ms, float* ms_visible)
{
    BL_CHECK_ARG(sc != nullptr && ms != nullptr);
    if (!sc->timed) { bl_set_error("bl_shortcut_last_device_ms: no bl_shortcut_cells yet"); return BL_ERR_STATE; }
    *ms = sc->last_ms;
    if (ms_visible) *ms_visible = sc->last_ms_visible;
    return BL_OK;
}
