// bl_mppi.hip -- the sampling local planner (include/botlab_hip.h, "sampling local planner"): model-predictive path-integral control
// over a navigation field.  No reference counterpart; the definition in the header is the contract and tests/mppi_model.py restates it.
// No sequence is stored: a sample's controls are regenerated from Philox and the two `prev` registers of the clamp chain wherever
// they are needed.  Everything compared or summed is an integer, so no launch shape and no reduction order shows in the result.
//
//   k_mppi_rollout  a thread per sample, a workgroup per (state, MP_THREADS consecutive samples): the cost window staged in LDS as
//                   int16 (STAGED, the local planner's window rule with n_steps = T * n_sub) or read from the grids; MOVING: a lane per
//                   tracker slot decides used, the used slots go to LDS in slot order by ballot, and every visited cell is tested
//                   against them at its step.  Writes cost[k] and the workgroup's least (cost, k) key.
//   k_mppi_average  the same grid: the least key over the state's workgroups, the weight by table lookup in LDS, the controls
//                   regenerated, and the 2 T + 2 integer sums of the workgroup by wave shuffles, then LDS, into its slot
//   k_mppi_finish   a workgroup per state: the slots summed, the floor divisions, the clamp chain, the candidate's rollout (one
//                   thread, grids read directly) and the fall-back to the best sample
//   k_mppi_poses    one thread: the poses of a given sequence (bl_mppi_debug_rollout)
//
// Every rule this planner has in common with the arc planner (bl_localplan.hip) is called from bl_localplan_dev.h and stated there
// once.  Here stay the controls (Philox, the clamp chain, Q16), the rollout's loop over periods and sub-steps, the averaging, and
// mp_keep_slots' two barriers around the shared compaction.
#include <math.h>
#include <string.h>

#include "bl_internal.h"
#include "bl_navfield_dev.h"
#include "bl_localplan_dev.h"

#define MP_THREADS 256
#define MP_WAVES (MP_THREADS / 64)
#define MP_RED_BYTES 64                // per wave: key cost (8), key k (4), count (4)
#define MP_KEPT_BYTES (BL_OBSTRACKS_MAX_TRACKS * 20)
#define MP_LDS_FIXED (MP_RED_BYTES + MP_KEPT_BYTES)
#define MP_MAX_SUMS (2 * BL_MPPI_MAX_HORIZON + 2)
static_assert(MP_THREADS == LP_THREADS, "the shared prologue, staging loop and reduction are written for LP_THREADS threads");
static_assert(MP_LDS_FIXED % 16 == 0, "the window starts 16-byte aligned");
static_assert(sizeof(lp_kept) == 20, "MP_KEPT_BYTES");
static_assert(sizeof(bl_mppi_params_t) == 72 && sizeof(bl_mppi_state_t) == 40 && sizeof(bl_mppi_result_t) == 56, "botlab_hip.h states these sizes");

struct mp_args {
    lp_field f;
    const bl_mppi_state_t* states;
    const int32_t* seq_in;                        // [state][T][2], or null: zeros
    int K, T, n_sub, bps;                         // bps: workgroups per state
    int lambda;
    int vmin_q, vmax_q, wmax_q, nv_q, nw_q, av_q, aw_q;
    uint32_t seed_lo, seed_hi;
    lp_partial* partial;                          // [state][bps]
    long long* costs;                             // [state][K]
    long long* sums;                              // [state][bps][2 T + 2]: N of (t, channel), then S and Q
    const uint32_t* wtab;                         // the 257 weights
    int debug;                                    // bl_mppi_debug_samples: rolled out whatever the flags
    int* first_hit; int32_t* seqs;                // debug: per sample; either may be null
    lp_moving m;                                  // MOVING only
};

// one link of the clamp chain
__device__ __forceinline__ int mp_clamp(long long raw, int prev, int lim_lo, int lim_hi, int a_q)
{
    int lo = max(lim_lo, prev - a_q), hi = min(lim_hi, prev + a_q);
    if (lo > hi) lo = hi = min(max(prev, lim_lo), lim_hi);
    return (int)min(max(raw, (long long)lo), (long long)hi);
}

__device__ __forceinline__ void mp_clamp_pair(const mp_args& a, long long rv, long long rw, int& pv, int& pw)
{
    pv = mp_clamp(rv, pv, a.vmin_q, a.vmax_q, a.av_q);
    pw = mp_clamp(rw, pw, -a.wmax_q, a.wmax_q, a.aw_q);
}

__device__ __forceinline__ int mp_irwin_hall(uint32_t x, uint32_t y) { return (int)((x & 0xffffu) + (x >> 16) + (y & 0xffffu) + (y >> 16)) - 131070; }

// the controls of sample k at period t; (pv, pw) the chain's prev on entry and the controls on return
__device__ __forceinline__ void mp_sample_ctrl(const mp_args& a, int state, const bl_mppi_state_t& st, int k, int t, int& pv, int& pw)
{
    long long rv = 0, rw = 0;
    if (a.seq_in) {
        const int32_t* u = a.seq_in + ((size_t)state * a.T + t) * 2;
        rv = u[0]; rw = u[1];
    }
    if (k == 1) { rv = 0; rw = 0; }                                    // brake (K >= 2: sample 0 is the nominal whatever K)
    else if (k > 1) {
        uint32_t o[4];
        bl_philox4x32((uint32_t)k, (uint32_t)t, st.stream, st.tick, a.seed_lo, a.seed_hi, o);
        rv += ((long long)mp_irwin_hall(o[0], o[1]) * a.nv_q) >> 17;   // >> of a negative int64: floor
        rw += ((long long)mp_irwin_hall(o[2], o[3]) * a.nw_q) >> 17;
    }
    mp_clamp_pair(a, rv, rw, pv, pw);
}

__host__ __device__ __forceinline__ int mp_q16(float x) { return (int)lrint((double)x * 65536.0); }

// The rollout of a sequence: ctrl(t, &qv, &qw) hands out the controls of period t, in order.  Returns the cost, LP_COST_NONE when
// inadmissible; *hit_k the first step inside a used box (0: none).  all_steps: every step is looked at for the moving rule.
template <bool STAGED, bool MOVING, class Ctrl>
__device__ __forceinline__ long long mp_rollout(const mp_args& a, const bl_localplan_state_t& st, const int16_t* s_win, int wx0, int wy0,
                                                const lp_kept* s_kept, int kept, bool all_steps, int* hit_k_out, Ctrl ctrl)
{
    const int W = a.f.frame.width, H = a.f.frame.height;
    float x = st.pose.x, y = st.pose.y, theta = bl_wrap_to_pi(st.pose.theta);
    int ex = 0, ey = 0, pen = 0, hit_k = 0, step = 0;
    bool ok = true, done = false;
    for (int t = 0; t < a.T && !done; ++t) {
        int qv, qw;
        ctrl(t, &qv, &qw);
        const float v = (float)qv * 0x1p-16f, w = (float)qw * 0x1p-16f;
        const float s = v * a.f.dt_sim, dth = w * a.f.dt_sim;
        for (int i = 0; i < a.n_sub && !done; ++i) {
            ++step;
            lp_unicycle_step(x, y, theta, s, dth);
            if (!nav_pose_cell(a.f.frame, x, y, &ex, &ey)) { ok = false; done = !all_steps; continue; }
            if (MOVING && hit_k == 0) {
                bool hit = false;
                for (int b = 0; b < kept; ++b) hit = hit || lp_mov_in_box(s_kept[b], step + a.m.mlead, a.m.mq, ex, ey);
                if (hit) { hit_k = step; ok = false; done = !all_steps; continue; }
            }
            if (!ok) continue;                                       // (all_steps: only the moving test is still wanted)
            const int q = lp_cell_cost<STAGED>(a.f, s_win, wx0, wy0, ex, ey);
            if (q < 0) { ok = false; done = !all_steps; continue; }
            pen += q;
        }
    }
    if (hit_k_out) *hit_k_out = hit_k;
    long long score;
    return lp_end_score(a.f, W, H, ok, ex, ey, theta, pen, &score) ? score : LP_COST_NONE;
}

// MOVING: a lane per slot decides used; the used slots compacted in slot order into s_kept.  Returns how many.  All MP_THREADS
// threads of the workgroup call it; s_cnt is MP_WAVES ints.
template <bool MOVING>
__device__ __forceinline__ int mp_keep_slots(const mp_args& a, lp_kept* s_kept, int* s_cnt)
{
    if (!MOVING) return 0;
    const int tid = threadIdx.x;
    const bl_obstrack_t tr = a.m.slots[tid];
    const bool used = lp_mov_used(tr);
    const lp_kept rec = lp_mov_record(tr, a.m.mmargin);
    const unsigned long long mask = __ballot(used);
    if ((tid & 63) == 0) s_cnt[tid >> 6] = __popcll(mask);
    __syncthreads();
    const int kept = lp_mov_compact(s_cnt, mask, used, rec, s_kept);
    __syncthreads();
    return kept;
}

template <bool STAGED, bool MOVING>
__global__ __launch_bounds__(MP_THREADS) void k_mppi_rollout(mp_args a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    long long* s_cost = (long long*)s_raw;
    int* s_k = (int*)(s_raw + 32);
    int* s_n = (int*)(s_raw + 48);
    lp_kept* s_kept = (lp_kept*)(s_raw + MP_RED_BYTES);
    int16_t* s_win = (int16_t*)(s_raw + MP_LDS_FIXED);
    const int state = blockIdx.x / a.bps, blk = blockIdx.x % a.bps;
    const int tid = threadIdx.x;
    const bl_mppi_state_t st = a.states[state];
    if (!a.debug && lp_start_flags(a.f, st.s)) return;                // nothing is drawn (uniform over the workgroup)
    int wx0 = 0, wy0 = 0;
    if (STAGED) {
        lp_window_corner(a.f.frame, st.s.pose, a.f.win_r, &wx0, &wy0);
        lp_stage_window(a.f, s_win, wx0, wy0);
    }
    const int kept = mp_keep_slots<MOVING>(a, s_kept, s_n);
    __syncthreads();
    const int k = blk * MP_THREADS + tid;
    long long cost = LP_COST_NONE;
    int key = 0x7FFFFFFF, adm = 0;
    if (k < a.K) {
        const int pv0 = mp_q16(st.s.v), pw0 = mp_q16(st.s.w);
        int pv = pv0, pw = pw0, hit_k = 0;
        const bool all_steps = MOVING && a.first_hit != nullptr;
        cost = mp_rollout<STAGED, MOVING>(a, st.s, s_win, wx0, wy0, s_kept, kept, all_steps, &hit_k,
                                          [&](int t, int* qv, int* qw) { mp_sample_ctrl(a, state, st, k, t, pv, pw); *qv = pv; *qw = pw; });
        a.costs[(size_t)state * a.K + k] = cost;
        if (all_steps) a.first_hit[k] = hit_k;
        if (a.seqs) {
            pv = pv0; pw = pw0;
            for (int t = 0; t < a.T; ++t) {
                mp_sample_ctrl(a, state, st, k, t, pv, pw);
                a.seqs[((size_t)k * a.T + t) * 2] = pv;
                a.seqs[((size_t)k * a.T + t) * 2 + 1] = pw;
            }
        }
        if (cost != LP_COST_NONE) { key = k; adm = 1; }
    }
    lp_block_best(cost, key, adm, s_cost, s_k, s_n, a.partial + blockIdx.x);
}

__global__ __launch_bounds__(MP_THREADS) void k_mppi_average(mp_args a)
{
    __shared__ uint32_t s_tab[257];
    __shared__ long long s_part[MP_WAVES][MP_MAX_SUMS];
    const int state = blockIdx.x / a.bps, blk = blockIdx.x % a.bps;
    const int tid = threadIdx.x, wave = tid >> 6;
    const bl_mppi_state_t st = a.states[state];
    if (lp_start_flags(a.f, st.s)) return;
    long long c_min; int best, n_adm;
    lp_state_best(a.partial + (size_t)state * a.bps, a.bps, &c_min, &best, &n_adm);
    if (n_adm == 0) return;                                            // BLOCKED: k_mppi_finish reads no sums
    s_tab[tid] = a.wtab[tid];
    if (tid == 0) s_tab[256] = a.wtab[256];
    __syncthreads();
    const int k = blk * MP_THREADS + tid;
    long long wgt = 0;
    if (k < a.K) {
        const long long cost = a.costs[(size_t)state * a.K + k];
        if (cost != LP_COST_NONE) {
            const unsigned long long idx = ((unsigned long long)(cost - c_min) * 16ull) / (unsigned long long)a.lambda;
            wgt = (long long)s_tab[idx < 256ull ? (int)idx : 256];
        }
    }
    int pv = mp_q16(st.s.v), pw = mp_q16(st.s.w);
    for (int t = 0; t <= a.T; ++t) {
        long long n0, n1;
        if (t < a.T) {
            if (wgt) mp_sample_ctrl(a, state, st, k, t, pv, pw);      // a sample of weight 0 adds nothing
            n0 = wgt * pv; n1 = wgt * pw;
        } else { n0 = wgt; n1 = wgt * wgt; }                           // S and Q (as uint64: the same bits)
        for (int off = 32; off > 0; off >>= 1) {
            n0 += __shfl_xor(n0, off);
            n1 += __shfl_xor(n1, off);
        }
        if ((tid & 63) == 0) { s_part[wave][2 * t] = n0; s_part[wave][2 * t + 1] = n1; }
    }
    __syncthreads();
    const int n_sums = 2 * a.T + 2;
    if (tid < n_sums) {
        long long s = 0;
        for (int w = 0; w < MP_WAVES; ++w) s += s_part[w][tid];
        a.sums[((size_t)state * a.bps + blk) * n_sums + tid] = s;
    }
}

template <bool MOVING>
__global__ __launch_bounds__(MP_THREADS) void k_mppi_finish(mp_args a, int32_t* __restrict__ seq_out, bl_mppi_result_t* __restrict__ out)
{
    __shared__ long long s_sum[MP_MAX_SUMS];
    __shared__ int s_cand[2 * BL_MPPI_MAX_HORIZON];
    __shared__ int s_cnt[MP_WAVES];
    __shared__ lp_kept s_kept[BL_OBSTRACKS_MAX_TRACKS];
    const int state = blockIdx.x, tid = threadIdx.x;
    const bl_mppi_state_t st = a.states[state];
    int32_t* so = seq_out + (size_t)state * a.T * 2;
    bl_mppi_result_t r;
    r.trans_v = 0.0f; r.angular_v = 0.0f; r.index_best = -1; r.n_admissible = 0; r.cost_best = LP_COST_NONE; r.cost_out = LP_COST_NONE;
    r.weight_sum = 0; r.weight_sq_sum = 0; r.pad = 0;
    r.flags = lp_start_flags(a.f, st.s);
    long long c_min = LP_COST_NONE; int best = 0x7FFFFFFF, n_adm = 0;
    if (!r.flags) {
        lp_state_best(a.partial + (size_t)state * a.bps, a.bps, &c_min, &best, &n_adm);
        if (n_adm == 0) r.flags = BL_LOCALPLAN_BLOCKED;
    }
    if (r.flags) {                                                     // uniform over the workgroup
        if (r.flags == BL_LOCALPLAN_REACHED) { r.cost_best = 0; r.cost_out = 0; }
        for (int i = tid; i < 2 * a.T; i += MP_THREADS) so[i] = 0;
        if (tid == 0) out[state] = r;
        return;
    }
    const int n_sums = 2 * a.T + 2;
    if (tid < n_sums) {
        long long s = 0;
        for (int b = 0; b < a.bps; ++b) s += a.sums[((size_t)state * a.bps + b) * n_sums + tid];
        s_sum[tid] = s;
    }
    const int kept = mp_keep_slots<MOVING>(a, s_kept, s_cnt);
    __syncthreads();
    if (tid != 0) return;
    const long long S = s_sum[2 * a.T];
    const int pv0 = mp_q16(st.s.v), pw0 = mp_q16(st.s.w);
    int pv = pv0, pw = pw0;
    for (int t = 0; t < a.T; ++t) {
        long long av[2];
        for (int c = 0; c < 2; ++c) {
            const long long num = 2 * s_sum[2 * t + c] + S, den = 2 * S;   // S >= 2^24: the best sample's weight
            long long q = num / den;
            if (num % den < 0) --q;                                   // floor towards minus infinity
            av[c] = q;
        }
        mp_clamp_pair(a, av[0], av[1], pv, pw);
        s_cand[2 * t] = pv; s_cand[2 * t + 1] = pw;
    }
    const long long cost = mp_rollout<false, MOVING>(a, st.s, nullptr, 0, 0, s_kept, kept, false, nullptr,
                                                     [&](int t, int* qv, int* qw) { *qv = s_cand[2 * t]; *qw = s_cand[2 * t + 1]; });
    r.index_best = best; r.n_admissible = n_adm; r.cost_best = c_min;
    r.weight_sum = (unsigned long long)S; r.weight_sq_sum = (unsigned long long)s_sum[2 * a.T + 1];
    if (cost != LP_COST_NONE) {
        r.cost_out = cost;
        for (int i = 0; i < 2 * a.T; ++i) so[i] = s_cand[i];
        r.trans_v = (float)s_cand[0] * 0x1p-16f; r.angular_v = (float)s_cand[1] * 0x1p-16f;
    } else {
        r.cost_out = c_min; r.flags = BL_MPPI_FELL_BACK;
        pv = pv0; pw = pw0;
        for (int t = 0; t < a.T; ++t) {
            mp_sample_ctrl(a, state, st, best, t, pv, pw);
            so[2 * t] = pv; so[2 * t + 1] = pw;
            if (t == 0) { r.trans_v = (float)pv * 0x1p-16f; r.angular_v = (float)pw * 0x1p-16f; }
        }
    }
    out[state] = r;
}

__global__ __launch_bounds__(64) void k_mppi_poses(mp_args a, const int32_t* __restrict__ seq, bl_pose_xyt_t* __restrict__ out)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const bl_localplan_state_t st = a.states[0].s;
    float x = st.pose.x, y = st.pose.y, theta = bl_wrap_to_pi(st.pose.theta);
    int step = 0;
    for (int t = 0; t < a.T; ++t) {
        const float v = (float)seq[2 * t] * 0x1p-16f, w = (float)seq[2 * t + 1] * 0x1p-16f;
        const float s = v * a.f.dt_sim, dth = w * a.f.dt_sim;
        for (int i = 0; i < a.n_sub; ++i) {
            lp_unicycle_step(x, y, theta, s, dth);
            bl_pose_xyt_t p;
            p.utime = st.pose.utime; p.x = x; p.y = y; p.theta = theta;
            out[step++] = p;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- host
struct mp_derived { int vmin_q, vmax_q, wmax_q, nv_q, nw_q, av_q, aw_q; };

struct bl_mppi {
    bl_ctx* ctx;
    bl_mppi_params_t params; mp_derived q; bool have_params;
    void* d_in; size_t d_in_cap;                  // states | seq_in
    void* h_in; size_t h_in_cap;                  // pinned
    void* d_out; size_t d_out_cap;                // results | seq_out, or the debug calls' output
    void* h_out; size_t h_out_cap;                // pinned
    void* d_partial; size_t partial_cap;
    void* d_costs; size_t costs_cap;
    void* d_sums; size_t sums_cap;
    uint32_t* d_wtab;
    hipEvent_t ev0, ev1;
    int last_path; bool timed; float last_ms;
};

extern "C" void bl_mppi_weight_table(uint32_t out[257])
{
    if (!out) return;
    out[0] = 1u << 24;
    for (int i = 1; i < 256; ++i) out[i] = (uint32_t)(((uint64_t)out[i - 1] * 4034748382ull) >> 32);
    out[256] = 0;
}

extern "C" int bl_mppi_create(bl_ctx* ctx, bl_mppi** out)
{
    BL_CHECK_ARG(ctx != nullptr && out != nullptr);
    BL_HIP(hipSetDevice(ctx->device));
    bl_mppi* mp = new bl_mppi();
    memset((void*)mp, 0, sizeof(*mp));
    mp->ctx = ctx;
    mp->last_path = -1;
    uint32_t tab[257];
    bl_mppi_weight_table(tab);
    hipError_t e = hipEventCreate(&mp->ev0);
    if (e == hipSuccess) e = hipEventCreate(&mp->ev1);
    if (e == hipSuccess) e = hipMalloc((void**)&mp->d_wtab, sizeof(tab));
    if (e == hipSuccess) e = hipMemcpy(mp->d_wtab, tab, sizeof(tab), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        bl_set_error("bl_mppi_create: %s", hipGetErrorString(e));
        bl_mppi_destroy(mp);
        return BL_ERR_HIP;
    }
    *out = mp;
    return BL_OK;
}

extern "C" void bl_mppi_destroy(bl_mppi* mp)
{
    if (!mp) return;
    (void)hipSetDevice(mp->ctx->device);
    (void)hipStreamSynchronize(mp->ctx->stream);
    if (mp->d_in) (void)hipFree(mp->d_in);
    if (mp->d_out) (void)hipFree(mp->d_out);
    if (mp->d_partial) (void)hipFree(mp->d_partial);
    if (mp->d_costs) (void)hipFree(mp->d_costs);
    if (mp->d_sums) (void)hipFree(mp->d_sums);
    if (mp->d_wtab) (void)hipFree(mp->d_wtab);
    if (mp->h_in) (void)hipHostFree(mp->h_in);
    if (mp->h_out) (void)hipHostFree(mp->h_out);
    if (mp->ev0) (void)hipEventDestroy(mp->ev0);
    if (mp->ev1) (void)hipEventDestroy(mp->ev1);
    delete mp;
}

extern "C" int bl_mppi_set_params(bl_mppi* mp, const bl_mppi_params_t* p)
{
    BL_CHECK_ARG(mp != nullptr && p != nullptr);
    const float fl[8] = {p->v_min, p->v_max, p->w_max, p->acc_v, p->acc_w, p->dt_sim, p->noise_v, p->noise_w};
    for (float f : fl) BL_CHECK_ARG(isfinite(f));
    BL_CHECK_ARG(p->v_min <= p->v_max && p->w_max >= 0.0f && p->noise_v >= 0.0f && p->noise_w >= 0.0f);
    BL_CHECK_ARG(p->acc_v >= 0.0f && p->acc_w >= 0.0f && p->dt_sim > 0.0f);
    BL_CHECK_ARG(p->n_samples >= 1 && p->n_samples <= BL_MPPI_MAX_SAMPLES && p->horizon >= 1 && p->horizon <= BL_MPPI_MAX_HORIZON);
    BL_CHECK_ARG(p->n_sub >= 1 && p->n_sub <= BL_MPPI_MAX_SUB && p->horizon * p->n_sub <= BL_MPPI_MAX_STEPS);
    BL_CHECK_ARG(p->lambda >= 1 && p->lambda <= BL_MPPI_MAX_LAMBDA);
    const int32_t wt[3] = {p->w_field, p->w_heading, p->w_clear};
    for (int32_t w : wt) BL_CHECK_ARG(w >= 0 && w <= BL_LOCALPLAN_MAX_WEIGHT);
    const double d[7] = {(double)p->v_min * 65536.0, (double)p->v_max * 65536.0, (double)p->w_max * 65536.0, (double)p->noise_v * 65536.0,
                         (double)p->noise_w * 65536.0, (double)p->acc_v * (double)p->dt_sim * p->n_sub * 65536.0,
                         (double)p->acc_w * (double)p->dt_sim * p->n_sub * 65536.0};
    int q[7];
    for (int i = 0; i < 7; ++i) {
        BL_CHECK_ARG(fabs(d[i]) < 4.0 * BL_MPPI_MAX_Q);                // lrint's domain
        q[i] = (int)lrint(d[i]);
        BL_CHECK_ARG(q[i] > -BL_MPPI_MAX_Q && q[i] < BL_MPPI_MAX_Q);
    }
    mp->params = *p;
    mp->q.vmin_q = q[0]; mp->q.vmax_q = q[1]; mp->q.wmax_q = q[2]; mp->q.nv_q = q[3]; mp->q.nw_q = q[4]; mp->q.av_q = q[5]; mp->q.aw_q = q[6];
    mp->have_params = true;
    return BL_OK;
}

static int mp_state_ok(const bl_mppi_state_t* s, int n)
{
    for (int i = 0; i < n; ++i) {
        const bl_localplan_state_t& l = s[i].s;
        const int rc = lp_state_ok(&l, 1);
        if (rc) return rc;
        BL_CHECK_ARG(fabs((double)l.v * 65536.0) < 4.0 * BL_MPPI_MAX_Q && fabs((double)l.w * 65536.0) < 4.0 * BL_MPPI_MAX_Q);
        BL_CHECK_ARG(abs(mp_q16(l.v)) < BL_MPPI_MAX_Q && abs(mp_q16(l.w)) < BL_MPPI_MAX_Q);
    }
    return BL_OK;
}

// what every call that sees the field checks, and the launch arguments that follow from field, tracker and parameters
static int mp_prepare(bl_mppi* mp, bl_navfield* nf, bl_obstracks* tr, const bl_localplan_moving_t* m, const bl_mppi_state_t* states, int n,
                      mp_args* a, bool* staged)
{
    BL_CHECK_ARG(mp != nullptr && nf != nullptr);
    BL_CHECK_ARG((tr == nullptr) == (m == nullptr));
    int rc = m ? lp_moving_check(m) : BL_OK;
    if (rc) return rc;
    if (!mp->have_params) { bl_set_error("sampling local planner has no parameters (bl_mppi_set_params first)"); return BL_ERR_STATE; }
    const bl_mppi_params_t& p = mp->params;
    memset((void*)a, 0, sizeof(*a));
    int reach_r;                                                       // (only the arc planner's moving prologue wants it)
    rc = lp_prepare_field("sampling local planner", mp->ctx, nf, n, states != nullptr, p.v_min, p.v_max, p.dt_sim, p.horizon * p.n_sub, p.w_field,
                          p.w_heading, p.w_clear, &a->f, &reach_r, staged);
    if (!rc) rc = mp_state_ok(states, n);
    if (!rc && tr) rc = lp_prepare_tracks(mp->ctx, nf, tr, m, &a->m);
    if (rc) return rc;
    a->K = p.n_samples; a->T = p.horizon; a->n_sub = p.n_sub;
    a->bps = (p.n_samples + MP_THREADS - 1) / MP_THREADS;
    a->lambda = p.lambda;
    a->vmin_q = mp->q.vmin_q; a->vmax_q = mp->q.vmax_q; a->wmax_q = mp->q.wmax_q; a->nv_q = mp->q.nv_q; a->nw_q = mp->q.nw_q;
    a->av_q = mp->q.av_q; a->aw_q = mp->q.aw_q;
    a->seed_lo = (uint32_t)(p.seed & 0xFFFFFFFFull); a->seed_hi = (uint32_t)(p.seed >> 32);
    a->wtab = mp->d_wtab;
    return BL_OK;
}

// states and the nominal sequences into the pinned block and on to the device (no synchronisation); the per-sample buffers grown
static int mp_upload(bl_mppi* mp, const bl_mppi_state_t* states, int n, const int32_t* seq_in, mp_args* a)
{
    bl_ctx* ctx = mp->ctx;
    const size_t sb = (size_t)n * sizeof(bl_mppi_state_t), qb = seq_in ? (size_t)n * a->T * 8 : 0;
    int rc = bl_grow(&mp->d_in, &mp->d_in_cap, sb + qb, false, ctx);
    if (!rc) rc = bl_grow(&mp->h_in, &mp->h_in_cap, sb + qb, true, ctx);
    if (!rc) rc = bl_grow(&mp->d_partial, &mp->partial_cap, (size_t)n * a->bps * sizeof(lp_partial), false, ctx);
    if (!rc) rc = bl_grow(&mp->d_costs, &mp->costs_cap, (size_t)n * a->K * 8, false, ctx);
    if (!rc) rc = bl_grow(&mp->d_sums, &mp->sums_cap, (size_t)n * a->bps * (2 * a->T + 2) * 8, false, ctx);
    if (rc) return rc;
    char* h = (char*)mp->h_in;
    memcpy(h, states, sb);
    if (seq_in) memcpy(h + sb, seq_in, qb);
    BL_HIP(hipMemcpyAsync(mp->d_in, mp->h_in, sb + qb, hipMemcpyHostToDevice, ctx->stream));
    a->states = (const bl_mppi_state_t*)mp->d_in;
    a->seq_in = seq_in ? (const int32_t*)((char*)mp->d_in + sb) : nullptr;
    a->partial = (lp_partial*)mp->d_partial;
    a->costs = (long long*)mp->d_costs;
    a->sums = (long long*)mp->d_sums;
    return BL_OK;
}

static int mp_launch_rollout(bl_mppi* mp, const mp_args& a, int n, bool staged, bool moving)
{
    bl_ctx* ctx = mp->ctx;
    const size_t lds = MP_LDS_FIXED + lp_window_lds(a.f, staged);
    const dim3 grid((unsigned int)(n * a.bps)), block(MP_THREADS);
    const size_t lds_max = MP_LDS_FIXED + BL_LOCALPLAN_WINDOW_BYTES + 16;
    if (staged && moving) {
        BL_DYN_LDS_ONCE_PER_DEVICE((k_mppi_rollout<true, true>), lds_max, ctx);
        hipLaunchKernelGGL((k_mppi_rollout<true, true>), grid, block, lds, ctx->stream, a);
    } else if (staged) {
        BL_DYN_LDS_ONCE_PER_DEVICE((k_mppi_rollout<true, false>), lds_max, ctx);
        hipLaunchKernelGGL((k_mppi_rollout<true, false>), grid, block, lds, ctx->stream, a);
    } else if (moving) {
        hipLaunchKernelGGL((k_mppi_rollout<false, true>), grid, block, lds, ctx->stream, a);
    } else {
        hipLaunchKernelGGL((k_mppi_rollout<false, false>), grid, block, lds, ctx->stream, a);
    }
    BL_HIP(hipGetLastError());
    mp->last_path = staged ? 0 : 1;
    return BL_OK;
}

extern "C" int bl_mppi_plan(bl_mppi* mp, bl_navfield* nf, bl_obstracks* tr, const bl_localplan_moving_t* m, const bl_mppi_state_t* states, int n,
                            const int32_t* seq_in, int32_t* seq_out, bl_mppi_result_t* results)
{
    mp_args a;
    bool staged = false;
    int rc = mp_prepare(mp, nf, tr, m, states, n, &a, &staged);
    if (rc) return rc;
    BL_CHECK_ARG(n == 0 || (results != nullptr && seq_out != nullptr));
    if (n == 0) return BL_OK;
    bl_ctx* ctx = mp->ctx;
    BL_HIP(hipSetDevice(ctx->device));
    const size_t rb = (size_t)n * sizeof(bl_mppi_result_t), qb = (size_t)n * a.T * 8;
    rc = bl_grow(&mp->d_out, &mp->d_out_cap, rb + qb, false, ctx);
    if (!rc) rc = bl_grow(&mp->h_out, &mp->h_out_cap, rb + qb, true, ctx);
    if (!rc) rc = mp_upload(mp, states, n, seq_in, &a);
    if (rc) return rc;
    BL_HIP(hipEventRecord(mp->ev0, ctx->stream));
    rc = mp_launch_rollout(mp, a, n, staged, tr != nullptr);
    if (rc) return rc;
    hipLaunchKernelGGL(k_mppi_average, dim3((unsigned int)(n * a.bps)), dim3(MP_THREADS), 0, ctx->stream, a);
    BL_HIP(hipGetLastError());
    bl_mppi_result_t* d_res = (bl_mppi_result_t*)mp->d_out;
    int32_t* d_seq = (int32_t*)((char*)mp->d_out + rb);
    if (tr) hipLaunchKernelGGL(k_mppi_finish<true>, dim3((unsigned int)n), dim3(MP_THREADS), 0, ctx->stream, a, d_seq, d_res);
    else hipLaunchKernelGGL(k_mppi_finish<false>, dim3((unsigned int)n), dim3(MP_THREADS), 0, ctx->stream, a, d_seq, d_res);
    BL_HIP(hipGetLastError());
    BL_HIP(hipEventRecord(mp->ev1, ctx->stream));
    BL_HIP(hipMemcpyAsync(mp->h_out, mp->d_out, rb + qb, hipMemcpyDeviceToHost, ctx->stream));
    BL_HIP(hipStreamSynchronize(ctx->stream));
    memcpy(results, mp->h_out, rb);
    memcpy(seq_out, (const char*)mp->h_out + rb, qb);
    BL_HIP(hipEventElapsedTime(&mp->last_ms, mp->ev0, mp->ev1));
    mp->timed = true;
    return BL_OK;
}

extern "C" int bl_mppi_debug_samples(bl_mppi* mp, bl_navfield* nf, bl_obstracks* tr, const bl_localplan_moving_t* m, const bl_mppi_state_t* state,
                                     const int32_t* seq_in, int64_t* costs, int32_t* first_hit, int32_t* seqs)
{
    mp_args a;
    bool staged = false;
    BL_CHECK_ARG(state != nullptr && costs != nullptr);
    int rc = mp_prepare(mp, nf, tr, m, state, 1, &a, &staged);
    if (rc) return rc;
    bl_ctx* ctx = mp->ctx;
    BL_HIP(hipSetDevice(ctx->device));
    const size_t K = (size_t)a.K, cb = K * 8, fb = K * 4, qb = K * a.T * 8, ob = cb + fb + qb;   // costs | first hits | sequences
    rc = bl_grow(&mp->d_out, &mp->d_out_cap, ob, false, ctx);
    if (!rc) rc = bl_grow(&mp->h_out, &mp->h_out_cap, ob, true, ctx);
    if (!rc) rc = mp_upload(mp, state, 1, seq_in, &a);
    if (rc) return rc;
    a.debug = 1;
    a.costs = (long long*)mp->d_out;
    a.first_hit = tr ? (int*)((char*)mp->d_out + cb) : nullptr;
    a.seqs = seqs ? (int32_t*)((char*)mp->d_out + cb + fb) : nullptr;
    rc = mp_launch_rollout(mp, a, 1, staged, tr != nullptr);
    if (rc) return rc;
    BL_HIP(hipMemcpyAsync(mp->h_out, mp->d_out, seqs ? ob : cb + fb, hipMemcpyDeviceToHost, ctx->stream));
    BL_HIP(hipStreamSynchronize(ctx->stream));
    memcpy(costs, mp->h_out, cb);
    if (first_hit) { if (tr) memcpy(first_hit, (const char*)mp->h_out + cb, fb); else memset(first_hit, 0, fb); }
    if (seqs) memcpy(seqs, (const char*)mp->h_out + cb + fb, qb);
    return BL_OK;
}

extern "C" int bl_mppi_debug_rollout(bl_mppi* mp, bl_navfield* nf, const bl_mppi_state_t* state, const int32_t* seq, bl_pose_xyt_t* out)
{
    mp_args a;
    bool staged = false;
    BL_CHECK_ARG(state != nullptr && out != nullptr);
    int rc = mp_prepare(mp, nf, nullptr, nullptr, state, 1, &a, &staged);
    if (rc) return rc;
    if (seq) for (int i = 0; i < 2 * a.T; ++i) BL_CHECK_ARG(seq[i] > -BL_MPPI_MAX_Q && seq[i] < BL_MPPI_MAX_Q);
    bl_ctx* ctx = mp->ctx;
    BL_HIP(hipSetDevice(ctx->device));
    const size_t pb = (size_t)a.T * a.n_sub * sizeof(bl_pose_xyt_t);
    rc = bl_grow(&mp->d_out, &mp->d_out_cap, pb, false, ctx);
    if (!rc) rc = bl_grow(&mp->h_out, &mp->h_out_cap, pb, true, ctx);
    std::vector<int32_t> zeros;
    if (!seq) { zeros.assign((size_t)2 * a.T, 0); seq = zeros.data(); }
    if (!rc) rc = mp_upload(mp, state, 1, seq, &a);
    if (rc) return rc;
    hipLaunchKernelGGL(k_mppi_poses, dim3(1), dim3(64), 0, ctx->stream, a, a.seq_in, (bl_pose_xyt_t*)mp->d_out);
    BL_HIP(hipGetLastError());
    BL_HIP(hipMemcpyAsync(mp->h_out, mp->d_out, pb, hipMemcpyDeviceToHost, ctx->stream));
    BL_HIP(hipStreamSynchronize(ctx->stream));
    memcpy(out, mp->h_out, pb);
    return BL_OK;
}

extern "C" int bl_mppi_debug_path(const bl_mppi* mp) { return mp ? mp->last_path : -1; }

extern "C" int bl_mppi_last_device_ms(const bl_mppi* mp, float* ms)
{
    BL_CHECK_ARG(mp != nullptr && ms != nullptr);
    if (!mp->timed) { bl_set_error("bl_mppi_last_device_ms: no bl_mppi_plan yet"); return BL_ERR_STATE; }
    *ms = mp->last_ms;
    return BL_OK;
}
