// bl_localplan.hip -- the local planner (include/botlab_hip.h, "local planner"): velocity commands by rollout over a navigation
// field.  No reference counterpart for the algorithm; the definition in the header is the contract and tests/local_plan_model.py
// restates it.
//
//   k_lp_rollout  a workgroup per (state, run of LP jpb consecutive headings j).  Three phases:
//                   A  one thread per j walks theta_k = wrap_to_pi(theta_{k-1} + dth) into LDS (a serial chain, float adds only)
//                   B  all threads turn the jpb * n_steps headings into (cos, sin) in place: the double-precision polynomial is
//                      paid once per (j, k), not once per candidate
//                   C  a thread per candidate (i, j) integrates its arc; the n_v lanes of one j read the same (cos, sin) slot, an
//                      LDS broadcast; every visited cell's cost (-1 or the penalty) comes from the window staged in LDS (STAGED) or
//                      from the grids; the end cell's field and the descent move from it are read from the grids, once
//                 then the least (cost, c) key of the workgroup goes to its slot: no atomics, no floats in the reduction
//                 MOVING (bl_localplan_commands_moving) adds a prologue -- a lane per tracker slot decides used and can-reach, the kept
//                 slots go to LDS in slot order by ballot -- and, when they fit, a table of the kept boxes at every step beside
//                 phase B; phase C then also tests every visited cell against the boxes of its step
//   k_lp_finish   a thread per state: the flags of the pose's own cell, else the least key over the state's workgroups
//   k_lp_poses    one thread: the poses of one candidate (bl_localplan_debug_rollout)
//
// What the sampling planner (bl_mppi.hip) does by the same rule is in bl_localplan_dev.h: the start flags, the window (corner, staging,
// a visited cell's cost), the end score, the unicycle step, the key reductions, the moving rule and its compaction, and on the host
// the field's and the tracker's checks and launch arguments.  Here stay the (cos, sin) phases, the box table, w_speed and the tables.
#include <math.h>
#include <string.h>

#include "bl_internal.h"
#include "bl_navfield_dev.h"
#include "bl_localplan_dev.h"

#define LP_TRIG_SLOTS 2048             // (cos, sin) pairs of a workgroup: jpb * (n_steps + 1) of them, the last of each j holds theta_end
#define LP_RED_BYTES 64                // per wave: key cost (8), key c (4), admissible count (4)
#define LP_LDS_FIXED (LP_TRIG_SLOTS * 8 + LP_RED_BYTES)
#define LP_MOV_KEPT_BYTES (BL_OBSTRACKS_MAX_TRACKS * 20)                  // lp_kept: five words per kept slot
#define LP_MOV_BYTES (LP_MOV_KEPT_BYTES + BL_LOCALPLAN_MOVING_BYTES)
// two workgroups with the largest window and the moving block fit a CU's 160 KiB
static_assert(2 * (LP_LDS_FIXED + BL_LOCALPLAN_WINDOW_BYTES + 16 + LP_MOV_BYTES) <= 160 * 1024, "BL_LOCALPLAN_MOVING_BYTES too large");

struct lp_args {
    lp_field f;
    const bl_localplan_state_t* states;
    const float* v_tab; const float* w_tab;      // [state][n_v], [state][n_w]
    int n_v, n_w, n_steps;
    int nvp, jpb, bps;                            // lanes per heading (a power of two >= n_v), headings and workgroups per state
    int w_speed;
    lp_partial* partial;                          // [state][bps]
    long long* costs;                             // bl_localplan_debug_costs: every candidate's cost (one state); else null
    // MOVING only
    lp_moving m;
    int reach_r;                                  // R of the window rule, staged or not
    int mov_off;                                  // where the moving block starts in the dynamic LDS
    int* first_hit;                               // bl_localplan_debug_costs_moving: per candidate; else null
    int* mpath;                                   // [state]: 0 table, 1 per step, 2 nothing kept, -1 not rolled out (the state's first workgroup writes it)
};

template <bool STAGED, bool MOVING>
__global__ __launch_bounds__(LP_THREADS) void k_lp_rollout(lp_args a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    float2* s_trig = (float2*)s_raw;
    long long* s_cost = (long long*)(s_raw + LP_TRIG_SLOTS * 8);
    int* s_c = (int*)(s_raw + LP_TRIG_SLOTS * 8 + 32);
    int* s_n = (int*)(s_raw + LP_TRIG_SLOTS * 8 + 48);
    int16_t* s_win = (int16_t*)(s_raw + LP_LDS_FIXED);
    const int state = blockIdx.x / a.bps, blk = blockIdx.x % a.bps;
    const int tid = threadIdx.x;
    const int W = a.f.frame.width, H = a.f.frame.height;
    const bl_localplan_state_t st = a.states[state];
    const int flags = lp_start_flags(a.f, st);
    if (flags && !a.costs) {                                         // nothing is rolled out (uniform over the workgroup)
        if (MOVING && blk == 0 && tid == 0) a.mpath[state] = -1;
        return;
    }
    int wx0 = 0, wy0 = 0;
    int rx0 = 0, ry0 = 0;                                             // MOVING: the reach square's corner, its side 2 * reach_r + 1
    if (STAGED || MOVING) {
        lp_window_corner(a.f.frame, st.pose, a.f.win_r, &wx0, &wy0);
        lp_window_corner(a.f.frame, st.pose, a.reach_r, &rx0, &ry0);
    }
    // MOVING prologue, first half: a lane per slot decides used and can-reach; the waves' counts go where the reduction's will
    lp_kept* s_kept = (lp_kept*)(s_raw + a.mov_off);
    short4* s_box = (short4*)(s_raw + a.mov_off + LP_MOV_KEPT_BYTES);
    const int rside = 2 * a.reach_r;
    bool keep = false, used = false;
    lp_kept rec;
    unsigned long long keep_mask = 0ull;
    if (MOVING) {
        const bl_obstrack_t tr = a.m.slots[tid];
        used = lp_mov_used(tr);
        rec = lp_mov_record(tr, a.m.mmargin);
        if (used) {
            // the displacement is monotone in k per axis: the two ends bound the sweep
            const int vx = (int)(short)(rec.v & 0xffff), vy = rec.v >> 16;
            const int ox1 = lp_mov_offset(1 + a.m.mlead, vx, a.m.mq), oxn = lp_mov_offset(a.n_steps + a.m.mlead, vx, a.m.mq);
            const int oy1 = lp_mov_offset(1 + a.m.mlead, vy, a.m.mq), oyn = lp_mov_offset(a.n_steps + a.m.mlead, vy, a.m.mq);
            const long long lx = (long long)rec.x0 + min(ox1, oxn), hx = (long long)rec.x1 + max(ox1, oxn);
            const long long ly = (long long)rec.y0 + min(oy1, oyn), hy = (long long)rec.y1 + max(oy1, oyn);
            keep = hx >= (long long)rx0 && lx <= (long long)rx0 + rside && hy >= (long long)ry0 && ly <= (long long)ry0 + rside;
        }
        keep_mask = __ballot(keep);
        const unsigned long long used_mask = __ballot(used);
        if ((tid & 63) == 0) { s_n[tid >> 6] = __popcll(keep_mask); s_c[tid >> 6] = __popcll(used_mask); }
    }
    if (STAGED) lp_stage_window(a.f, s_win, wx0, wy0);
    // A: the headings of this workgroup's j
    const int stride = a.n_steps + 1;
    const int j0 = blk * a.jpb;
    if (tid < a.jpb && j0 + tid < a.n_w) {
        float theta = bl_wrap_to_pi(st.pose.theta);
        const float dth = a.w_tab[(size_t)state * a.n_w + j0 + tid] * a.f.dt_sim;
        float2* row = s_trig + tid * stride;
        for (int k = 0; k < a.n_steps; ++k) {
            row[k].x = theta;
            theta = bl_wrap_to_pi(theta + dth);
        }
        row[a.n_steps].x = theta;
    }
    __syncthreads();
    // MOVING prologue, second half: the kept slots compacted in slot order
    int kept = 0, n_used = 0;
    bool boxed = false;
    if (MOVING) {
        for (int w = 0; w < LP_WAVES; ++w) n_used += s_c[w];
        kept = lp_mov_compact(s_n, keep_mask, keep, rec, s_kept);
        boxed = kept > 0 && (long long)kept * a.n_steps * 8 <= (long long)BL_LOCALPLAN_MOVING_BYTES;
        if (blk == 0 && tid == 0) a.mpath[state] = kept == 0 ? 2 : boxed ? 0 : 1;
    }
    // B: their (cos, sin), in place
    for (int idx = tid; idx < a.jpb * stride; idx += LP_THREADS) {
        const int jl = idx / stride, k = idx - jl * stride;
        if (k == a.n_steps || j0 + jl >= a.n_w) continue;
        float sn, cs;
        bl_sincosf(s_trig[idx].x, &sn, &cs);
        s_trig[idx] = make_float2(cs, sn);
    }
    __syncthreads();
    // MOVING, the table: every kept box at every step, clamped to the reach square and relative to its corner (an empty one is 1 > 0)
    if (MOVING) {
        if (boxed) {
            for (int idx = tid; idx < kept * a.n_steps; idx += LP_THREADS) {
                const int b = idx / a.n_steps, k = idx - b * a.n_steps;
                const lp_kept r = s_kept[b];
                const int t = k + 1 + a.m.mlead;
                const int ox = lp_mov_offset(t, (int)(short)(r.v & 0xffff), a.m.mq), oy = lp_mov_offset(t, r.v >> 16, a.m.mq);
                const long long lx = max((long long)r.x0 + ox, (long long)rx0) - rx0, hx = min((long long)r.x1 + ox, (long long)rx0 + rside) - rx0;
                const long long ly = max((long long)r.y0 + oy, (long long)ry0) - ry0, hy = min((long long)r.y1 + oy, (long long)ry0 + rside) - ry0;
                short4 bx;
                if (lx > hx || ly > hy) { bx.x = 1; bx.y = 1; bx.z = 0; bx.w = 0; }
                else { bx.x = (short)lx; bx.y = (short)ly; bx.z = (short)hx; bx.w = (short)hy; }
                s_box[idx] = bx;
            }
        }
        __syncthreads();
    }
    // C: a thread per candidate
    const int i = tid & (a.nvp - 1), jl = tid / a.nvp, j = j0 + jl;
    const bool active = i < a.n_v && jl < a.jpb && j < a.n_w;
    long long cost = LP_COST_NONE;
    int c = 0x7FFFFFFF, adm = 0;
    if (active) {
        c = j * a.n_v + i;
        const float s = a.v_tab[(size_t)state * a.n_v + i] * a.f.dt_sim;
        const float2* row = s_trig + jl * stride;
        float x = st.pose.x, y = st.pose.y;
        int ex = 0, ey = 0, pen = 0;
        bool ok = true;
        const bool all_steps = MOVING && a.first_hit != nullptr;      // the debug call looks at every step, rejected or not
        int hit_k = 0;
        for (int k = 0; k < a.n_steps; ++k) {
            const float2 t = row[k];
            x = x + s * t.x;
            y = y + s * t.y;
            if (!nav_pose_cell(a.f.frame, x, y, &ex, &ey)) { ok = false; if (all_steps) continue; break; }
            if (MOVING && hit_k == 0 && n_used > 0) {
                const int mx = ex - rx0, my = ey - ry0;
                bool hit = false;
                if ((unsigned)mx <= (unsigned)rside && (unsigned)my <= (unsigned)rside) {
                    if (boxed) {
                        for (int b = 0; b < kept; ++b) {
                            const short4 bx = s_box[b * a.n_steps + k];  // one broadcast read per (box, step)
                            hit = hit || (mx >= bx.x && mx <= bx.z && my >= bx.y && my <= bx.w);
                        }
                    } else {
                        for (int b = 0; b < kept; ++b) hit = hit || lp_mov_in_box(s_kept[b], k + 1 + a.m.mlead, a.m.mq, ex, ey);
                    }
                } else hit = lp_mov_hit_all(a.m.slots, a.m.mmargin, k + 1 + a.m.mlead, a.m.mq, ex, ey);
                if (hit) { hit_k = k + 1; ok = false; if (all_steps) continue; break; }
            }
            if (MOVING && !ok) continue;                              // (all_steps: only the moving test is still wanted)
            const int q = lp_cell_cost<STAGED>(a.f, s_win, wx0, wy0, ex, ey);
            if (q < 0) { ok = false; if (all_steps) continue; break; }
            pen += q;
        }
        if (all_steps) a.first_hit[c] = hit_k;
        long long score;
        if (lp_end_score(a.f, W, H, ok, ex, ey, row[a.n_steps].x, pen, &score)) {
            cost = score + (long long)a.w_speed * (a.n_v - 1 - i);
            adm = 1;
        }
        if (a.costs) a.costs[c] = cost;
        if (!adm) c = 0x7FFFFFFF;
    }
    lp_block_best(cost, c, adm, s_cost, s_c, s_n, a.partial + blockIdx.x);
}

__global__ __launch_bounds__(64) void k_lp_finish(lp_args a, int n_states, bl_localplan_result_t* __restrict__ out)
{
    const int state = blockIdx.x * 64 + threadIdx.x;
    if (state >= n_states) return;
    const bl_localplan_state_t st = a.states[state];
    bl_localplan_result_t r;
    r.trans_v = 0.0f; r.angular_v = 0.0f; r.index = -1; r.n_admissible = 0; r.cost = LP_COST_NONE; r.pad = 0;
    r.flags = lp_start_flags(a.f, st);
    if (r.flags == BL_LOCALPLAN_REACHED) r.cost = 0;
    if (!r.flags) {
        long long cost;
        int c, adm;
        lp_state_best(a.partial + (size_t)state * a.bps, a.bps, &cost, &c, &adm);
        r.n_admissible = adm;
        if (adm == 0) r.flags = BL_LOCALPLAN_BLOCKED;
        else {
            r.index = c; r.cost = cost;
            r.trans_v = a.v_tab[(size_t)state * a.n_v + c % a.n_v];
            r.angular_v = a.w_tab[(size_t)state * a.n_w + c / a.n_v];
        }
    }
    out[state] = r;
}

__global__ __launch_bounds__(64) void k_lp_poses(lp_args a, int c, bl_pose_xyt_t* __restrict__ out)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const bl_localplan_state_t st = a.states[0];
    const float s = a.v_tab[c % a.n_v] * a.f.dt_sim, dth = a.w_tab[c / a.n_v] * a.f.dt_sim;
    float x = st.pose.x, y = st.pose.y, theta = bl_wrap_to_pi(st.pose.theta);
    for (int k = 0; k < a.n_steps; ++k) {
        lp_unicycle_step(x, y, theta, s, dth);
        bl_pose_xyt_t p;
        p.utime = st.pose.utime; p.x = x; p.y = y; p.theta = theta;
        out[k] = p;
    }
}

// ---------------------------------------------------------------------------------------------------------------- host
struct bl_localplan {
    bl_ctx* ctx;
    bl_localplan_params_t params; bool have_params;
    void* d_in; size_t d_in_cap;                  // states | v tables | w tables
    void* h_in; size_t h_in_cap;                  // pinned
    void* d_out; size_t d_out_cap;                // results, or debug costs / poses
    void* h_out; size_t h_out_cap;                // pinned
    lp_partial* d_partial; size_t partial_cap;
    hipEvent_t ev0, ev1;
    int last_path; bool timed; float last_ms;
    int last_mpath;                               // bl_localplan_debug_moving_path
};

extern "C" int bl_localplan_create(bl_ctx* ctx, bl_localplan** out)
{
    BL_CHECK_ARG(ctx != nullptr && out != nullptr);
    BL_HIP(hipSetDevice(ctx->device));
    bl_localplan* lp = new bl_localplan();
    memset((void*)lp, 0, sizeof(*lp));
    lp->ctx = ctx;
    lp->last_path = -1;
    lp->last_mpath = -1;
    hipError_t e = hipEventCreate(&lp->ev0);
    if (e == hipSuccess) e = hipEventCreate(&lp->ev1);
    if (e != hipSuccess) {
        bl_set_error("bl_localplan_create: %s", hipGetErrorString(e));
        bl_localplan_destroy(lp);
        return BL_ERR_HIP;
    }
    *out = lp;
    return BL_OK;
}

extern "C" void bl_localplan_destroy(bl_localplan* lp)
{
    if (!lp) return;
    (void)hipSetDevice(lp->ctx->device);
    (void)hipStreamSynchronize(lp->ctx->stream);
    if (lp->d_in) (void)hipFree(lp->d_in);
    if (lp->d_out) (void)hipFree(lp->d_out);
    if (lp->d_partial) (void)hipFree(lp->d_partial);
    if (lp->h_in) (void)hipHostFree(lp->h_in);
    if (lp->h_out) (void)hipHostFree(lp->h_out);
    if (lp->ev0) (void)hipEventDestroy(lp->ev0);
    if (lp->ev1) (void)hipEventDestroy(lp->ev1);
    delete lp;
}

extern "C" int bl_localplan_set_params(bl_localplan* lp, const bl_localplan_params_t* p)
{
    BL_CHECK_ARG(lp != nullptr && p != nullptr);
    const float fl[7] = {p->v_min, p->v_max, p->w_max, p->acc_v, p->acc_w, p->dt_control, p->dt_sim};
    for (float f : fl) BL_CHECK_ARG(isfinite(f));
    BL_CHECK_ARG(p->v_min <= p->v_max && p->w_max >= 0.0f && p->dt_control > 0.0f && p->dt_sim > 0.0f);
    BL_CHECK_ARG(p->n_v >= 1 && p->n_v <= BL_LOCALPLAN_MAX_NV && p->n_w >= 1 && p->n_w <= BL_LOCALPLAN_MAX_NW);
    BL_CHECK_ARG(p->n_steps >= 1 && p->n_steps <= BL_LOCALPLAN_MAX_STEPS);
    const int32_t wt[4] = {p->w_field, p->w_heading, p->w_clear, p->w_speed};
    for (int32_t w : wt) BL_CHECK_ARG(w >= 0 && w <= BL_LOCALPLAN_MAX_WEIGHT);
    lp->params = *p;
    lp->have_params = true;
    return BL_OK;
}

// one candidate table of the definition, in double, narrowed once
static void lp_table(double cur, double lim_lo, double lim_hi, double acc, double dt, int n, float* out)
{
    double lo = fmax(lim_lo, cur - acc * dt), hi = fmin(lim_hi, cur + acc * dt);
    if (lo > hi) lo = hi = fmin(fmax(cur, lim_lo), lim_hi);
    for (int i = 0; i < n; ++i) out[i] = n == 1 ? (float)hi : (float)(lo + (hi - lo) * i / (n - 1));
}

static void lp_tables_of(const bl_localplan_params_t& p, const bl_localplan_state_t& st, float* v, float* w)
{
    if (v) lp_table((double)st.v, (double)p.v_min, (double)p.v_max, (double)p.acc_v, (double)p.dt_control, p.n_v, v);
    if (w) lp_table((double)st.w, -(double)p.w_max, (double)p.w_max, (double)p.acc_w, (double)p.dt_control, p.n_w, w);
}

extern "C" int bl_localplan_tables(bl_localplan* lp, const bl_localplan_state_t* state, float* v, float* w)
{
    BL_CHECK_ARG(lp != nullptr && state != nullptr);
    if (!lp->have_params) { bl_set_error("bl_localplan_tables: no parameters (bl_localplan_set_params first)"); return BL_ERR_STATE; }
    int rc = lp_state_ok(state, 1);
    if (rc) return rc;
    lp_tables_of(lp->params, *state, v, w);
    return BL_OK;
}

// what every call that sees the field checks, and the launch arguments that follow from field and parameters
static int lp_prepare(bl_localplan* lp, bl_navfield* nf, const bl_localplan_state_t* states, int n, lp_args* a, bool* staged)
{
    BL_CHECK_ARG(lp != nullptr && nf != nullptr);
    if (!lp->have_params) { bl_set_error("local planner has no parameters (bl_localplan_set_params first)"); return BL_ERR_STATE; }
    const bl_localplan_params_t& p = lp->params;
    memset((void*)a, 0, sizeof(*a));
    int rc = lp_prepare_field("local planner", lp->ctx, nf, n, states != nullptr, p.v_min, p.v_max, p.dt_sim, p.n_steps, p.w_field, p.w_heading,
                              p.w_clear, &a->f, &a->reach_r, staged);
    if (!rc) rc = lp_state_ok(states, n);
    if (rc) return rc;
    a->n_v = p.n_v; a->n_w = p.n_w; a->n_steps = p.n_steps;
    int nvp = 1;
    while (nvp < p.n_v) nvp *= 2;
    a->nvp = nvp;
    int jpb = LP_THREADS / nvp;
    if (jpb > LP_TRIG_SLOTS / (p.n_steps + 1)) jpb = LP_TRIG_SLOTS / (p.n_steps + 1);
    if (jpb > p.n_w) jpb = p.n_w;
    a->jpb = jpb;
    a->bps = (p.n_w + jpb - 1) / jpb;
    a->w_speed = p.w_speed;
    return BL_OK;
}

// states and their tables into the pinned block and on to the device (no synchronisation)
static int lp_upload(bl_localplan* lp, const bl_localplan_state_t* states, int n, lp_args* a)
{
    bl_ctx* ctx = lp->ctx;
    const bl_localplan_params_t& p = lp->params;
    const size_t sb = (size_t)n * sizeof(bl_localplan_state_t), vb = (size_t)n * p.n_v * 4, wb = (size_t)n * p.n_w * 4;
    int rc = bl_grow(&lp->d_in, &lp->d_in_cap, sb + vb + wb, false, ctx);
    if (!rc) rc = bl_grow(&lp->h_in, &lp->h_in_cap, sb + vb + wb, true, ctx);
    if (!rc) rc = bl_grow((void**)&lp->d_partial, &lp->partial_cap, (size_t)n * a->bps * sizeof(lp_partial), false, ctx);
    if (rc) return rc;
    char* h = (char*)lp->h_in;
    memcpy(h, states, sb);
    for (int i = 0; i < n; ++i) lp_tables_of(p, states[i], (float*)(h + sb) + (size_t)i * p.n_v, (float*)(h + sb + vb) + (size_t)i * p.n_w);
    BL_HIP(hipMemcpyAsync(lp->d_in, lp->h_in, sb + vb + wb, hipMemcpyHostToDevice, ctx->stream));
    a->states = (const bl_localplan_state_t*)lp->d_in;
    a->v_tab = (const float*)((char*)lp->d_in + sb);
    a->w_tab = (const float*)((char*)lp->d_in + sb + vb);
    a->partial = lp->d_partial;
    return BL_OK;
}

static int lp_launch_rollout(bl_localplan* lp, const lp_args& a, int n, bool staged)
{
    bl_ctx* ctx = lp->ctx;
    const size_t lds = LP_LDS_FIXED + lp_window_lds(a.f, staged);
    if (staged) {
        BL_DYN_LDS_ONCE_PER_DEVICE((k_lp_rollout<true, false>), LP_LDS_FIXED + BL_LOCALPLAN_WINDOW_BYTES + 16, ctx);
        hipLaunchKernelGGL((k_lp_rollout<true, false>), dim3((unsigned int)(n * a.bps)), dim3(LP_THREADS), lds, ctx->stream, a);
    } else {
        hipLaunchKernelGGL((k_lp_rollout<false, false>), dim3((unsigned int)(n * a.bps)), dim3(LP_THREADS), lds, ctx->stream, a);
    }
    BL_HIP(hipGetLastError());
    lp->last_path = staged ? 0 : 1;
    return BL_OK;
}

// a.mov_off is set here: the moving block lies behind the window
static int lp_launch_rollout_moving(bl_localplan* lp, lp_args& a, int n, bool staged)
{
    bl_ctx* ctx = lp->ctx;
    a.mov_off = (int)(LP_LDS_FIXED + lp_window_lds(a.f, staged));
    const size_t lds = (size_t)a.mov_off + LP_MOV_BYTES;
    if (staged) {
        BL_DYN_LDS_ONCE_PER_DEVICE((k_lp_rollout<true, true>), LP_LDS_FIXED + BL_LOCALPLAN_WINDOW_BYTES + 16 + LP_MOV_BYTES, ctx);
        hipLaunchKernelGGL((k_lp_rollout<true, true>), dim3((unsigned int)(n * a.bps)), dim3(LP_THREADS), lds, ctx->stream, a);
    } else {
        hipLaunchKernelGGL((k_lp_rollout<false, true>), dim3((unsigned int)(n * a.bps)), dim3(LP_THREADS), lds, ctx->stream, a);
    }
    BL_HIP(hipGetLastError());
    lp->last_path = staged ? 0 : 1;
    return BL_OK;
}

extern "C" int bl_localplan_commands(bl_localplan* lp, bl_navfield* nf, const bl_localplan_state_t* states, int n, bl_localplan_result_t* results)
{
    lp_args a;
    bool staged = false;
    int rc = lp_prepare(lp, nf, states, n, &a, &staged);
    if (rc) return rc;
    BL_CHECK_ARG(n == 0 || results != nullptr);
    if (n == 0) return BL_OK;
    bl_ctx* ctx = lp->ctx;
    BL_HIP(hipSetDevice(ctx->device));
    const size_t ob = (size_t)n * sizeof(bl_localplan_result_t);
    rc = bl_grow(&lp->d_out, &lp->d_out_cap, ob, false, ctx);
    if (!rc) rc = bl_grow(&lp->h_out, &lp->h_out_cap, ob, true, ctx);
    if (!rc) rc = lp_upload(lp, states, n, &a);
    if (rc) return rc;
    BL_HIP(hipEventRecord(lp->ev0, ctx->stream));
    rc = lp_launch_rollout(lp, a, n, staged);
    if (rc) return rc;
    hipLaunchKernelGGL(k_lp_finish, dim3((n + 63) / 64), dim3(64), 0, ctx->stream, a, n, (bl_localplan_result_t*)lp->d_out);
    BL_HIP(hipGetLastError());
    BL_HIP(hipEventRecord(lp->ev1, ctx->stream));
    BL_HIP(hipMemcpyAsync(lp->h_out, lp->d_out, ob, hipMemcpyDeviceToHost, ctx->stream));
    BL_HIP(hipStreamSynchronize(ctx->stream));
    memcpy(results, lp->h_out, ob);
    BL_HIP(hipEventElapsedTime(&lp->last_ms, lp->ev0, lp->ev1));
    lp->timed = true;
    return BL_OK;
}

extern "C" int bl_localplan_debug_costs(bl_localplan* lp, bl_navfield* nf, const bl_localplan_state_t* state, int64_t* out)
{
    lp_args a;
    bool staged = false;
    BL_CHECK_ARG(state != nullptr && out != nullptr);
    int rc = lp_prepare(lp, nf, state, 1, &a, &staged);
    if (rc) return rc;
    bl_ctx* ctx = lp->ctx;
    BL_HIP(hipSetDevice(ctx->device));
    const size_t ob = (size_t)a.n_v * a.n_w * 8;
    rc = bl_grow(&lp->d_out, &lp->d_out_cap, ob, false, ctx);
    if (!rc) rc = bl_grow(&lp->h_out, &lp->h_out_cap, ob, true, ctx);
    if (!rc) rc = lp_upload(lp, state, 1, &a);
    if (rc) return rc;
    a.costs = (long long*)lp->d_out;
    rc = lp_launch_rollout(lp, a, 1, staged);
    if (rc) return rc;
    BL_HIP(hipMemcpyAsync(lp->h_out, lp->d_out, ob, hipMemcpyDeviceToHost, ctx->stream));
    BL_HIP(hipStreamSynchronize(ctx->stream));
    memcpy(out, lp->h_out, ob);
    return BL_OK;
}

extern "C" int bl_localplan_debug_rollout(bl_localplan* lp, bl_navfield* nf, const bl_localplan_state_t* state, int c, bl_pose_xyt_t* out)
{
    lp_args a;
    bool staged = false;
    BL_CHECK_ARG(state != nullptr && out != nullptr);
    int rc = lp_prepare(lp, nf, state, 1, &a, &staged);
    if (rc) return rc;
    BL_CHECK_ARG(c >= 0 && c < a.n_v * a.n_w);
    bl_ctx* ctx = lp->ctx;
    BL_HIP(hipSetDevice(ctx->device));
    const size_t ob = (size_t)a.n_steps * sizeof(bl_pose_xyt_t);
    rc = bl_grow(&lp->d_out, &lp->d_out_cap, ob, false, ctx);
    if (!rc) rc = bl_grow(&lp->h_out, &lp->h_out_cap, ob, true, ctx);
    if (!rc) rc = lp_upload(lp, state, 1, &a);
    if (rc) return rc;
    hipLaunchKernelGGL(k_lp_poses, dim3(1), dim3(64), 0, ctx->stream, a, c, (bl_pose_xyt_t*)lp->d_out);
    BL_HIP(hipGetLastError());
    BL_HIP(hipMemcpyAsync(lp->h_out, lp->d_out, ob, hipMemcpyDeviceToHost, ctx->stream));
    BL_HIP(hipStreamSynchronize(ctx->stream));
    memcpy(out, lp->h_out, ob);
    return BL_OK;
}

// what the moving calls check beyond lp_prepare, and the tracker's share of the launch arguments
static int lp_prepare_moving(bl_localplan* lp, bl_navfield* nf, bl_obstracks* tr, const bl_localplan_moving_t* m, const bl_localplan_state_t* states,
                             int n, lp_args* a, bool* staged)
{
    BL_CHECK_ARG(tr != nullptr && m != nullptr);
    int rc = lp_moving_check(m);
    if (!rc) rc = lp_prepare(lp, nf, states, n, a, staged);
    if (!rc) rc = lp_prepare_tracks(lp->ctx, nf, tr, m, &a->m);
    return rc;
}

// the path of the first state that was rolled out; 2 when none was
static int lp_mpath_of(const int* mpath, int n)
{
    for (int i = 0; i < n; ++i) if (mpath[i] >= 0) return mpath[i];
    return 2;
}

extern "C" int bl_localplan_commands_moving(bl_localplan* lp, bl_navfield* nf, bl_obstracks* tr, const bl_localplan_moving_t* m,
                                            const bl_localplan_state_t* states, int n, bl_localplan_result_t* results)
{
    lp_args a;
    bool staged = false;
    int rc = lp_prepare_moving(lp, nf, tr, m, states, n, &a, &staged);
    if (rc) return rc;
    BL_CHECK_ARG(n == 0 || results != nullptr);
    if (n == 0) return BL_OK;
    bl_ctx* ctx = lp->ctx;
    BL_HIP(hipSetDevice(ctx->device));
    const size_t rb = (size_t)n * sizeof(bl_localplan_result_t), ob = rb + (size_t)n * 4;   // results | the states' moving paths
    rc = bl_grow(&lp->d_out, &lp->d_out_cap, ob, false, ctx);
    if (!rc) rc = bl_grow(&lp->h_out, &lp->h_out_cap, ob, true, ctx);
    if (!rc) rc = lp_upload(lp, states, n, &a);
    if (rc) return rc;
    a.mpath = (int*)((char*)lp->d_out + rb);
    BL_HIP(hipEventRecord(lp->ev0, ctx->stream));
    rc = lp_launch_rollout_moving(lp, a, n, staged);
    if (rc) return rc;
    hipLaunchKernelGGL(k_lp_finish, dim3((n + 63) / 64), dim3(64), 0, ctx->stream, a, n, (bl_localplan_result_t*)lp->d_out);
    BL_HIP(hipGetLastError());
    BL_HIP(hipEventRecord(lp->ev1, ctx->stream));
    BL_HIP(hipMemcpyAsync(lp->h_out, lp->d_out, ob, hipMemcpyDeviceToHost, ctx->stream));
    BL_HIP(hipStreamSynchronize(ctx->stream));
    memcpy(results, lp->h_out, rb);
    lp->last_mpath = lp_mpath_of((const int*)((const char*)lp->h_out + rb), n);
    BL_HIP(hipEventElapsedTime(&lp->last_ms, lp->ev0, lp->ev1));
    lp->timed = true;
    return BL_OK;
}

extern "C" int bl_localplan_debug_costs_moving(bl_localplan* lp, bl_navfield* nf, bl_obstracks* tr, const bl_localplan_moving_t* m,
                                               const bl_localplan_state_t* state, int64_t* costs, int32_t* first_hit)
{
    lp_args a;
    bool staged = false;
    BL_CHECK_ARG(state != nullptr);
    int rc = lp_prepare_moving(lp, nf, tr, m, state, 1, &a, &staged);
    if (rc) return rc;
    bl_ctx* ctx = lp->ctx;
    BL_HIP(hipSetDevice(ctx->device));
    const size_t nc = (size_t)a.n_v * a.n_w, ob = nc * 12 + 4;            // costs | first hits | the moving path
    rc = bl_grow(&lp->d_out, &lp->d_out_cap, ob, false, ctx);
    if (!rc) rc = bl_grow(&lp->h_out, &lp->h_out_cap, ob, true, ctx);
    if (!rc) rc = lp_upload(lp, state, 1, &a);
    if (rc) return rc;
    a.costs = (long long*)lp->d_out;
    a.first_hit = (int*)((char*)lp->d_out + nc * 8);
    a.mpath = a.first_hit + nc;
    rc = lp_launch_rollout_moving(lp, a, 1, staged);
    if (rc) return rc;
    BL_HIP(hipMemcpyAsync(lp->h_out, lp->d_out, ob, hipMemcpyDeviceToHost, ctx->stream));
    BL_HIP(hipStreamSynchronize(ctx->stream));
    if (costs) memcpy(costs, lp->h_out, nc * 8);
    if (first_hit) memcpy(first_hit, (const char*)lp->h_out + nc * 8, nc * 4);
    lp->last_mpath = *(const int*)((const char*)lp->h_out + nc * 12);
    return BL_OK;
}

extern "C" int bl_localplan_debug_moving_path(const bl_localplan* lp) { return lp ? lp->last_mpath : -1; }

extern "C" int bl_localplan_debug_path(const bl_localplan* lp) { return lp ? lp->last_path : -1; }

extern "C" int bl_localplan_last_device_ms(const bl_localplan* lp, float* ms)
{
    BL_CHECK_ARG(lp != nullptr && ms != nullptr);
    if (!lp->timed) { bl_set_error("bl_localplan_last_device_ms: no bl_localplan_commands yet"); return BL_ERR_STATE; }
    *ms = lp->last_ms;
    return BL_OK;
}
