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
#include <math.h>
#include <string.h>

#include "bl_internal.h"
#include "bl_navfield_dev.h"
#include "bl_localplan_dev.h"

#define LP_THREADS 256
#define LP_TRIG_SLOTS 2048             // (cos, sin) pairs of a workgroup: jpb * (n_steps + 1) of them, the last of each j holds theta_end
#define LP_RED_BYTES 64                // per wave: key cost (8), key c (4), admissible count (4)
#define LP_LDS_FIXED (LP_TRIG_SLOTS * 8 + LP_RED_BYTES)
#define LP_COST_NONE 0x7FFFFFFFFFFFFFFFll
#define LP_MOV_KEPT_BYTES (BL_OBSTRACKS_MAX_TRACKS * 20)                  // lp_kept: five words per kept slot
#define LP_MOV_BYTES (LP_MOV_KEPT_BYTES + BL_LOCALPLAN_MOVING_BYTES)
static_assert(LP_THREADS == BL_OBSTRACKS_MAX_TRACKS, "the moving prologue has a lane per slot");
// two workgroups with the largest window and the moving block fit a CU's 160 KiB
static_assert(2 * (LP_LDS_FIXED + BL_LOCALPLAN_WINDOW_BYTES + 16 + LP_MOV_BYTES) <= 160 * 1024, "BL_LOCALPLAN_MOVING_BYTES too large");

struct lp_partial { long long cost; int c; int n_adm; };

struct lp_args {
    const uint32_t* field; const uint16_t* l1; const int32_t* table; int table_n;
    bl_frame frame;
    const bl_localplan_state_t* states;
    const float* v_tab; const float* w_tab;      // [state][n_v], [state][n_w]
    int n_v, n_w, n_steps;
    int nvp, jpb, bps;                            // lanes per heading (a power of two >= n_v), headings and workgroups per state
    float dt_sim;
    int w_field, w_heading, w_clear, w_speed;
    int win_r;                                    // half side of the staged window
    lp_partial* partial;                          // [state][bps]
    long long* costs;                             // bl_localplan_debug_costs: every candidate's cost (one state); else null
    float k_heading;                              // (float)(1024 / pi)
    float move_angle[8];
    // MOVING only
    const bl_obstrack_t* slots;                   // the tracker's BL_OBSTRACKS_MAX_TRACKS slots
    lp_mov_div mq; int mmargin, mlead;            // bl_localplan_moving_t
    int reach_r;                                  // R of the window rule, staged or not
    int mov_off;                                  // where the moving block starts in the dynamic LDS
    int* first_hit;                               // bl_localplan_debug_costs_moving: per candidate; else null
    int* mpath;                                   // [state]: 0 table, 1 per step, 2 nothing kept, -1 not rolled out (the state's first workgroup writes it)
};

// the flags of the pose's own cell; (cx, cy) its cell where it has one
__device__ __forceinline__ int lp_start_flags(const lp_args& a, const bl_localplan_state_t& st, int* cx, int* cy)
{
    const int W = a.frame.width, H = a.frame.height;
    if (!nav_pose_cell(a.frame, st.pose.x, st.pose.y, cx, cy)) return BL_LOCALPLAN_OFF_FIELD;
    if (nav_cost(a.l1, a.table, a.table_n, W, H, *cx, *cy) < 0) return BL_LOCALPLAN_OFF_FIELD;
    const uint32_t f = a.field[(size_t)*cy * W + *cx];
    if (f == NAV_UNREACHED) return BL_LOCALPLAN_OFF_FIELD;
    return f == 0 ? BL_LOCALPLAN_REACHED : 0;
}

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
    const int W = a.frame.width, H = a.frame.height;
    const bl_localplan_state_t st = a.states[state];
    int scx = 0, scy = 0;
    const int flags = lp_start_flags(a, st, &scx, &scy);
    if (flags && !a.costs) {                                         // nothing is rolled out (uniform over the workgroup)
        if (MOVING && blk == 0 && tid == 0) a.mpath[state] = -1;
        return;
    }
    // the window's centre: the pose's cell, or (for the debug costs of a pose off the grid) the grid cell nearest to it
    const int side = 2 * a.win_r + 1;
    int wx0 = 0, wy0 = 0;
    int rx0 = 0, ry0 = 0;                                             // MOVING: the reach square's corner, its side 2 * reach_r + 1
    if (STAGED || MOVING) {
        const double vx = ((double)st.pose.x - (double)a.frame.ox) * (double)a.frame.cpm, vy = ((double)st.pose.y - (double)a.frame.oy) * (double)a.frame.cpm;
        const int ccx = (int)fmin(fmax(vx, 0.0), (double)(W - 1)), ccy = (int)fmin(fmax(vy, 0.0), (double)(H - 1));
        wx0 = ccx - a.win_r; wy0 = ccy - a.win_r;
        rx0 = ccx - a.reach_r; ry0 = ccy - a.reach_r;
    }
    // MOVING prologue, first half: a lane per slot decides used and can-reach; the waves' counts go where the reduction's will
    lp_kept* s_kept = (lp_kept*)(s_raw + a.mov_off);
    short4* s_box = (short4*)(s_raw + a.mov_off + LP_MOV_KEPT_BYTES);
    const int rside = 2 * a.reach_r;
    bool keep = false, used = false;
    lp_kept rec;
    unsigned long long keep_mask = 0ull;
    if (MOVING) {
        const bl_obstrack_t tr = a.slots[tid];
        used = lp_mov_used(tr);
        rec = lp_mov_record(tr, a.mmargin);
        if (used) {
            // the displacement is monotone in k per axis: the two ends bound the sweep
            const int vx = (int)(short)(rec.v & 0xffff), vy = rec.v >> 16;
            const int ox1 = lp_mov_offset(1 + a.mlead, vx, a.mq), oxn = lp_mov_offset(a.n_steps + a.mlead, vx, a.mq);
            const int oy1 = lp_mov_offset(1 + a.mlead, vy, a.mq), oyn = lp_mov_offset(a.n_steps + a.mlead, vy, a.mq);
            const long long lx = (long long)rec.x0 + min(ox1, oxn), hx = (long long)rec.x1 + max(ox1, oxn);
            const long long ly = (long long)rec.y0 + min(oy1, oyn), hy = (long long)rec.y1 + max(oy1, oyn);
            keep = hx >= (long long)rx0 && lx <= (long long)rx0 + rside && hy >= (long long)ry0 && ly <= (long long)ry0 + rside;
        }
        keep_mask = __ballot(keep);
        const unsigned long long used_mask = __ballot(used);
        if ((tid & 63) == 0) { s_n[tid >> 6] = __popcll(keep_mask); s_c[tid >> 6] = __popcll(used_mask); }
    }
    if (STAGED) {
        for (int idx = tid; idx < side * side; idx += LP_THREADS)
            s_win[idx] = (int16_t)nav_cost(a.l1, a.table, a.table_n, W, H, wx0 + idx % side, wy0 + idx / side);
    }
    // A: the headings of this workgroup's j
    const int stride = a.n_steps + 1;
    const int j0 = blk * a.jpb;
    if (tid < a.jpb && j0 + tid < a.n_w) {
        float theta = bl_wrap_to_pi(st.pose.theta);
        const float dth = a.w_tab[(size_t)state * a.n_w + j0 + tid] * a.dt_sim;
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
        int base = 0;
        for (int w = 0; w < LP_THREADS / 64; ++w) {
            if (w < (tid >> 6)) base += s_n[w];
            kept += s_n[w]; n_used += s_c[w];
        }
        if (keep) s_kept[base + __popcll(keep_mask & ((1ull << (tid & 63)) - 1ull))] = rec;
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
                const int t = k + 1 + a.mlead;
                const int ox = lp_mov_offset(t, (int)(short)(r.v & 0xffff), a.mq), oy = lp_mov_offset(t, r.v >> 16, a.mq);
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
        const float s = a.v_tab[(size_t)state * a.n_v + i] * a.dt_sim;
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
            if (!nav_pose_cell(a.frame, x, y, &ex, &ey)) { ok = false; if (all_steps) continue; break; }
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
                        for (int b = 0; b < kept; ++b) hit = hit || lp_mov_in_box(s_kept[b], k + 1 + a.mlead, a.mq, ex, ey);
                    }
                } else hit = lp_mov_hit_all(a.slots, a.mmargin, k + 1 + a.mlead, a.mq, ex, ey);
                if (hit) { hit_k = k + 1; ok = false; if (all_steps) continue; break; }
            }
            if (MOVING && !ok) continue;                              // (all_steps: only the moving test is still wanted)
            int q;
            const int ux = ex - wx0, uy = ey - wy0;
            if (STAGED && (unsigned)ux < (unsigned)side && (unsigned)uy < (unsigned)side) q = s_win[uy * side + ux];
            else q = nav_cost(a.l1, a.table, a.table_n, W, H, ex, ey);
            if (q < 0) { ok = false; if (all_steps) continue; break; }
            pen += q;
        }
        if (all_steps) a.first_hit[c] = hit_k;
        uint32_t fe = NAV_UNREACHED;
        if (ok) fe = a.field[(size_t)ey * W + ex];
        if (fe != NAV_UNREACHED) {
            int h = 0;
            if (fe != 0) {
                uint32_t to_f;
                const int bm = nav_descent_move(a.field, a.l1, a.table, a.table_n, W, H, ex, ey, &to_f);
                if (bm < 0) h = 1024;
                else {
                    const float d = (float)bl_angle_diff((double)row[a.n_steps].x, (double)a.move_angle[bm]);
                    h = (int)floorf(fabsf(d) * a.k_heading);
                }
            }
            cost = (long long)a.w_field * (long long)fe + (long long)a.w_heading * h + (long long)a.w_clear * pen +
                   (long long)a.w_speed * (a.n_v - 1 - i);
            adm = 1;
        }
        if (a.costs) a.costs[c] = cost;
        if (!adm) c = 0x7FFFFFFF;
    }
    // the least key of the workgroup
    for (int off = 32; off > 0; off >>= 1) {
        const long long oc = __shfl_xor(cost, off);
        const int oi = __shfl_xor(c, off);
        adm += __shfl_xor(adm, off);
        if (lp_key_less(oc, oi, cost, c)) { cost = oc; c = oi; }
    }
    if ((tid & 63) == 0) { s_cost[tid >> 6] = cost; s_c[tid >> 6] = c; s_n[tid >> 6] = adm; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < LP_THREADS / 64; ++w) {
            if (lp_key_less(s_cost[w], s_c[w], cost, c)) { cost = s_cost[w]; c = s_c[w]; }
            adm += s_n[w];
        }
        lp_partial p;
        p.cost = cost; p.c = c; p.n_adm = adm;
        a.partial[blockIdx.x] = p;
    }
}

__global__ __launch_bounds__(64) void k_lp_finish(lp_args a, int n_states, bl_localplan_result_t* __restrict__ out)
{
    const int state = blockIdx.x * 64 + threadIdx.x;
    if (state >= n_states) return;
    const bl_localplan_state_t st = a.states[state];
    int cx = 0, cy = 0;
    bl_localplan_result_t r;
    r.trans_v = 0.0f; r.angular_v = 0.0f; r.index = -1; r.n_admissible = 0; r.cost = LP_COST_NONE; r.pad = 0;
    r.flags = lp_start_flags(a, st, &cx, &cy);
    if (r.flags == BL_LOCALPLAN_REACHED) r.cost = 0;
    if (!r.flags) {
        long long cost = LP_COST_NONE;
        int c = 0x7FFFFFFF, adm = 0;
        const lp_partial* p = a.partial + (size_t)state * a.bps;
        for (int b = 0; b < a.bps; ++b) {
            if (lp_key_less(p[b].cost, p[b].c, cost, c)) { cost = p[b].cost; c = p[b].c; }
            adm += p[b].n_adm;
        }
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
    const float s = a.v_tab[c % a.n_v] * a.dt_sim, dth = a.w_tab[c / a.n_v] * a.dt_sim;
    float x = st.pose.x, y = st.pose.y, theta = bl_wrap_to_pi(st.pose.theta);
    for (int k = 0; k < a.n_steps; ++k) {
        float sn, cs;
        bl_sincosf(theta, &sn, &cs);
        x = x + s * cs;
        y = y + s * sn;
        theta = bl_wrap_to_pi(theta + dth);
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

static int lp_grow(void** p, size_t* cap, size_t want, bool host, bl_ctx* ctx)
{
    if (want <= *cap) return BL_OK;
    BL_HIP(hipStreamSynchronize(ctx->stream));
    if (*p) { if (host) BL_HIP(hipHostFree(*p)); else BL_HIP(hipFree(*p)); }
    *p = nullptr; *cap = 0;
    if (host) BL_HIP(hipHostMalloc(p, want, hipHostMallocDefault)); else BL_HIP(hipMalloc(p, want));
    *cap = want;
    return BL_OK;
}

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

static int lp_state_ok(const bl_localplan_state_t* s, int n)
{
    for (int i = 0; i < n; ++i) {
        BL_CHECK_ARG(isfinite(s[i].pose.x) && isfinite(s[i].pose.y) && isfinite(s[i].pose.theta) && isfinite(s[i].v) && isfinite(s[i].w));
        BL_CHECK_ARG(!(fabsf(s[i].pose.theta) > BL_LOCALPLAN_MAX_THETA));             // every accepted heading wraps within bl_wrap_to_pi's guard
    }
    return BL_OK;
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
    if (!nf->valid) { bl_set_error("navigation field not computed (bl_navfield_compute first)"); return BL_ERR_STATE; }
    BL_CHECK_ARG(nf->ctx == lp->ctx);
    BL_CHECK_ARG(n >= 0 && (n == 0 || states != nullptr));
    const bl_localplan_params_t& p = lp->params;
    bl_dist_host_view v;
    int rc = bl_dist_view_host(nf->dist, &v);
    if (rc) return rc;
    if (v.l1 != nf->l1 || v.frame.width != nf->frame.width || v.frame.height != nf->frame.height || v.table_n != nf->table_n) {
        bl_set_error("local planner: the distance grid was resized since the field was computed");
        return BL_ERR_STATE;
    }
    const double vabs = fmax(fabs((double)p.v_min), fabs((double)p.v_max));
    if (vabs * (double)p.dt_sim > (double)nf->frame.mpc) {
        bl_set_error("local planner: a step of %g m can skip a cell of %g m", vabs * (double)p.dt_sim, (double)nf->frame.mpc);
        return BL_ERR_ARG;
    }
    rc = lp_state_ok(states, n);
    if (rc) return rc;
    memset((void*)a, 0, sizeof(*a));
    a->field = nf->field; a->l1 = nf->l1; a->table = nf->table; a->table_n = nf->table_n;
    a->frame = nf->frame;
    a->n_v = p.n_v; a->n_w = p.n_w; a->n_steps = p.n_steps;
    int nvp = 1;
    while (nvp < p.n_v) nvp *= 2;
    a->nvp = nvp;
    int jpb = LP_THREADS / nvp;
    if (jpb > LP_TRIG_SLOTS / (p.n_steps + 1)) jpb = LP_TRIG_SLOTS / (p.n_steps + 1);
    if (jpb > p.n_w) jpb = p.n_w;
    a->jpb = jpb;
    a->bps = (p.n_w + jpb - 1) / jpb;
    a->dt_sim = p.dt_sim;
    a->w_field = p.w_field; a->w_heading = p.w_heading; a->w_clear = p.w_clear; a->w_speed = p.w_speed;
    const int R = (int)ceil(vabs * (double)p.dt_sim * p.n_steps * (double)nf->frame.cpm) + 2;
    *staged = (long long)(2 * R + 1) * (2 * R + 1) * 2 <= (long long)BL_LOCALPLAN_WINDOW_BYTES;
    a->win_r = *staged ? R : 0;
    a->reach_r = R;
    a->k_heading = (float)(1024.0 / BL_PI);
    const double ang[8] = {0.0, BL_PI, BL_PI / 2, -BL_PI / 2, BL_PI / 4, 3 * BL_PI / 4, -BL_PI / 4, -3 * BL_PI / 4};
    for (int m = 0; m < 8; ++m) a->move_angle[m] = (float)ang[m];
    return BL_OK;
}

// states and their tables into the pinned block and on to the device (no synchronisation)
static int lp_upload(bl_localplan* lp, const bl_localplan_state_t* states, int n, lp_args* a)
{
    bl_ctx* ctx = lp->ctx;
    const bl_localplan_params_t& p = lp->params;
    const size_t sb = (size_t)n * sizeof(bl_localplan_state_t), vb = (size_t)n * p.n_v * 4, wb = (size_t)n * p.n_w * 4;
    int rc = lp_grow(&lp->d_in, &lp->d_in_cap, sb + vb + wb, false, ctx);
    if (!rc) rc = lp_grow(&lp->h_in, &lp->h_in_cap, sb + vb + wb, true, ctx);
    if (!rc) rc = lp_grow((void**)&lp->d_partial, &lp->partial_cap, (size_t)n * a->bps * sizeof(lp_partial), false, ctx);
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

// the window's share of the dynamic LDS
static size_t lp_window_lds(const lp_args& a, bool staged)
{
    const int side = 2 * a.win_r + 1;
    return staged ? (((size_t)side * side * 2 + 15) & ~(size_t)15) : 0;
}

static int lp_launch_rollout(bl_localplan* lp, const lp_args& a, int n, bool staged)
{
    bl_ctx* ctx = lp->ctx;
    const size_t lds = LP_LDS_FIXED + lp_window_lds(a, staged);
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
    a.mov_off = (int)(LP_LDS_FIXED + lp_window_lds(a, staged));
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
    rc = lp_grow(&lp->d_out, &lp->d_out_cap, ob, false, ctx);
    if (!rc) rc = lp_grow(&lp->h_out, &lp->h_out_cap, ob, true, ctx);
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
    rc = lp_grow(&lp->d_out, &lp->d_out_cap, ob, false, ctx);
    if (!rc) rc = lp_grow(&lp->h_out, &lp->h_out_cap, ob, true, ctx);
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
    rc = lp_grow(&lp->d_out, &lp->d_out_cap, ob, false, ctx);
    if (!rc) rc = lp_grow(&lp->h_out, &lp->h_out_cap, ob, true, ctx);
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
    BL_CHECK_ARG(m->steps_per_update >= 1 && m->steps_per_update <= 255);
    BL_CHECK_ARG(m->margin_cells >= 0 && m->margin_cells <= BL_LOCALPLAN_MAX_MARGIN);
    BL_CHECK_ARG(m->lead_steps >= 0 && m->lead_steps <= 255);
    BL_CHECK_ARG(m->reserved == 0);
    int rc = lp_prepare(lp, nf, states, n, a, staged);
    if (rc) return rc;
    bl_obstracks_view v;
    bl_obstracks_view_host(tr, &v);
    BL_CHECK_ARG(v.ctx == lp->ctx && v.W == nf->frame.width && v.H == nf->frame.height);
    if (!v.have_params) { bl_set_error("obstacle tracks have no parameters (bl_obstracks_set_params first)"); return BL_ERR_STATE; }
    a->slots = v.d_slots;
    a->mq.q = m->steps_per_update; a->mq.magic = (unsigned int)(((1u << 28) + (unsigned int)m->steps_per_update - 1u) / (unsigned int)m->steps_per_update);
    a->mmargin = m->margin_cells; a->mlead = m->lead_steps;
    return BL_OK;
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
    rc = lp_grow(&lp->d_out, &lp->d_out_cap, ob, false, ctx);
    if (!rc) rc = lp_grow(&lp->h_out, &lp->h_out_cap, ob, true, ctx);
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
    rc = lp_grow(&lp->d_out, &lp->d_out_cap, ob, false, ctx);
    if (!rc) rc = lp_grow(&lp->h_out, &lp->h_out_cap, ob, true, ctx);
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
