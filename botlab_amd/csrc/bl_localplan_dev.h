// bl_localplan_dev.h -- what the two local planners share: bl_localplan.hip rolls out constant arcs and bl_mppi.hip sampled control
// sequences, over the same navigation field, by the same rules (include/botlab_hip.h, "local planner"); each rule lives here once.
//   device  the moving rule ("local planner, moving obstacles": used slots, the clamped box, the floor division of the offsets, the
//           margin) and the second half of the slot compaction; the flags of the pose's own cell; the window (corner, staging loop,
//           cost of a visited cell); the end score; the unicycle step; the order of the integer keys and their reduction over a
//           workgroup and over a state's workgroups
//   host    the checks and the launch arguments that follow from the field (lp_prepare_field) and from the tracker (lp_moving_check,
//           lp_prepare_tracks), the state check, and the window's share of the dynamic LDS
// What differs stays in the two files: how a rollout's controls come about, the arc planner's (cos, sin) phases and box table, the
// sampling planner's averaging, and each kernel's LDS layout and barriers.
#ifndef BL_LOCALPLAN_DEV_H
#define BL_LOCALPLAN_DEV_H

#include <math.h>

#include "bl_internal.h"
#include "bl_navfield_dev.h"

#define LP_THREADS 256                 // both rollout kernels: a lane per tracker slot, LP_WAVES wave slots in the reduction
#define LP_WAVES (LP_THREADS / 64)
#define LP_COST_NONE 0x7FFFFFFFFFFFFFFFll
#define LP_MOV_POS_MAX (1 << 30)
static_assert(LP_THREADS == BL_OBSTRACKS_MAX_TRACKS, "the moving prologue has a lane per slot");

// what a rollout reads of the field, and what scores its end
struct lp_field {
    const uint32_t* field; const uint16_t* l1; const int32_t* table; int table_n;
    bl_frame frame;
    int win_r;                                    // half side of the staged window
    float dt_sim;
    int w_field, w_heading, w_clear;
    float k_heading;                              // (float)(1024 / pi)
    float move_angle[8];
};

struct lp_partial { long long cost; int c; int n_adm; };   // a workgroup's least (cost, index) key and admissible count

struct lp_mov_div { int q; unsigned int magic; };     // steps_per_update and ceil(2^28 / q): lp_mov_offset

// what the moving rule reads: the tracker's BL_OBSTRACKS_MAX_TRACKS slots and bl_localplan_moving_t
struct lp_moving { const bl_obstrack_t* slots; lp_mov_div mq; int mmargin, mlead; };

// a kept slot: its clamped box widened by the margin, and (vx, vy) as two int16
struct lp_kept { int x0, y0, x1, y1, v; };

// floor((t * v + 128 q) / (256 q)) without a division: floor(n / (256 q)) = floor((n >> 8) / q), and for 0 <= a < 2^20, q < 2^8,
// floor(a / q) = (a * ceil(2^28 / q)) >> 28 (Granlund & Montgomery).  |t * v| <= 510 * 1023, so (n >> 8) + 2048 q lies in [9, 2^20).
__device__ __forceinline__ int lp_mov_offset(int t, int v, lp_mov_div d)
{
    const unsigned int a = (unsigned int)(((t * v + 128 * d.q) >> 8) + 2048 * d.q);   // >> of a negative int: floor
    return (int)(((unsigned long long)a * d.magic) >> 28) - 2048;
}

__device__ __forceinline__ int lp_mov_clamp(int v) { return v < -LP_MOV_POS_MAX ? -LP_MOV_POS_MAX : v > LP_MOV_POS_MAX ? LP_MOV_POS_MAX : v; }

__device__ __forceinline__ bool lp_mov_used(const bl_obstrack_t& t)
{
    return t.id != 0u && (t.flags & (BL_OBSTRACK_CONFIRMED | BL_OBSTRACK_MOVING)) == (BL_OBSTRACK_CONFIRMED | BL_OBSTRACK_MOVING) &&
           (t.flags & (BL_OBSTRACK_MATCHED | BL_OBSTRACK_BORN)) != 0;
}

__device__ __forceinline__ lp_kept lp_mov_record(const bl_obstrack_t& t, int margin)
{
    lp_kept r;
    r.x0 = lp_mov_clamp(t.x0) - margin; r.y0 = lp_mov_clamp(t.y0) - margin;
    r.x1 = lp_mov_clamp(t.x1) + margin; r.y1 = lp_mov_clamp(t.y1) + margin;
    const int vx = min(max(t.vx, -1023), 1023), vy = min(max(t.vy, -1023), 1023);   // what every update and upload leaves; lp_mov_offset's domain
    r.v = (vx & 0xffff) | (int)((unsigned int)vy << 16);
    return r;
}

// is (ex, ey) inside the record's box at time t (rollout step + lead)
__device__ __forceinline__ bool lp_mov_in_box(const lp_kept& r, int t, lp_mov_div q, int ex, int ey)
{
    const int ox = lp_mov_offset(t, (int)(short)(r.v & 0xffff), q), oy = lp_mov_offset(t, r.v >> 16, q);
    return ex >= r.x0 + ox && ex <= r.x1 + ox && ey >= r.y0 + oy && ey <= r.y1 + oy;
}

// a visited cell outside the reach square (the bound is floating point): every used slot, straight from the tracker
__device__ __noinline__ bool lp_mov_hit_all(const bl_obstrack_t* __restrict__ slots, int margin, int t, lp_mov_div q, int ex, int ey)
{
    for (int sl = 0; sl < BL_OBSTRACKS_MAX_TRACKS; ++sl) {
        const bl_obstrack_t tr = slots[sl];
        if (lp_mov_used(tr) && lp_mov_in_box(lp_mov_record(tr, margin), t, q, ex, ey)) return true;
    }
    return false;
}

__device__ __forceinline__ bool lp_key_less(long long ca, int ia, long long cb, int ib) { return ca < cb || (ca == cb && ia < ib); }

// The slot compaction's second half.  The first is the caller's: a lane per slot decides `keep`, mask = __ballot(keep), lane 0 of
// wave w writes __popcll(mask) to s_cnt[w], and a barrier follows.  Here the kept records go to s_kept in slot order; returns how many.
__device__ __forceinline__ int lp_mov_compact(const int* s_cnt, unsigned long long mask, bool keep, const lp_kept& rec, lp_kept* s_kept)
{
    const int tid = threadIdx.x;
    int base = 0, kept = 0;
    for (int w = 0; w < LP_WAVES; ++w) {
        if (w < (tid >> 6)) base += s_cnt[w];
        kept += s_cnt[w];
    }
    if (keep) s_kept[base + __popcll(mask & ((1ull << (tid & 63)) - 1ull))] = rec;
    return kept;
}

// the flags of the pose's own cell
__device__ __forceinline__ int lp_start_flags(const lp_field& f, const bl_localplan_state_t& st)
{
    const int W = f.frame.width, H = f.frame.height;
    int cx = 0, cy = 0;
    if (!nav_pose_cell(f.frame, st.pose.x, st.pose.y, &cx, &cy)) return BL_LOCALPLAN_OFF_FIELD;
    if (nav_cost(f.l1, f.table, f.table_n, W, H, cx, cy) < 0) return BL_LOCALPLAN_OFF_FIELD;
    const uint32_t v = f.field[(size_t)cy * W + cx];
    if (v == NAV_UNREACHED) return BL_LOCALPLAN_OFF_FIELD;
    return v == 0 ? BL_LOCALPLAN_REACHED : 0;
}

// the corner of the square of half side r about the window's centre: the pose's cell, or (for the debug calls of a pose off the grid)
// the grid cell nearest to it
__device__ __forceinline__ void lp_window_corner(const bl_frame& f, const bl_pose_xyt_t& pose, int r, int* x0, int* y0)
{
    const double vx = ((double)pose.x - (double)f.ox) * (double)f.cpm, vy = ((double)pose.y - (double)f.oy) * (double)f.cpm;
    const int ccx = (int)fmin(fmax(vx, 0.0), (double)(f.width - 1)), ccy = (int)fmin(fmax(vy, 0.0), (double)(f.height - 1));
    *x0 = ccx - r; *y0 = ccy - r;
}

// the window at (wx0, wy0) staged as int16, by all LP_THREADS threads
__device__ __forceinline__ void lp_stage_window(const lp_field& f, int16_t* s_win, int wx0, int wy0)
{
    const int side = 2 * f.win_r + 1;
    for (int idx = threadIdx.x; idx < side * side; idx += LP_THREADS)
        s_win[idx] = (int16_t)nav_cost(f.l1, f.table, f.table_n, f.frame.width, f.frame.height, wx0 + idx % side, wy0 + idx / side);
}

// the cost of a visited cell (-1 or the penalty): from the staged window where it covers the cell, else from the grids
template <bool STAGED>
__device__ __forceinline__ int lp_cell_cost(const lp_field& f, const int16_t* s_win, int wx0, int wy0, int ex, int ey)
{
    const int side = 2 * f.win_r + 1;
    const int ux = ex - wx0, uy = ey - wy0;
    if (STAGED && (unsigned)ux < (unsigned)side && (unsigned)uy < (unsigned)side) return s_win[uy * side + ux];
    return nav_cost(f.l1, f.table, f.table_n, f.frame.width, f.frame.height, ex, ey);
}

// The score of a rollout that ended in cell (ex, ey) at heading theta with the summed penalty pen, into *score; false, and no score,
// when it was rejected on the way (!ok) or ends where the field does not reach: the caller's cost stays LP_COST_NONE.  Two things are
// the way they are for the code the compiler makes of them: a flag and not the LP_COST_NONE value comes back, which
// k_lp_rollout would have to compare again, and (W, H), f.frame's, are read by the caller before its loop over the steps, as
// nav_cost's callers do: read here, behind the loop, they cost k_mppi_rollout<false, *> two VGPRs.
__device__ __forceinline__ bool lp_end_score(const lp_field& f, int W, int H, bool ok, int ex, int ey, float theta, int pen, long long* score)
{
    uint32_t fe = NAV_UNREACHED;
    if (ok) fe = f.field[(size_t)ey * W + ex];
    if (fe == NAV_UNREACHED) return false;
    int h = 0;
    if (fe != 0) {
        uint32_t to_f;
        const int bm = nav_descent_move(f.field, f.l1, f.table, f.table_n, W, H, ex, ey, &to_f);
        if (bm < 0) h = 1024;
        else {
            const float d = (float)bl_angle_diff((double)theta, (double)f.move_angle[bm]);
            h = (int)floorf(fabsf(d) * f.k_heading);
        }
    }
    *score = (long long)f.w_field * (long long)fe + (long long)f.w_heading * h + (long long)f.w_clear * pen;
    return true;
}

// one unicycle step: s the arc length and dth the turn of a step
__device__ __forceinline__ void lp_unicycle_step(float& x, float& y, float& theta, float s, float dth)
{
    float sn, cs;
    bl_sincosf(theta, &sn, &cs);
    x = x + s * cs;
    y = y + s * sn;
    theta = bl_wrap_to_pi(theta + dth);
}

// The least key and the admissible count of a workgroup, written to *out by thread 0: no atomics, no floats.  All LP_THREADS threads
// call it (one barrier); s_cost, s_c and s_n hold LP_WAVES entries each.
__device__ __forceinline__ void lp_block_best(long long cost, int c, int adm, long long* s_cost, int* s_c, int* s_n, lp_partial* out)
{
    const int tid = threadIdx.x;
    for (int off = 32; off > 0; off >>= 1) {
        const long long oc = __shfl_xor(cost, off);
        const int oi = __shfl_xor(c, off);
        adm += __shfl_xor(adm, off);
        if (lp_key_less(oc, oi, cost, c)) { cost = oc; c = oi; }
    }
    if ((tid & 63) == 0) { s_cost[tid >> 6] = cost; s_c[tid >> 6] = c; s_n[tid >> 6] = adm; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < LP_WAVES; ++w) {
            if (lp_key_less(s_cost[w], s_c[w], cost, c)) { cost = s_cost[w]; c = s_c[w]; }
            adm += s_n[w];
        }
        lp_partial p;
        p.cost = cost; p.c = c; p.n_adm = adm;
        *out = p;
    }
}

// the least key and the admissible count of a state, over its workgroups' slots p[0 .. bps)
__device__ __forceinline__ void lp_state_best(const lp_partial* p, int bps, long long* cost, int* c, int* adm)
{
    *cost = LP_COST_NONE; *c = 0x7FFFFFFF; *adm = 0;
    for (int b = 0; b < bps; ++b) {
        if (lp_key_less(p[b].cost, p[b].c, *cost, *c)) { *cost = p[b].cost; *c = p[b].c; }
        *adm += p[b].n_adm;
    }
}

// ---------------------------------------------------------------------------------------------------------------- host
static int lp_state_ok(const bl_localplan_state_t* s, int n)
{
    for (int i = 0; i < n; ++i) {
        BL_CHECK_ARG(isfinite(s[i].pose.x) && isfinite(s[i].pose.y) && isfinite(s[i].pose.theta) && isfinite(s[i].v) && isfinite(s[i].w));
        BL_CHECK_ARG(!(fabsf(s[i].pose.theta) > BL_LOCALPLAN_MAX_THETA));             // every accepted heading wraps within bl_wrap_to_pi's guard
    }
    return BL_OK;
}

// What every call that sees the field checks once the planner (`who` in the texts, on ctx) has parameters, and what follows from the
// field and from them: rollouts of `steps` steps of dt_sim at speeds within [v_min, v_max].  *reach_r is R of the window rule.
static int lp_prepare_field(const char* who, bl_ctx* ctx, const bl_navfield* nf, int n, bool have_states, float v_min, float v_max, float dt_sim,
                            int steps, int w_field, int w_heading, int w_clear, lp_field* f, int* reach_r, bool* staged)
{
    if (!nf->valid) { bl_set_error("navigation field not computed (bl_navfield_compute first)"); return BL_ERR_STATE; }
    BL_CHECK_ARG(nf->ctx == ctx);
    BL_CHECK_ARG(n >= 0 && (n == 0 || have_states));
    bl_dist_host_view v;
    int rc = bl_dist_view_host(nf->dist, &v);
    if (rc) return rc;
    if (v.l1 != nf->l1 || v.frame.width != nf->frame.width || v.frame.height != nf->frame.height || v.table_n != nf->table_n) {
        bl_set_error("%s: the distance grid was resized since the field was computed", who);
        return BL_ERR_STATE;
    }
    const double vabs = fmax(fabs((double)v_min), fabs((double)v_max));
    if (vabs * (double)dt_sim > (double)nf->frame.mpc) {
        bl_set_error("%s: a step of %g m can skip a cell of %g m", who, vabs * (double)dt_sim, (double)nf->frame.mpc);
        return BL_ERR_ARG;
    }
    f->field = nf->field; f->l1 = nf->l1; f->table = nf->table; f->table_n = nf->table_n;
    f->frame = nf->frame;
    f->dt_sim = dt_sim;
    f->w_field = w_field; f->w_heading = w_heading; f->w_clear = w_clear;
    const int R = (int)ceil(vabs * (double)dt_sim * steps * (double)nf->frame.cpm) + 2;
    *staged = (long long)(2 * R + 1) * (2 * R + 1) * 2 <= (long long)BL_LOCALPLAN_WINDOW_BYTES;
    f->win_r = *staged ? R : 0;
    *reach_r = R;
    f->k_heading = (float)(1024.0 / BL_PI);
    const double ang[8] = {0.0, BL_PI, BL_PI / 2, -BL_PI / 2, BL_PI / 4, 3 * BL_PI / 4, -BL_PI / 4, -3 * BL_PI / 4};
    for (int m = 0; m < 8; ++m) f->move_angle[m] = (float)ang[m];
    return BL_OK;
}

// the moving side comes in two steps, because every entry point checks bl_localplan_moving_t before it looks at the field and the
// tracker after: the ranges ...
static int lp_moving_check(const bl_localplan_moving_t* m)
{
    BL_CHECK_ARG(m->steps_per_update >= 1 && m->steps_per_update <= 255);
    BL_CHECK_ARG(m->margin_cells >= 0 && m->margin_cells <= BL_LOCALPLAN_MAX_MARGIN);
    BL_CHECK_ARG(m->lead_steps >= 0 && m->lead_steps <= 255);
    BL_CHECK_ARG(m->reserved == 0);
    return BL_OK;
}

// ... and the tracker's view and its share of the launch arguments
static int lp_prepare_tracks(bl_ctx* ctx, const bl_navfield* nf, const bl_obstracks* tr, const bl_localplan_moving_t* m, lp_moving* out)
{
    bl_obstracks_view v;
    bl_obstracks_view_host(tr, &v);
    BL_CHECK_ARG(v.ctx == ctx && v.W == nf->frame.width && v.H == nf->frame.height);
    if (!v.have_params) { bl_set_error("obstacle tracks have no parameters (bl_obstracks_set_params first)"); return BL_ERR_STATE; }
    out->slots = v.d_slots;
    out->mq.q = m->steps_per_update; out->mq.magic = (unsigned int)(((1u << 28) + (unsigned int)m->steps_per_update - 1u) / (unsigned int)m->steps_per_update);
    out->mmargin = m->margin_cells; out->mlead = m->lead_steps;
    return BL_OK;
}

// the window's share of the dynamic LDS
static size_t lp_window_lds(const lp_field& f, bool staged)
{
    const int side = 2 * f.win_r + 1;
    return staged ? (((size_t)side * side * 2 + 15) & ~(size_t)15) : 0;
}

#endif  // BL_LOCALPLAN_DEV_H
