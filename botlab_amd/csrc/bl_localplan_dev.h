// bl_localplan_dev.h -- what the kernels that roll out against moving obstacles share: the moving rule of include/botlab_hip.h,
// "local planner, moving obstacles" (used slots, the clamped box, the floor division of the offsets, the margin) and the order of the
// integer keys.  bl_localplan.hip rolls out constant arcs and bl_mppi.hip sampled sequences; the rule lives here once.
#ifndef BL_LOCALPLAN_DEV_H
#define BL_LOCALPLAN_DEV_H

#include "bl_internal.h"

#define LP_MOV_POS_MAX (1 << 30)

struct lp_mov_div { int q; unsigned int magic; };     // steps_per_update and ceil(2^28 / q): lp_mov_offset

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

#endif  // BL_LOCALPLAN_DEV_H
