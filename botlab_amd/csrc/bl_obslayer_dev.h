// bl_obslayer_dev.h -- what the obstacle layer (bl_obslayer.hip) shares with the obstacle tracks (bl_obstracks.hip): the rule by which
// a cell is live, the layer's handle, and the layer's row-major list of live cells as stream-ordered work that waits for nothing
// on the host.
#ifndef BL_OBSLAYER_DEV_H
#define BL_OBSLAYER_DEV_H

#include "bl_internal.h"

struct obs_live_rule { uint32_t n, ttl, min_hits; };
__device__ __forceinline__ bool obs_live(const obs_live_rule& q, uint32_t count, uint32_t last)
{
    return count >= q.min_hits && last != 0u && q.n - last < q.ttl;
}

struct bl_obslayer {
    bl_ctx* ctx;
    int W, H;
    bl_obslayer_params_t params; bool have_params;
    uint32_t n;
    uint8_t* d_count; uint32_t* d_last; uint32_t* d_hit; uint32_t* d_clr;
    float* d_rays; uint8_t* d_classes; int ray_cap;         // ranges | thetas, ray_cap each
    float* h_rays;                                          // pinned, the same layout
    int4* d_rows; int* d_totals;
    int32_t* d_xy; int xy_cap;
    int last_rays, last_valid;                              // of the last update (0 after a reset)
    bool sets_valid;                                        // the stamps speak of update n (not after a reset or an upload)
    bool updated, composed, staged;
    hipEvent_t ev_stage, ev_ua, ev_ub, ev_ca, ev_cb;
};

// bl_obslayer.hip: the layer's readers' three launches (k_obs_rowcount, k_obs_rowscan, k_obs_livewrite) on the ctx stream, nothing
// copied back: the first min(cap, live cells) x, y pairs in row-major order to d_xy (device, room for cap pairs), the number of live
// cells to ol->d_totals[0] (device).  The layer has its parameters.
int obs_live_list_enqueue(bl_obslayer* ol, int32_t* d_xy, int cap);

#endif  // BL_OBSLAYER_DEV_H
