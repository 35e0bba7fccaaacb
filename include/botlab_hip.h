/* botlab_hip.h -- C ABI of libbotlab_hip.so: the MI355X (gfx950) implementation of botLab's SLAM / MCL / planning
 * hot path.  Plain C, POD arguments, caller-owned buffers, int status returns (0 = ok), no exceptions, no torch types.
 *
 * Each entry point names the reference interface it stands in for (paths relative to the botLab checkout).  The C++
 * classes in include/botlab/ (OccupancyGrid, Mapping, ParticleFilter, ObstacleDistanceGrid, search_for_path) keep the
 * reference's signatures and forward to these calls; INTEGRATION.md shows the binding.
 *
 * Threading: one bl_ctx per host thread (the reference touches Mapping / ParticleFilter / map_ only from the runSLAM
 * thread, src/slam/slam_main.cpp:56-58).  All work of a ctx is stream-ordered on ONE HIP stream (its own, or a
 * caller-supplied one); calls return after enqueueing unless they hand a result back to host memory, in which case
 * they synchronise that stream first.
 */
#ifndef BOTLAB_HIP_H
#define BOTLAB_HIP_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ status */
#define BL_OK 0
#define BL_ERR_HIP 1        /* a HIP runtime call failed; text in bl_last_error() */
#define BL_ERR_ARG 2        /* bad argument (null handle, shape mismatch, out-of-range parameter) */
#define BL_ERR_CAPACITY 3   /* a device-side work list (A* open list) ran out of its configured capacity */
#define BL_ERR_STATE 4      /* call order violated (e.g. update before init) */

const char* bl_last_error(void);          /* thread-local message of the last failing call */
const char* bl_version(void);

/* ------------------------------------------------------------------ message records (in-memory layout of the
 * lcm-gen structs the reference passes around; field order from the lcmtypes .lcm files) */
typedef struct bl_pose_xyt_t {            /* lcmtypes/pose_xyt_t.lcm:1-8 ; 24 bytes */
    int64_t utime;
    float x, y, theta;
} bl_pose_xyt_t;

typedef struct bl_particle_t {            /* lcmtypes/particle_t.lcm:4-9 ; 56 bytes */
    bl_pose_xyt_t pose;
    bl_pose_xyt_t parent_pose;
    double weight;
} bl_particle_t;

typedef struct bl_lidar_t {               /* lcmtypes/lidar_t.lcm:1-14 ; arrays are HOST pointers, num_ranges long */
    int64_t utime;
    int32_t num_ranges;
    const float* ranges;
    const float* thetas;
    const int64_t* times;
    const float* intensities;             /* may be NULL (unused on the hot path) */
} bl_lidar_t;

typedef struct bl_search_params_t {       /* src/planning/astar.hpp:15-27 */
    double minDistanceToObstacle;
    double maxDistanceWithCost;
    double distanceCostExponent;
} bl_search_params_t;

/* ------------------------------------------------------------------ context */
typedef struct bl_ctx bl_ctx;

/* device: HIP device ordinal.  stream: NULL -> the ctx creates its own non-blocking stream; otherwise a hipStream_t
 * owned by the caller (e.g. torch's current stream, so collectives issued by the caller order with this ctx). */
int bl_ctx_create(int device, void* stream, bl_ctx** out);
void bl_ctx_destroy(bl_ctx* ctx);
int bl_ctx_sync(bl_ctx* ctx);
/* Per-kernel HIP-event timing on the ctx stream (bench.py's roofline leg).  kernel ids: BL_K_* below. */
int bl_ctx_timing_enable(bl_ctx* ctx, int on);   /* 0: off; 1: every kernel; else a bit mask, bit i = kernel id i */
/* Time only every `every`-th launch of each enabled kernel (default 1): an event pair costs ~13 us of stream time per
 * launch on this stack, which would distort a pipelined step. */
int bl_ctx_timing_stride(bl_ctx* ctx, int every);
int bl_ctx_timing_get(bl_ctx* ctx, int kernel_id, double* total_ms, int64_t* launches);
int bl_ctx_timing_reset(bl_ctx* ctx);
#define BL_K_MCL_MAIN 0      /* resample-gather + action + sensor model, one thread per particle */
#define BL_K_MCL_SCAN 1      /* weight prefix scan + pose estimate (3 small launches, timed together) */
#define BL_K_MAP 2           /* Mapping::updateMap */
#define BL_K_DIST 3          /* ObstacleDistanceGrid::setDistances (2 launches, timed together) */
#define BL_K_ASTAR 4         /* search_for_path */
#define BL_K_FRONTIERS 5     /* find_map_frontiers */
/* the launches inside setDistances and the replanner's snapshot copy one by one (timed only when asked for by id: "every
 * kernel" means ids 0..5; an event pair between two kernels costs a few microseconds of stream time) */
#define BL_K_DIST_ROWS 6
#define BL_K_DIST_COLS_SUMMARY 7
#define BL_K_DIST_COLS_APPLY 8
#define BL_K_SNAPSHOT 9
#define BL_K_DIST_FUSED 10   /* the whole-grid transform as one launch (grids of at least 512 x 512, width a multiple of 16) */
#define BL_K_COUNT 11

/* ------------------------------------------------------------------ OccupancyGrid  (src/slam/occupancy_grid.hpp:51-209)
 * Device-resident int8 log-odds cells, row-major y*width+x.  meters_per_cell and cells_per_meter are both carried
 * because the reference carries both (occupancy_grid.cpp:19-36 computes cpm = 1.0f/mpc; loadFromFile :138-175 does
 * not touch cpm). */
typedef struct bl_grid bl_grid;
int bl_grid_create(bl_ctx* ctx, int width, int height, float meters_per_cell, float cells_per_meter,
                   float origin_x, float origin_y, bl_grid** out);       /* cells zeroed (reset(), :48-52) */
void bl_grid_destroy(bl_grid* g);
int bl_grid_upload(bl_grid* g, const int8_t* cells);                     /* host -> device, width*height bytes */
int bl_grid_download(bl_grid* g, int8_t* cells);                         /* device -> host (synchronises) */
int bl_grid_reset(bl_grid* g);                                           /* OccupancyGrid::reset */
int bl_grid_set_frame(bl_grid* g, float meters_per_cell, float cells_per_meter, float origin_x, float origin_y);
int bl_grid_copy(bl_grid* dst, const bl_grid* src);                      /* device -> device, same shape */
void* bl_grid_device_ptr(bl_grid* g);                                    /* int8_t* in HBM */
int bl_grid_shape(const bl_grid* g, int* width, int* height);

/* ------------------------------------------------------------------ Mapping  (src/slam/mapping.hpp:25-34, mapping.cpp:8-127) */
typedef struct bl_mapping bl_mapping;
/* 0 <= hit_odds, miss_odds <= 127 */
int bl_mapping_create(bl_ctx* ctx, float max_laser_distance, int8_t hit_odds, int8_t miss_odds, bl_mapping** out);
void bl_mapping_destroy(bl_mapping* m);
/* Mapping::updateMap(scan, pose, map): first call ever latches the pose and changes no cell (initialized_). */
int bl_mapping_update(bl_mapping* m, const bl_lidar_t* scan, const bl_pose_xyt_t* pose, bl_grid* map);
/* Same, the pose read from device memory (the particle filter's estimate of this step) -- no host round trip. */
int bl_mapping_update_dev_pose(bl_mapping* m, const bl_lidar_t* scan, const void* d_pose /* bl_pose_xyt_t* */,
                               int64_t pose_utime, bl_grid* map);

/* ------------------------------------------------------------------ ParticleFilter  (src/slam/particle_filter.hpp:38-77)
 * Particles [shard_lo, shard_hi) of num_particles live on this device; the exchange record of all num_particles
 * (x, y, theta, weight-units: 16 bytes each) is replicated.  Single GPU: shard = [0, N). */
typedef struct bl_pf bl_pf;
typedef struct bl_dist bl_dist;           /* ObstacleDistanceGrid (below); bl_pf_init_uniform takes one */
int bl_pf_create(bl_ctx* ctx, int num_particles, int shard_lo, int shard_hi, bl_pf** out);
void bl_pf_destroy(bl_pf* pf);
/* Optional, before init: use caller-allocated device buffers for the two exchange records (each at least
 * num_particles*16 B) so a caller can run the all-gather on them in place. */
int bl_pf_set_exchange_buffers(bl_pf* pf, void* d_rec0, void* d_rec1);
void* bl_pf_exchange_rec_ptr(bl_pf* pf);     /* the record written by the last update_begin (all N; own slice filled) */
/* initializeFilterAtPose (particle_filter.cpp:16-34): N(pose, 0.01) per coordinate from a counter-based Philox stream
 * keyed by seed (reference: std::random_device), last particle = pose, weights 1/N. */
int bl_pf_init_at_pose(bl_pf* pf, const bl_pose_xyt_t* pose, uint64_t seed);
/* Global localization: the filter seeded uniformly over the free space of a known map (Monte-Carlo localization from no known
 * start).  A cell is eligible when its log-odds is < 0 (frontiers.hpp:23-24) and, if `dist` is given (same shape as the map, already
 * transformed), when the distance that grid shows for it is > min_dist (keeps the robot's centre off the walls).  Each particle takes
 * an eligible cell uniformly, a uniform offset inside it and a uniform heading; parent pose = pose, equal weights, pose utimes = utime.
 * The cloud depends on (seed, map, dist, min_dist, num_particles) only: Philox keyed by seed and the global particle index, with
 * counter words of its own (exact formulas: bl_mcl.hip, k_pf_init_uniform).  poseEstimate() becomes estimatePosteriorPose of the
 * new cloud (a composed shard: the last particle's pose).  No eligible cell, or a `dist` of another shape: BL_ERR_ARG and the filter
 * is left as it was. */
int bl_pf_init_uniform(bl_pf* pf, const bl_grid* map, const bl_dist* dist /* NULL: log-odds only */, float min_dist, int64_t utime,
                       uint64_t seed);
/* Spread of the posterior (is a filter started by bl_pf_init_uniform converged?), one reduction of fixed order over the current record
 * (u = a particle's weight units, S = sum of u, weights u / S):
 *   units_sum = S; units_sq_hi:units_sq_lo = sum of u^2 as a 128-bit integer; n_eff = (double)S * (double)S / (double)(sum of u^2)
 *   mean_x, mean_y: weighted means;  var_x, var_y, cov_xy: weighted (population) second moments about them;
 *   theta_resultant: mean resultant length R of the heading, |sum of u (cos theta, sin theta)| / S in double (circular std sqrt(-2 ln R)).
 * BL_ERR_STATE while an update is pending and on a composed shard (bl_pf_estimate_posterior_pose's rule).  Synchronises. */
typedef struct bl_pf_spread_t {
    double n_eff, mean_x, mean_y, var_x, var_y, cov_xy, theta_resultant;
    uint64_t units_sum, units_sq_lo, units_sq_hi;
} bl_pf_spread_t;                         /* 80 bytes */
int bl_pf_spread(bl_pf* pf, bl_pf_spread_t* out);
/* Kidnapped-robot recovery (augmented MCL, Probabilistic Robotics 8.3.5): while the measurements stop fitting the cloud, a fraction
 * of the resampled particles is replaced by poses drawn uniformly over the free space of a known map.
 *   Eligible list: a snapshot of the eligible cells of `map` at call time (bl_pf_init_uniform's rule: log-odds < 0 and, with `dist`,
 *     distance > min_dist), in a buffer of the recovery's own.  The tracker starts unprimed, updates = 0.  Calling again rebuilds the
 *     list and resets the tracker; params == NULL turns recovery off and frees the list.
 *   Errors: BL_ERR_ARG for bad parameters, a `dist` of another shape or no eligible cell; BL_ERR_STATE while an update is pending and
 *     on a composed shard or a partial slice (n_local < N).  Either way the filter is left exactly as it was.
 *   Tracking: u counts the moved, sensor-weighted updates since recovery was enabled (1, 2, ...).  At the start of update u the
 *     posterior about to be resampled is folded in, if a sensor update produced it from a scan it did not interpolate: not a
 *     cloud of bl_pf_init_at_pose, bl_pf_init_uniform or bl_pf_set_particles, and not the posterior of an update whose particles
 *     carried a nonzero pose utime -- the first update after an initialisation or upload with utime != 0, which interpolates its
 *     scan towards utime 0 (the reference's MovingLaserScan with ActionModel::utime_ == 0) and scores an order of magnitude low.
 *     An action-only update keeps the weights it moved and so the flag:
 *       w_avg = ((double)S * 0.0005) / (double)N           (S = the posterior's weight units: the mean of max(likelihood, 0.001))
 *       unprimed: w_slow = w_fast = w_avg, primed = 1;  else w_slow = w_slow + alpha_slow * (w_avg - w_slow), w_fast likewise
 *     (plain IEEE double, no contraction).
 *   Injected fraction: p = (primed && w_fast < ratio * w_slow) ? min(max_fraction, 1.0 - w_fast / (ratio * w_slow)) : 0;
 *     t = p >= 1 ? 2^32 : floor(p * 2^32) (a uint64).
 *   Injection: output particle m (global index) is injected iff word 0 of Philox4x32-10((m, u, 0x72637679, 2), seed) < t.  Its prior
 *     (the pose the action model moves and the sensor model weights) is bl_pf_init_uniform's sample over the recovery list, with
 *     counter words (m, u, 0x72637679, 0 / 1) and the recovery seed.  Every other particle takes its resampled source.  All three
 *     resampling rules (integer prefix, strict, equal weights) compose with it.  bl_pf_debug_last reports index -1 for an injected
 *     particle.  Injected particles enter estimatePosteriorPose like any other. */
typedef struct bl_pf_recovery_params_t {
    double alpha_slow, alpha_fast;        /* 0 < alpha_slow < alpha_fast <= 1 (defaults 0.001, 0.1) */
    double ratio;                         /* inject only while w_fast < ratio * w_slow; > 0 and finite */
    double max_fraction;                  /* cap on the injected fraction, in [0, 1] */
    float min_dist;                       /* eligibility as bl_pf_init_uniform: log-odds < 0 and, with dist, distance > min_dist */
    uint64_t seed;
} bl_pf_recovery_params_t;                /* 48 bytes */
int bl_pf_set_recovery(bl_pf* pf, const bl_grid* map, const bl_dist* dist /* NULL: log-odds only */,
                       const bl_pf_recovery_params_t* params /* NULL: off */);
typedef struct bl_pf_recovery_state_t {
    double w_slow, w_fast, w_avg, p_inject;
    uint32_t updates, primed, injected_last, pad;   /* injected_last: particles injected by the last moved update */
    uint64_t injected_total;
} bl_pf_recovery_state_t;                 /* 56 bytes; all zero while recovery is off */
int bl_pf_recovery_state(bl_pf* pf, bl_pf_recovery_state_t* out);   /* synchronises; BL_ERR_STATE while an update is pending */
/* Adaptive particle count (KLD-sampling, Fox 2003; Probabilistic Robotics Table 8.4), off by default.
 *   Capacity = bl_pf_create's num_particles; every buffer stays sized for it.  Inits and uploads fill it: active = next = capacity.
 *   active: particles of the current record (exports, spread, debug_last, the estimate and recovery's w_avg use it).  next: what
 *     the next resampling update draws from the active records, by the usual rule with M = next (U_m = r + m / next); in parity
 *     mode it takes 3 * next noise floats, and bl_pf_debug_resample reports next indices.
 *   The count: after every resampling update, k = distinct bins of its parent poses (injected particles included), a bin being
 *     (floor(x / bin_xy), floor(y / bin_xy), floor(theta / bin_theta)) in double from the float pose, each index clamped to
 *     [-2^20, 2^20 - 1] (NaN: -2^20).  Exact for |x|, |y| < 2^20 bin_xy and |theta| < 2^20 bin_theta.
 *   The bound: for k >= 2, b = 2 / (9 (k - 1)), c = 1 - b + sqrt(b) * z, n = ceil((k - 1) / (2 epsilon) * c * c * c) (plain double);
 *     n = min_particles for k <= 1;  next = min(capacity, max(min_particles, n)).  k_sat = the smallest k in [2, capacity] with
 *     n(k) >= capacity (capacity + 1 if none): the count stops there and reports min(k, k_sat).
 *   Action-only and unmoved updates keep active, next and the count.  Enabling sets next = active; params == NULL turns it off and
 *     the next resampling update draws the capacity.  The first resampling update after a count waits for its 8-byte read-back.
 *   Errors: BL_ERR_ARG for bad parameters; BL_ERR_STATE while an update is pending and on a sharded filter (partial slice, composed
 *     finish, external exchange buffers; bl_pf_shard_setup is refused while it is on).  Either way the filter is left as it was. */
typedef struct bl_pf_adaptive_params_t {
    int32_t min_particles;                /* 2 <= min_particles <= capacity */
    int32_t pad;
    double epsilon;                       /* KLD bound on the error, > 0 */
    double z;                             /* upper standard-normal quantile, > 0 (2.326: the 0.99 quantile) */
    double bin_xy, bin_theta;             /* histogram bin, metres / radians, > 0 */
} bl_pf_adaptive_params_t;                /* 40 bytes */
int bl_pf_set_adaptive(bl_pf* pf, const bl_pf_adaptive_params_t* params /* NULL: off */);
typedef struct bl_pf_adaptive_state_t {
    int32_t active;                       /* particles in the current record */
    int32_t next;                         /* particles the next resampling update will draw */
    uint32_t bins;                        /* k of the last count, saturated at k_sat; 0 if none yet */
    uint32_t k_sat;                       /* 0 while adaptive mode is off */
    uint64_t counts;                      /* resampling updates counted since enabling */
} bl_pf_adaptive_state_t;                 /* 24 bytes */
int bl_pf_adaptive_state(bl_pf* pf, bl_pf_adaptive_state_t* out);   /* synchronises; BL_ERR_STATE while an update is pending */
/* Pose hypotheses: the clusters of the cloud (AMCL's pf_cluster_stats).  The particles [0, active) of the current record are
 * binned, the connected components of the occupied bins are the clusters, and the heaviest ones are reported with exact integer
 * sums.  Everything summed or compared is an integer: the result does not depend on a launch shape or an order of arrival.
 *   Constants, formed once in plain double:  xy_scale = 1024.0 / bin_xy,  th_scale = (double)T / 6.283185307179586  (T = theta_bins).
 *   Per particle (x, y, theta floats, u its weight units):
 *     fine position  px = clamp(floor((double)x * xy_scale), -2^30, 2^30 - 1) as int64 (NaN: -2^30), py likewise;
 *     position bin   ix = px >> 10 (floor), iy likewise -- a bin is bin_xy wide, a fine unit bin_xy / 1024;
 *     heading bin    q = clamp(floor((double)theta * th_scale), -2^40, 2^40 - 1) (NaN: -2^40), it = q mod T in [0, T);
 *     heading terms  (sn, cs) = bl_sincosf(theta) -- glibc's sinf / cosf, bit for bit -- when theta is finite and |theta| < 100,
 *                    else (0, 0);  si = (int64)rint((double)sn * 1048576.0), ci likewise.
 *   Clusters: a bin (ix, iy, it) is occupied when at least one particle falls into it (a particle of 0 units counts).  Two different
 *     occupied bins are adjacent iff |d ix| <= 1, |d iy| <= 1 and d it = -1, 0 or +1 (mod T).  A cluster is a connected component
 *     of the occupied bins under this adjacency.
 *   Per cluster, over its particles: count; units U = sum u; sx = sum u px, sy = sum u py, sxx = sum u px^2, syy = sum u py^2,
 *     sxy = sum u px py, sc = sum u ci, ss = sum u si as signed 128-bit integers (|sxx| can reach 2^112); anchor = the
 *     lexicographically smallest (ix, iy, it) of its bins.
 *   Order: U descending, then anchor ascending (a total order).  The call reports the number of clusters C, the total units S, active,
 *     and the first min(C, max_clusters) clusters; the rest of clusters[] is zero.  labels, if given, takes one int32 per particle:
 *     the rank of its cluster when that rank is < max_clusters, else -1.
 *   Runs on the ctx stream and synchronises.  BL_ERR_ARG for bad parameters; BL_ERR_STATE before an initialisation, while an update is
 *     pending and on a composed shard (bl_pf_spread's rule).  Either way the filter, out and labels are left as they were.
 *     bin_xy, theta_bins and any share threshold a caller puts on the result are untuned knobs. */
#define BL_PF_MAX_CLUSTERS 64
typedef struct bl_pf_cluster_params_t {
    double bin_xy;                        /* position bin, metres: > 0 and finite */
    int32_t theta_bins;                   /* T, heading bins of the full turn: 1 .. 4096 */
    int32_t max_clusters;                 /* K, clusters reported: 1 .. BL_PF_MAX_CLUSTERS */
} bl_pf_cluster_params_t;                 /* 16 bytes */
typedef struct bl_i128_t { uint64_t lo; int64_t hi; } bl_i128_t;       /* value = hi * 2^64 + lo */
typedef struct bl_pf_cluster_t {
    uint64_t count, units;
    bl_i128_t sx, sy, sxx, syy, sxy, sc, ss;
    int32_t anchor_ix, anchor_iy, anchor_it, pad;
} bl_pf_cluster_t;                        /* 144 bytes */
typedef struct bl_pf_clusters_t {
    uint64_t num_clusters;                /* C */
    uint64_t units_sum;                   /* S */
    int32_t active, pad;
    bl_pf_cluster_t clusters[BL_PF_MAX_CLUSTERS];
} bl_pf_clusters_t;                       /* 9240 bytes */
int bl_pf_clusters(bl_pf* pf, const bl_pf_cluster_params_t* params, bl_pf_clusters_t* out, int32_t* labels /* NULL or active ints */);
/* A cluster's pose, in plain double: not part of the byte-equality contract (the library exports the same function for bindings).
 * The position sums are recentred on the anchor bin exactly, in 128-bit integers -- a = 1024 anchor_ix: sx' = sx - a U,
 * sxx' = sxx - 2 a sx + a^2 U, likewise y and the cross term -- and every integer is converted to double once:
 *   share = U / S;  mean_x = (a + sx' / U + 0.5) / xy_scale (the middle of the mean fine unit), mean_y likewise;
 *   var_x = (sxx' / U - (sx' / U)^2) / xy_scale^2, var_y and cov_xy likewise (population moments);
 *   theta = atan2(ss, sc);  theta_resultant = hypot(ss, sc) / (U * 2^20)  (circular std sqrt(-2 ln R)).
 * Returns 1; a cluster of 0 units has no pose: returns 0 and writes nothing. */
typedef struct bl_pf_cluster_pose_t {
    double share, mean_x, mean_y, var_x, var_y, cov_xy, theta, theta_resultant;
} bl_pf_cluster_pose_t;                   /* 64 bytes */
#ifndef BL_PF_HELPER
#define BL_PF_HELPER static inline
#endif
BL_PF_HELPER int bl_pf_cluster_pose(const bl_pf_cluster_t* c, uint64_t units_sum, const bl_pf_cluster_params_t* params,
                                    bl_pf_cluster_pose_t* out)
{
    if (c->units == 0) return 0;
    {
        const double xy_scale = 1024.0 / params->bin_xy;
        const __int128 U = (__int128)c->units, ax = (__int128)1024 * c->anchor_ix, ay = (__int128)1024 * c->anchor_iy;
#define BL_PF_I128(v) ((__int128)(((unsigned __int128)(uint64_t)(v).hi << 64) | (v).lo))
        const __int128 sx = BL_PF_I128(c->sx), sy = BL_PF_I128(c->sy);
        const __int128 rx = sx - ax * U, ry = sy - ay * U;
        const __int128 rxx = BL_PF_I128(c->sxx) - 2 * ax * sx + ax * ax * U;
        const __int128 ryy = BL_PF_I128(c->syy) - 2 * ay * sy + ay * ay * U;
        const __int128 rxy = BL_PF_I128(c->sxy) - ax * sy - ay * sx + ax * ay * U;
        const double dU = (double)c->units, mx = (double)rx / dU, my = (double)ry / dU;
        const double dss = (double)BL_PF_I128(c->ss), dsc = (double)BL_PF_I128(c->sc);
#undef BL_PF_I128
        out->share = dU / (double)units_sum;
        out->mean_x = ((double)ax + mx + 0.5) / xy_scale;
        out->mean_y = ((double)ay + my + 0.5) / xy_scale;
        out->var_x = ((double)rxx / dU - mx * mx) / (xy_scale * xy_scale);
        out->var_y = ((double)ryy / dU - my * my) / (xy_scale * xy_scale);
        out->cov_xy = ((double)rxy / dU - mx * my) / (xy_scale * xy_scale);
        out->theta = atan2(dss, dsc);
        out->theta_resultant = hypot(dss, dsc) / (dU * 1048576.0);
    }
    return 1;
}
/* Replace the whole posterior from a host AoS array of num_particles records.  The `weight` fields are not read: the weights are
 * units[m] / sum(units), units == NULL -> uniform (every unit 1).
 *   Legal units: any uint32 values, zeros included, whose total is not 0 (num_particles * (2^32 - 1) < 2^53: the total and every
 *     prefix of it are exact in a double).  A total of 0 would make every weight 0 / 0: BL_ERR_ARG, and the filter keeps what it held.
 *   Resampling: equal units (the host compares them) are resampled against the reference's own rounded cumulative of N weights 1 / N;
 *     any other upload by the integer rule, first i with (r + m / N) * S <= prefix[i], clamped to N - 1 (strict resampling: the
 *     reference's cumulative for every set).
 *   A total of 2 * num_particles units means "every particle at the likelihood floor" (weight 0.001 / wSum in resampling, in the
 *     pose estimate and in what bl_pf_get_particles hands out) ONLY for a record a sensor update wrote, where every unit is at least 2.  An upload with that total -- [1,3,1,3..],
 *     [0,4,0,4..], one unit of 2 N, every unit 2 -- is resampled and estimated with units / S like any other upload. */
int bl_pf_set_particles(bl_pf* pf, const bl_particle_t* particles, const uint32_t* units);
/* particles(): the local shard as lcm particle_t records (synchronises).  weight = units / S; the all-floor set a sensor update
 * leaves has the reference's 0.001 / wSum of its particles (a few ulps from 1 / N), as in resampling and in the estimate. */
int bl_pf_get_particles(bl_pf* pf, bl_particle_t* out_local);
/* noise source of the action model: seed for the Philox stream used when update() gets noise == NULL */
int bl_pf_set_noise_seed(bl_pf* pf, uint64_t seed);

/* updateFilter (particle_filter.cpp:37-52), single GPU or replicated-call form.
 *   rand_value: the value the reference takes from rand() for the low-variance sampler (particle_filter.cpp:92).
 *   noise: NULL -> Philox; else HOST array of 3*num_particles floats (sampledRot1, sampledTrans, sampledRot2 per
 *          output particle, global index order) -- the parity mode.
 *   out_pose may be NULL (pose stays on device, see bl_pf_pose_device_ptr). */
int bl_pf_update(bl_pf* pf, const bl_pose_xyt_t* odometry, const bl_lidar_t* scan, const bl_grid* map, int rand_value,
                 const float* noise, bl_pose_xyt_t* out_pose);
/* Sharded form: begin enqueues action + sensor model for the shard and fills its slice of the exchange record; the
 * caller then all-gathers the record (the ONLY collective of an update); end scans the weight units of all N particles
 * and forms the pose estimate from the gathered record, in an addition order that depends on N alone -- every rank, and
 * every shard count, gets the identical estimate.  *moved == 0 -> nothing was enqueued (robot did not move). */
int bl_pf_update_begin(bl_pf* pf, const bl_pose_xyt_t* odometry, const bl_lidar_t* scan, const bl_grid* map,
                       int rand_value, const float* noise, int* moved);
int bl_pf_update_end(bl_pf* pf, bl_pose_xyt_t* out_pose);
/* updateFilterActionOnly (particle_filter.cpp:54-65) */
int bl_pf_update_action_only(bl_pf* pf, const bl_pose_xyt_t* odometry, const float* noise, bl_pose_xyt_t* out_pose);
int bl_pf_pose_estimate(bl_pf* pf, bl_pose_xyt_t* out_pose);              /* poseEstimate() (synchronises) */
const void* bl_pf_pose_device_ptr(bl_pf* pf);                             /* bl_pose_xyt_t in HBM */
/* estimatePosteriorPose(posterior_) (particle_filter.cpp:144-160) of the particles as they stand (all N on this device or
 * replicated): x / y the reference's serially rounded float sums, bit for bit; becomes poseEstimate().  out_pose may be NULL. */
int bl_pf_estimate_posterior_pose(bl_pf* pf, bl_pose_xyt_t* out_pose);
/* diagnostics of the last estimate, eight values: for the x sum, then for the y sum -- sub-tiles replayed generically, phases
 * of those replays, sub-tiles stepped through by their table, gaps walked the slow way (bl_serial_sum.h, bl_mcl_finish.h) */
int bl_pf_debug_estimate_stats(bl_pf* pf, uint32_t* out8);
/* map updates that ran ahead of the filter's exact pose (bl_mapping_update_finishing_filter) since the filter was created,
 * and those of them that had to run again because a ray's cells differed under the exact pose */
int bl_pf_debug_lookahead(bl_pf* pf, uint32_t out[2]);
int bl_pf_debug_set_finish_generation(bl_pf* pf, uint32_t generation);   /* tests: the record tags of the finish launches wrap every 256 launches */
/* Resampling rule.  The update's resampler compares U_m * S with an exact integer prefix of the weight units; the reference
 * (particle_filter.cpp:84-103) compares U_m with a sequentially rounded double sum of the normalised weights.  The two agree unless
 * U_m falls within that sum's rounding error of a partial sum -- measured: never for weights an update leaves behind
 * (tests/test_gpu_resample_sweep.py, tests/test_gpu_config3_1m.py).  The one kind of weights on which they did part ways is ALL EQUAL
 * weights -- a fresh filter's, an upload's, and the set an update leaves when EVERY particle ends at the likelihood floor (a lost filter:
 * the total is then exactly 2 N units): rand() <= ~1000 or == RAND_MAX puts every U_m on a partial sum, and about half of the particles
 * took the neighbouring source.  All three are recognised (the first two by the host, the all-floor set on the device by the launch that
 * writes the total) and resampled against the reference's own cumulative, which has a closed form for equal weights (a few runs of
 * constant increment per binade: bl_mcl_finish.h, uni_seg) -- on one device and on composed shards alike, at no cost to other updates.
 * BOTLAB_NO_AUTO_STRICT=1: the integer rule there too (tests).  bl_pf_debug_uniform_runs: the number of runs in force (0: the weights
 * of the record are not known to be equal; synchronises).
 * Strict mode (off by default): EVERY finish is followed by the launches that form the reference's cumulative bit
 * for bit and the resampler searches that one: identical indices for every rand() value, at ~50 us per update at 100k particles,
 * ~140 us at 1M (three launches: the chunks' sums with the binade predicted from the integer prefix, one wave walking the chunks'
 * records with the true sum, the chunks filled in side by side) behind the finish -- also behind the map kernel that carries it
 * (bl_mapping_update_finishing_pf): a 100k-particle SLAM step is 140 us instead of 90. */
int bl_pf_debug_uniform_runs(bl_pf* pf, int* out_runs);
int bl_pf_set_strict_resampling(bl_pf* pf, int on);
/* resamplePosteriorDistribution alone (particle_filter.cpp:84-103): the source index each output particle would take for this
 * rand() value, by the very search the update kernel runs; num_particles entries (whole set on this device; synchronises) */
int bl_pf_debug_resample(bl_pf* pf, int rand_value, int32_t* out_idx);
/* diagnostics for the parity tests: resample source index and raw likelihood (half-units) of the local shard of the last
 * update; recorded only while enabled (8 B per particle of extra stores) */
int bl_pf_debug_enable(bl_pf* pf, int on);
/* The hardware measurement behind the sensor model's fast trigonometry (SensorModel::scoreRay's endpoint cells,
 * sensor_model.cpp:34-38).  The ray loop takes the direction of pose.theta - ray theta by the addition theorems from the
 * particle's and the ray's (cos, sin) pairs: maxima of |that - the reference's sinf / cosf of wrap_to_pi(fl(p - r))| over `pairs`
 * random (p, r), p in [-pi, pi], r in [0, 6.2831], with the functions the loop calls (Monte Carlo: the pairs are 2^48); *eps_used
 * is the bound the kernel's guard band is built on (both maxima must stay below it). */
int bl_debug_trig_addition_probe(bl_ctx* ctx, uint64_t pairs, uint32_t seed, float* max_sin_err, float* max_cos_err, float* eps_used,
                                 uint64_t* pairs_checked);
int bl_pf_debug_last(bl_pf* pf, int32_t* resample_idx, int32_t* likelihood_half_units);

/* ------------------------------------------------------------------ correlative scan matching (no reference counterpart)
 * The pose of a scan against the map from the scan alone (Olson, "Real-time correlative scan matching", ICRA 2009, in its
 * exhaustive single-resolution form): the scan is rasterised at every candidate heading, slid over the map in whole cells, and
 * the best-scoring (di, dj, dk) of a bounded window around a centre pose c wins.  Every score is an exact integer.
 *   Valid rays: range > 0.15f (moving_laser_scan.cpp:24) and range < max_range; at most 4096 of them.
 *   Heading dk: theta_k = c.theta + (float)dk * dtheta in float; ray angle a = wrap_to_pi(theta_k - thetas[r])
 *     (moving_laser_scan.cpp:33); cosf / sinf the C library's.
 *   Endpoint cell of ray r at heading dk, SensorModel::scoreRay's float arithmetic and truncating conversion
 *     (sensor_model.cpp:28-40) with s = global_position_to_grid_position(c):
 *       ex = (int)(range * cosf(a) * cellsPerMeter + s.x),  ey = (int)(range * sinf(a) * cellsPerMeter + s.y);
 *     a float sum that is NaN or at least 2^30 in magnitude has no cell (the ray counts nothing).
 *   Score: score(di, dj, dk) = sum over the valid rays of max(0, L[ey + dj][ex + di]), L the int8 log-odds, a cell outside the
 *     grid counting 0: translation is a whole-cell shift of the rasterised scan, not a re-rounding per shift.
 *   Best candidate: the highest score; ties go to the smallest di*di + dj*dj, then the smallest |dk|, then the smallest dk, dj,
 *     di -- one 64-bit key per candidate, so the maximum does not depend on the order of reduction.  An empty or all-free map
 *     returns the centre.
 *   A motion prior, a covariance estimate and a sub-cell pose are bl_scanmatch_match_prior's ("correlative scan matching with a
 *   prior", below the wide match).  Windows beyond the limits below, up to the whole map, are
 *   bl_scanmatch_match_wide's (further down), which prunes. */
typedef struct bl_scan_match_params_t {
    int32_t nx, ny;          /* half window in cells: shifts di in [-nx, nx], dj in [-ny, ny];   0 <= nx, ny <= 64   */
    int32_t ntheta;          /* half window in heading steps: dk in [-ntheta, ntheta];           0 <= ntheta <= 180  */
    float   dtheta;          /* heading step in radians, > 0                                                          */
    float   max_range;       /* rays with range >= max_range are skipped (no return)                                  */
    int32_t min_score;       /* a best score below this is "no match": the pose is the centre, accepted = 0           */
    int32_t keep_volume;     /* != 0: keep the whole score volume on the device for bl_scanmatch_volume (tests, tools)*/
} bl_scan_match_params_t;    /* 28 bytes */
typedef struct bl_scan_match_result_t {
    bl_pose_xyt_t pose;      /* accepted: x = (float)((double)c.x + di * (double)meters_per_cell), y likewise with dj,
                                theta = wrap_to_pi(theta_dk); otherwise the centre's x, y, theta as given; utime = the scan's */
    int32_t di, dj, dk;      /* the best candidate (also when it is not accepted) */
    int32_t score;           /* of the best candidate */
    int32_t score_centre;    /* of (0, 0, 0): what the match gained */
    int32_t ties;            /* candidates sharing the best score (1 = unique) */
    int32_t rays_used;
    int32_t accepted;        /* score >= min_score */
} bl_scan_match_result_t;    /* 56 bytes */
typedef struct bl_scanmatch bl_scanmatch;
int bl_scanmatch_create(bl_ctx* ctx, bl_scanmatch** out);           /* buffers grow on demand up to the limits above */
void bl_scanmatch_destroy(bl_scanmatch* sm);
/* One stream-ordered sequence on the ctx stream (the map must belong to the same ctx); synchronises to hand the result back.
 * BL_ERR_ARG: a limit above exceeded, dtheta <= 0 (or NaN), a null pointer, more than 4096 valid rays. */
int bl_scanmatch_match(bl_scanmatch* sm, const bl_grid* map, const bl_lidar_t* scan, const bl_pose_xyt_t* centre,
                       const bl_scan_match_params_t* params, bl_scan_match_result_t* result);
/* scores[2 ntheta + 1][2 ny + 1][2 nx + 1] of the last match; BL_ERR_STATE if it was not kept -- a call of bl_scanmatch_match that
 * was refused counts as the last match and keeps nothing (synchronises) */
int bl_scanmatch_volume(bl_scanmatch* sm, int32_t* scores);
/* diagnostic: which scoring path the last match took -- 0 the map window staged in LDS, 1 the grid read directly (the window
 * the scan's endpoints and the shifts span does not fit in LDS); -1 before the first match */
int bl_scanmatch_debug_path(const bl_scanmatch* sm);

/* The wide match: the definition above word for word -- valid rays, headings, endpoint cells, score(di, dj, dk), score_centre,
 * rays_used, accepted, the pose -- over windows up to the whole map: 0 <= nx, ny <= 4096, 0 <= ntheta <= 720, at most 4096 valid
 * rays, dtheta > 0.  It returns exactly what scoring every candidate returns, and gets there by pruning (Olson's multi-resolution
 * speed-up, one pooled level).  With P the positive part of the map (0 outside the grid), B = 2^block_log2 and
 * M[y][x] = max P[y .. y+B-1][x .. x+B-1], the block of shifts di in [i0, i0+B), dj in [j0, j0+B) at heading dk has
 * bound = sum over the valid rays of M[ey + j0][ex + i0] >= every score of the block.  With L the exact score of any candidate
 * (here: the best of the centre and of each heading's best-bounded block), every candidate scoring >= L lies in a block with
 * bound >= L; those blocks are scored exactly, so the winner, its tie-break and `ties` are those of the exhaustive form.
 *   Best candidate: the same total order -- highest score; then smallest di*di + dj*dj, |dk|, dk, dj, di -- as a two-word key (a
 *     score is below 2^20), so the maximum does not depend on the order of reduction.
 *   ties: candidates of the whole window sharing the best score, saturating at INT32_MAX.  When no block's bound is above 0 the
 *     answer is known without scoring: the centre, score 0, ties = the window's candidate count (saturated).
 *   block_log2: 0 = the library chooses (8 x 8, grown until the bounds, one int32 per heading and block, stay within 2^26 blocks =
 *     256 MiB); otherwise 1 .. 6, refused with BL_ERR_ARG if its bounds exceed that budget.
 *   exhaustive != 0: every candidate is scored with the same key and no pruning (a yardstick for tests and tools); refused with
 *     BL_ERR_ARG above 2^31 candidates.
 * A flat landscape (L = 0 under positive bounds) prunes nothing and costs what the exhaustive form costs; it is never wrong.
 * One stream-ordered sequence on the ctx stream; synchronises to hand the result back.  BL_ERR_ARG (a limit exceeded, a null
 * pointer, a map of another ctx) changes nothing, the statistics of the last wide match included. */
typedef struct bl_scan_match_wide_params_t {
    int32_t nx, ny;          /* half window in cells, 0 <= nx, ny <= 4096 */
    int32_t ntheta;          /* half window in heading steps, 0 <= ntheta <= 720 */
    float   dtheta;          /* heading step in radians, > 0 */
    float   max_range;       /* rays with range >= max_range are skipped */
    int32_t min_score;       /* a best score below this is "no match" */
    int32_t block_log2;      /* 0, or 1 .. 6 */
    int32_t exhaustive;      /* != 0: no pruning */
} bl_scan_match_wide_params_t;   /* 32 bytes */
typedef struct bl_scan_match_wide_stats_t {
    int64_t candidates;          /* of the window */
    int64_t blocks;              /* per heading ceil((2 nx + 1) / B) * ceil((2 ny + 1) / B) */
    int64_t blocks_kept;         /* blocks with bound >= L (exhaustive: all) */
    int64_t candidates_scored;   /* exact scores computed: the kept blocks' candidates, the seed blocks' and the centre */
    int32_t block_log2;          /* used */
    int32_t path;                /* exact scoring read the map from 0: LDS (the whole grid fits), 1: the grid */
} bl_scan_match_wide_stats_t;    /* 40 bytes */
int bl_scanmatch_match_wide(bl_scanmatch* sm, const bl_grid* map, const bl_lidar_t* scan, const bl_pose_xyt_t* centre,
                            const bl_scan_match_wide_params_t* params, bl_scan_match_result_t* result);
/* of the last wide match that was not refused; BL_ERR_STATE before the first */
int bl_scanmatch_wide_stats(const bl_scanmatch* sm, bl_scan_match_wide_stats_t* out);

/* Correlative scan matching with a prior: bl_scanmatch_match's definition -- valid rays, headings, endpoint cells,
 * score(di, dj, dk), the window limits (nx, ny <= 64, ntheta <= 180, at most 4096 valid rays; a score is at most
 * 4096 * 127 < 2^19) -- word for word, and on top of it a motion prior on the candidate, a weighted second-moment summary of the
 * whole window (a covariance) and a sub-cell offset of the winner.  Everything that is compared or summed is an integer, so the
 * result does not depend on the launch shape or on the order of any reduction.  The numpy restatement is
 * tests/scan_match_prior_model.py.
 *   Prior, centred on the centre pose c, four integers in 1/256 of a score unit:
 *       pen(di, dj, dk) = (a_xx di^2 + 2 a_xy di dj + a_yy dj^2 + a_tt dk^2) >> 8,  formed in int64.
 *     Limits: 0 <= a_xx, a_yy, a_tt <= 32767, |a_xy| <= 32767, a_xy^2 <= a_xx a_yy (the form is then never negative; the sum
 *     stays below 2^31 and pen below 2^23).  Anything else is BL_ERR_ARG.
 *   Objective: obj = score - pen,  -2^23 < obj < 2^19.
 *   Best candidate: the highest obj, then bl_scanmatch_match's order exactly (smallest di*di + dj*dj, |dk|, dk, dj, di): one
 *     64-bit key with obj + 2^23 in the high word and that order's low word.  result.score is the RAW score of that candidate,
 *     accepted = score >= min_score, ties counts the candidates sharing the best OBJECTIVE, score_centre is the centre's score
 *     (its pen is 0).  With all four coefficients 0 the result equals bl_scanmatch_match's byte for byte.  On an empty or
 *     all-free map obj = -pen and the centre wins by the key alone.
 *   Weights.  half_life, 1 <= half_life <= 2^20, is the number of score units by which the objective must fall for a
 *     candidate's weight to halve.  With d = best_obj - obj >= 0, all divisions integer divisions:
 *       e = d / half_life,  f = d - e half_life,  i = (64 f) / half_life,  w = (e >= 21) ? 0 : (BL_SM_EXP2[i] >> e),
 *     BL_SM_EXP2[i] = floor(2^20 2^(-i/64)), i = 0 .. 63 (below).  The best candidate has w = 2^20.
 *   Moments: ten int64 sums over EVERY candidate of the window with di, dj, dk as the coordinates: s0 = sum w, sx = sum w di,
 *     sy, st, sxx = sum w di di, sxy, syy, sxt, syt, stt.  At most 129 * 129 * 361 < 2^23 candidates * 2^20 * 180^2 < 2^58.
 *   Sub-cell offset, one exact fraction (num, den) per axis (x: di, y: dj, t: dk).  If the axis' half window is at least 1 and
 *     the best candidate is not on that axis' window edge, with o-, o0, o+ the objectives at best - 1, best, best + 1 along the
 *     axis: den = 2 (2 o0 - o- - o+), num = o+ - o- (the vertex of the parabola through the three); if den == 0, or on the edge,
 *     or with a half window of 0, the offset is (0, 1).  o0 is the maximum, so |num / den| <= 1/2. */
#define BL_SM_EXP2_VALUES \
    1048576, 1037280, 1026107, 1015053, 1004119, 993303, 982603, 972019, \
    961548, 951190, 940944, 930808, 920781, 910863, 901051, 891345, \
    881743, 872245, 862849, 853555, 844360, 835265, 826267, 817367, \
    808562, 799852, 791236, 782713, 774282, 765941, 757690, 749529, \
    741455, 733468, 725567, 717751, 710019, 702371, 694805, 687321, \
    679917, 672593, 665348, 658181, 651091, 644077, 637139, 630276, \
    623487, 616770, 610126, 603554, 597053, 590621, 584259, 577965, \
    571740, 565581, 559488, 553462, 547500, 541602, 535768, 529997
static const int32_t BL_SM_EXP2[64] = { BL_SM_EXP2_VALUES };
#define BL_SM_MAX_COEFF 32767
#define BL_SM_MAX_HALF_LIFE (1 << 20)
typedef struct bl_scan_match_prior_t {
    int32_t a_xx, a_xy, a_yy, a_tt;  /* the prior, 1/256 score unit per cell^2 (a_tt: per heading step^2); all 0: no prior */
    int32_t half_life;               /* the weights' temperature; read only when want_moments != 0                          */
    int32_t want_moments;            /* != 0: fill the moments (stores the objective volume and runs two more kernels)      */
} bl_scan_match_prior_t;     /* 24 bytes */
typedef struct bl_scan_match_moments_t {
    int64_t s0, sx, sy, st, sxx, sxy, syy, sxt, syt, stt;
    int32_t best_obj;        /* objective of the best candidate */
    int32_t pen_best;        /* its penalty: result.score == best_obj + pen_best */
    int32_t sub_num[3];      /* sub-cell offset of the best candidate along x, y, t: sub_num[a] / sub_den[a] of a cell / step */
    int32_t sub_den[3];      /* never 0 */
} bl_scan_match_moments_t;   /* 112 bytes */
/* One stream-ordered sequence on the ctx stream (rasteriser, scoring, result; with want_moments the moments pass and its
 * reduction behind them), one synchronisation to hand the results back.  want_moments == 0: half_life is not read, moments may
 * be NULL (it is left alone), no volume is stored unless params->keep_volume asks.  After a call with keep_volume or
 * want_moments bl_scanmatch_volume returns the OBJECTIVE volume (with a zero prior: the scores).  BL_ERR_ARG -- a limit of
 * bl_scanmatch_match, a coefficient out of range, a_xy^2 > a_xx a_yy, want_moments with half_life outside 1 .. 2^20 or with
 * moments == NULL, a null pointer -- changes nothing: a kept volume stays. */
int bl_scanmatch_match_prior(bl_scanmatch* sm, const bl_grid* map, const bl_lidar_t* scan, const bl_pose_xyt_t* centre,
                             const bl_scan_match_params_t* params, const bl_scan_match_prior_t* prior,
                             bl_scan_match_result_t* result, bl_scan_match_moments_t* moments);
/* Two helpers for callers, in plain double: not part of the byte-equality contract (the library exports the same two functions
 * for bindings).
 * The weighted mean and covariance of the window.  mean[3]: the offset of the weighted mean from the centre pose, x and y in
 * metres, theta in radians (sx / s0 * meters_per_cell, ..., st / s0 * dtheta).  cov[6] = xx, xy, yy, xt, yt, tt:
 * cov_ab = (s_ab / s0 - (s_a / s0) (s_b / s0)) * scale_a scale_b with scale = meters_per_cell for x and y, dtheta for t.
 * s0 >= 2^20 after any match; a record with s0 <= 0 (never filled) gives zeros. */
#ifndef BL_SM_HELPER
#define BL_SM_HELPER static inline
#endif
BL_SM_HELPER void bl_scanmatch_covariance(const bl_scan_match_moments_t* m, double meters_per_cell, double dtheta, double* mean,
                                          double* cov)
{
    int i;
    for (i = 0; i < 3; ++i) mean[i] = 0.0;
    for (i = 0; i < 6; ++i) cov[i] = 0.0;
    if (m->s0 <= 0) return;
    {
        const double s0 = (double)m->s0, mx = (double)m->sx / s0, my = (double)m->sy / s0, mt = (double)m->st / s0;
        mean[0] = mx * meters_per_cell; mean[1] = my * meters_per_cell; mean[2] = mt * dtheta;
        cov[0] = ((double)m->sxx / s0 - mx * mx) * (meters_per_cell * meters_per_cell);
        cov[1] = ((double)m->sxy / s0 - mx * my) * (meters_per_cell * meters_per_cell);
        cov[2] = ((double)m->syy / s0 - my * my) * (meters_per_cell * meters_per_cell);
        cov[3] = ((double)m->sxt / s0 - mx * mt) * (meters_per_cell * dtheta);
        cov[4] = ((double)m->syt / s0 - my * mt) * (meters_per_cell * dtheta);
        cov[5] = ((double)m->stt / s0 - mt * mt) * (dtheta * dtheta);
    }
}
/* The matched pose moved by the sub-cell offsets: x = (float)(c.x + (di + num_x / den_x) * meters_per_cell), y likewise,
 * theta = the float (float)(c.theta + (dk + num_t / den_t) * dtheta) wrapped into [-pi, pi] as wrap_to_pi does (compared with
 * the double pi, stepped by the double 2 pi, narrowed on every step); utime = result's.  A match that was not accepted gives
 * result->pose, i.e. the centre. */
BL_SM_HELPER void bl_scanmatch_refined_pose(const bl_scan_match_result_t* result, const bl_scan_match_moments_t* m,
                                            const bl_pose_xyt_t* centre, double meters_per_cell, double dtheta, bl_pose_xyt_t* out)
{
    *out = result->pose;
    if (!result->accepted) return;
    {
        const double pi = 3.14159265358979323846;
        const double fx = (double)m->sub_num[0] / (double)m->sub_den[0], fy = (double)m->sub_num[1] / (double)m->sub_den[1];
        const double ft = (double)m->sub_num[2] / (double)m->sub_den[2];
        float th = (float)((double)centre->theta + ((double)result->dk + ft) * dtheta);
        int guard = 0;
        out->x = (float)((double)centre->x + ((double)result->di + fx) * meters_per_cell);
        out->y = (float)((double)centre->y + ((double)result->dj + fy) * meters_per_cell);
        while ((double)th < -pi && guard++ < 64) th = (float)((double)th + 2.0 * pi);
        while ((double)th > pi && guard++ < 64) th = (float)((double)th - 2.0 * pi);
        out->theta = th;
    }
}

/* ------------------------------------------------------------------ ObstacleDistanceGrid  (src/planning/obstacle_distance_grid.hpp:28-96) */
int bl_dist_create(bl_ctx* ctx, bl_dist** out);
void bl_dist_destroy(bl_dist* d);
/* setDistances(map), obstacle_distance_grid.cpp:73-91.  When `map` is a later state of the very map `d` last transformed --
 * Mapping::updateMap calls in between, nothing else; a replanner snapshot counts as the map it was taken from -- only the window
 * those updates can influence is transformed again (grids of at least 1024 cells a side); the result is the full transform's,
 * bit for bit.  BOTLAB_DIST_NO_INCREMENTAL=1 always transforms the whole grid. */
int bl_dist_set_distances(bl_dist* d, const bl_grid* map);
int bl_dist_forget(bl_dist* d);             /* the next bl_dist_set_distances transforms the whole map, whatever d holds now */
/* diagnostic, six counts: setDistances calls that went out as an incremental launch / as a whole-grid launch / found the map
 * unchanged; and of the incremental launches those the device ended with nothing to do / a window / the whole grid */
int bl_dist_debug_stats(bl_dist* d, int64_t* out6);
/* diagnostic: the bound D (an upper bound of every finite L1 distance of the grid, in cells) the next incremental transform
 * dilates its window by, and whether it has been formed (the whole-grid kernels leave none; the first incremental transform
 * after one forms it) */
int bl_dist_debug_bound(bl_dist* d, int* formed, unsigned int* bound);
/* diagnostic, the one-launch whole-grid transform (grids of 512 x 512 .. 4096 x 4096 cells, width a multiple of 16): workgroups
 * that gave up waiting for another tile's summary (never, unless the device is broken: the next bl_dist_set_distances then
 * returns BL_ERR_STATE), and tile summaries a workgroup computed in place of one that had not started yet.
 * BOTLAB_DIST_FUSED_TEST_DELAY=<n> holds every second workgroup back at its start (tests of that path). */
int bl_dist_debug_fused(bl_dist* d, int64_t* out2);
int bl_dist_download(bl_dist* d, float* cells);                           /* width*height floats (synchronises) */
int bl_dist_shape(const bl_dist* d, int* width, int* height);
int bl_dist_frame(const bl_dist* d, float* meters_per_cell, float* cells_per_meter, float* origin_x, float* origin_y);
/* float* in HBM.  A replan never needs the floats (the search reads the integer distances), so they are only formed for callers
 * that ask: bl_dist_download / bl_dist_gather on demand, and -- once this pointer has been handed out -- with every later
 * bl_dist_set_distances on `d`, on d's stream behind the transform, so that a caller who keeps the pointer keeps reading the
 * current transform.  (NULL before the first request on a grid that has never been transformed.) */
void* bl_dist_device_ptr(bl_dist* d);

/* ------------------------------------------------------------------ Euclidean distance grid  (no counterpart in the reference)
 * The grid above is the reference's: an L1 transform shown as 0.1 per cell whatever the cell size.  The search keeps it.  A grid
 * made by bl_dist_create_euclidean is the exact Euclidean transform in metres, capped at max_cells = R cells (1 .. 254):
 *   Sources are the cells with log-odds >= 0 (those of bl_dist_set_distances); off-grid cells are no sources.
 *   d2(c)   = min over sources s of (x_c - x_s)^2 + (y_c - y_s)^2, exact integers
 *   code(c) = d2(c) when d2(c) <= R^2, else FAR = R^2 + 1; 0xFFFF for every cell when the map has no source (uint16)
 *   f[k]    = (float)(sqrt((double)k) * (double)meters_per_cell), k = 0 .. R^2 + 1: the table has R^2 + 2 entries
 *   The float view (bl_dist_download, bl_dist_gather, bl_dist_device_ptr) is f[code], -1.0f for 0xFFFF.  f[FAR] is a LOWER BOUND of
 *   a far cell's distance, not its distance.
 * It is an ordinary bl_dist handle: bl_dist_set_distances transforms the whole map every time (no incremental form:
 * bl_dist_debug_stats counts `full`, bl_dist_debug_bound reports "not formed", bl_dist_forget changes nothing), the grid limits are
 * bl_dist's own.  The navigation field, the local planner over such a field and the path shortcut take it; bl_navfield_compute*
 * returns BL_ERR_ARG when maxDistanceWithCost > minDistanceToObstacle and maxDistanceWithCost > f[R^2] (a penalty would be priced
 * from the far bound).  Everything else that takes a bl_dist is defined on the L1 grid and returns BL_ERR_ARG for a Euclidean one:
 * bl_astar_search*, bl_plan_path_to_frontier, bl_pf_init_uniform, bl_pf_set_recovery. */
#define BL_DIST_L1 0
#define BL_DIST_EUCLIDEAN 1
#define BL_EDT_MAX_CELLS 254
int bl_dist_create_euclidean(bl_ctx* ctx, int max_cells, bl_dist** out);   /* max_cells outside 1 .. 254: BL_ERR_ARG */
int bl_dist_metric(const bl_dist* d, int* metric, int* max_cells);         /* L1 grids: BL_DIST_L1, 0 */
int bl_dist_download_codes(bl_dist* d, uint16_t* out);                     /* n(c) of either metric, width * height words (synchronises) */
/* the float table the codes index, after a transform: *n = width + height + 1 entries for an L1 grid, R^2 + 2 for a Euclidean one;
 * f may be NULL */
int bl_dist_table(const bl_dist* d, float* f, int* n);

/* ------------------------------------------------------------------ search_for_path  (src/planning/astar.hpp:58-61, astar.cpp:9-274)
 * out_path[0] is always the start pose; *out_len == 1 means "no path" (lcmtypes/robot_path_t.lcm:7).  If the path is
 * longer than cap, *out_len is the full length and only cap poses are written.  stats (optional, 2 x int64): pops,
 * pushes.  open_capacity (nodes) bounds the device open list; 0 -> default. */
int bl_astar_search(bl_ctx* ctx, const bl_dist* distances, const bl_pose_xyt_t* start, const bl_pose_xyt_t* goal,
                    const bl_search_params_t* params, bl_pose_xyt_t* out_path, int cap, int* out_len, int64_t* stats);
int bl_astar_set_open_capacity(bl_ctx* ctx, int64_t nodes);
/* Which kernel the last search launched on this ctx took: 2 = k_astar2 (16-bit keys apart from payloads), 1 = k_astar (8-byte entries:
 * a cost table that can take an fCost to -32768 or below, e.g. maxDistanceWithCost > 16.4 m at the reference's d * 2000, or an odd
 * distanceCostExponent > 1), 0 = no search yet.  Diagnostics for the parity tests. */
int bl_astar_debug_last_kernel(bl_ctx* ctx);
/* Test entry for the search's open list (std::priority_queue<Node, vector, greater>, astar.cpp:75-76,117-135, as the wave-parallel
 * std::push_heap / std::pop_heap of k_astar2): replays n operations -- keys[i] in [1, 65534]: push (keys[i], pays[i]); keys[i] < 0:
 * pop -- and returns the popped (key, payload) pairs in order.  cfg 0 / 1 / 2: the storage tiers of a lone search, of a
 * co-running search, of the tests (every tier within a few thousand entries).  cycles (optional, 4 x uint64): device cycles and
 * counts of pushes and of pops. */
int bl_debug_heap2_replay(bl_ctx* ctx, const int32_t* keys, const uint32_t* pays, int n, int cfg, int64_t capacity,
                          uint32_t* out_keys, uint32_t* out_pays, int* out_n, uint64_t* cycles);
/* Asynchronous form for step pipelines: enqueue the search, fetch the result later.  Up to 4 searches may be in flight;
 * results are fetched in launch order and fetching waits for that search only (work enqueued after it keeps running). */
int bl_astar_search_async(bl_ctx* ctx, const bl_dist* distances, const bl_pose_xyt_t* start, const bl_pose_xyt_t* goal,
                          const bl_search_params_t* params);
/* Same, the start pose read from device memory (e.g. bl_pf_pose_device_ptr: the estimate of this very step) so a
 * step pipeline needs no host round trip between localisation and replanning; out_path[0] of the result is that pose. */
int bl_astar_search_async_dev_start(bl_ctx* ctx, const bl_dist* distances, const void* d_start /* bl_pose_xyt_t* */,
                                    const bl_pose_xyt_t* goal, const bl_search_params_t* params);
int bl_astar_search_result(bl_ctx* ctx, bl_pose_xyt_t* out_path, int cap, int* out_len, int64_t* stats);

/* ------------------------------------------------------------------ asynchronous replanner
 * The reference's planner is a separate process fed by the maps/poses the SLAM process publishes
 * (src/planning/exploration.cpp:300-317).  bl_planner is the same arrangement on one device: submit() snapshots the
 * map and the (device-resident) pose on the SLAM ctx's stream and runs setDistances + search_for_path on a second
 * stream, overlapping the next scan's particle filter; fetch() returns results in submission order (up to 2 per lane in
 * flight; submit blocks the SLAM stream, not the host, while both snapshot slots of the lane are still being read). */
typedef struct bl_planner bl_planner;
/* lanes (1..4): consecutive submissions go to consecutive side streams, so up to `lanes` replans run concurrently (each
 * is one wavefront on its own CU and latency-bound; independent searches are what the GPU can overlap). */
int bl_planner_create(bl_ctx* ctx, int lanes, bl_planner** out);
/* batch (1..64): a lane collects `batch` consecutive submissions and issues their searches as ONE launch, a workgroup each,
 * so lanes x batch replans overlap although the runtime multiplexes streams onto four hardware queues.  For grids where a
 * search outlasts a step (2000x2000: ~1.5 ms against 0.2 ms); a result is then available `batch` - 1 submissions later
 * (a fetch that cannot wait for the batch to fill sends it off as it is).  bl_planner_create is batch = 1. */
int bl_planner_create_batched(bl_ctx* ctx, int lanes, int batch, bl_planner** out);
void bl_planner_destroy(bl_planner* p);
int bl_planner_submit(bl_planner* p, const bl_grid* map, const void* d_start_pose /* bl_pose_xyt_t* on the device */,
                      const bl_pose_xyt_t* goal, const bl_search_params_t* params);
int bl_planner_fetch(bl_planner* p, bl_pose_xyt_t* out_path, int cap, int* out_len, int64_t* stats);
/* tests: the cells of the snapshot the latest submission searched (n_cells = width * height of the submitted map) */
int bl_planner_debug_snapshot(bl_planner* p, int8_t* out_cells, int64_t n_cells);
/* End of input (the scan stream pauses, a run ends): sends off the batch every lane is still collecting, so that its work runs beside
 * whatever the SLAM stream still holds instead of behind the fetch that would have sent it.  Results are fetched as ever. */
int bl_planner_flush(bl_planner* p);
/* on: -1 = just read; 0/1 = disable/enable(+reset) HIP-event timing of the planner stream's kernels (totals in ms) */
int bl_planner_timing(bl_planner* p, int on, double* dist_ms, double* astar_ms, int64_t* launches);
/* bl_mapping_update_dev_pose followed by bl_planner_submit(p, map, d_pose, goal, params) as one call: on grids up to
 * 256 K cells the map kernel itself leaves the snapshot behind (one dependent launch less on the SLAM stream). */
int bl_planner_submit_with_map_update(bl_planner* p, bl_mapping* m, const bl_lidar_t* scan, const void* d_pose,
                                      int64_t pose_utime, bl_grid* map, const bl_pose_xyt_t* goal,
                                      const bl_search_params_t* params);
/* updateLocalization + updateMap of one runSLAMIteration (src/slam/slam.cpp:191-207, 262, 279) with the END of the filter
 * update folded into the map kernel: `pf` has an update begun with bl_pf_update_begin, and this call is its
 * bl_pf_update_end(pf, NULL) followed by bl_mapping_update_dev_pose(m, scan, bl_pf_pose_device_ptr(pf), pose_utime, map)
 * -- in ONE launch.  The map kernel's own workgroup forms the pose estimate right before Mapping::updateMap reads it and
 * further workgroups of the launch write the weight prefix meanwhile, so the SLAM stream carries one kernel less per step.
 * A filter with nothing pending (the robot did not move) or whose end cannot ride (sharded particle set) is ended the
 * ordinary way first.  Results are bit-identical to the separate calls. */
/* ------------------------------------------------------------------ particle shards over RCCL  
 * The shards' one collective -- the in-place all-gather of the 16-byte exchange record -- enqueued from this library on the
 * ctx stream, between the two halves of bl_pf_update (bl_pf_update_begin / bl_pf_update_end).  RCCL is not linked: the
 * caller names the librccl.so its process already uses (with PyTorch: torch/lib/librccl.so).  Rendezvous is the caller's:
 * rank 0 makes the id with bl_comm_unique_id, every rank receives its 128 bytes by whatever transport the host has
 * (torch.distributed in botlab_amd/sharded.py) and calls bl_comm_create (collective). */
typedef struct bl_comm bl_comm;
int bl_comm_load(const char* rccl_path);          /* dlopen + symbols only: 0 if the library is usable */
int bl_comm_unique_id(const char* rccl_path, char* out_id128);
int bl_comm_create(bl_ctx* ctx, const char* rccl_path, const char* id128, int rank, int world, bl_comm** out);
void bl_comm_destroy(bl_comm* c);
/* rec: world x per_rank_floats floats, this rank's slice already at its offset (bl_pf_exchange_rec_ptr) */
int bl_comm_all_gather_inplace(bl_comm* c, void* rec, size_t per_rank_floats);

/* Composed finish of a sharded particle set: instead of all-gathering the whole record (N x 16 B into every
 * rank) each rank keeps its own block, reads the resampling sources it needs from their owners' memory, and the end of an
 * update exchanges two SMALL all-gathers -- tile sums (40 B per 512 particles), then sub-tile records + tables (32 B per 128
 * particles + 80 KB) -- before every rank runs the (replicated, ~10 us) chain of estimatePosteriorPose.  Results are the single
 * rank's, bit for bit.  Set-up, once the filter holds particles: bl_pf_shard_setup (block = particles per rank, a multiple of
 * 2048 -- of 512 for fewer than 160 000 particles --, shard = [rank * block, min(N, (rank + 1) * block)) as given to bl_pf_create); hand every rank's three arrays to every
 * rank (bl_pf_shard_local_ptrs -> bl_ipc_export -> the host's transport -> bl_ipc_open -> bl_pf_shard_set_peer; a rank of the
 * same process passes the pointers themselves); bl_pf_shard_commit.  Per update: bl_pf_update_begin, bl_pf_shard_exchange (or
 * bl_pf_shard_stage(1), all-gather of the sums buffer, bl_pf_shard_stage(2), all-gather of the exchange buffer, both in place),
 * then bl_pf_update_end or one of the *_finishing_pf calls.  The all-gathers are what orders a rank's kernels against the other
 * ranks' reads of its memory: every rank must run them, on the filter's stream. */
int bl_dev_enable_peer_access(int device, int peer_device);   /* one process driving several devices (include/botlab/sharded_filter.hpp): kernels of `device` may use `peer_device`'s pointers */
int bl_dev_alloc(bl_ctx* ctx, size_t bytes, void** out);     /* plain zeroed device memory (the probe of botlab_amd/sharded.py) */
int bl_dev_free(void* dev_ptr);
int bl_dev_word(bl_ctx* ctx, void* dev_ptr, int write, uint32_t* value);   /* one word written / read by a kernel of ctx's device (the probe: a peer mapping must be readable by kernels) */
int bl_ipc_export(const void* dev_ptr, char* out_handle64);
int bl_ipc_open(const char* handle64, void** out_dev_ptr);
int bl_ipc_close(void* dev_ptr);
int bl_pf_shard_setup(bl_pf* pf, int rank, int world, int block);
int bl_pf_shard_local_ptrs(bl_pf* pf, void** rec0, void** rec1, void** prefix);
int bl_pf_shard_set_peer(bl_pf* pf, int rank, const void* rec0, const void* rec1, const void* prefix);
int bl_pf_shard_commit(bl_pf* pf);
int bl_pf_shard_buffers(bl_pf* pf, void** sums, size_t* sums_bytes_per_rank, void** xchg, size_t* xchg_bytes_per_rank);
int bl_pf_shard_stage(bl_pf* pf, int stage);
int bl_pf_shard_exchange(bl_pf* pf, bl_comm* c);
/* bytes per rank and update: sent into the two all-gathers, received from them, and the rank's own block of records (about what
 * its k_mcl_main reads of source records, from wherever they lie) */
int bl_pf_shard_traffic(bl_pf* pf, int64_t* out3);
/* The same exchange WITHOUT a collective (peer-store form): every rank copies its slice of the tile sums, then its exchange
 * block, straight into every other rank's buffers (mapped like the records: bl_pf_shard_local_ptrs_peer -> bl_ipc_export -> ...
 * -> bl_ipc_open -> bl_pf_shard_set_peer_buffers for every rank, after bl_pf_shard_commit; then bl_pf_shard_peer_commit), raises a
 * per-source counter there, and waits for the other ranks' counters in front of the launches that consume the data: two ~40 us
 * collective latencies per update become two pushes over xGMI.  Layouts and results are the collective form's.  First contact:
 * bl_pf_shard_peer_selftest pushes a pattern to every rank and checks every rank's pattern (device-side spin limit: it cannot
 * hang); the ranks agree on the outcome over their rendezvous and either keep the form (bl_pf_shard_peer_reset(pf, 1)) or all
 * leave it (..., 0) for the collective forms.  Per update: bl_pf_update_begin, bl_pf_shard_exchange_peer, then as above.
 * A rank that waits for another rank's part longer than the cross-rank limit (30 s on the device's real-time clock;
 * BOTLAB_SHARD_WAIT_MS for tests) gives up FOR GOOD: a sticky flag on the device turns the update's groups, finish and map store
 * and every later update of the set into no-ops, and every call that fetches the pose or the particles (bl_pf_update_end,
 * bl_map_update_finishing_pf + bl_pf_pose_estimate, bl_pf_get_particles) and every later bl_pf_update_begin returns
 * BL_ERR_STATE until bl_pf_shard_setup or bl_pf_init_at_pose: nothing is computed from another rank's stale data. */
int bl_pf_shard_local_ptrs_peer(bl_pf* pf, void** sums, void** xchg, void** flags);
int bl_pf_shard_set_peer_buffers(bl_pf* pf, int rank, void* sums, void* xchg, void* flags);
int bl_pf_shard_peer_commit(bl_pf* pf);
int bl_pf_shard_peer_active(const bl_pf* pf);
int bl_pf_shard_peer_selftest(bl_pf* pf, int* ok);
int bl_pf_shard_peer_reset(bl_pf* pf, int keep);
int bl_pf_shard_exchange_peer(bl_pf* pf);
int bl_pf_shard_exchange_peer_phase(bl_pf* pf, int phase);   /* 0 sums + push, 1 wait + groups + push, 2 wait: one process driving several ranks enqueues every rank's phase p before any rank's p + 1 */

/* The NEXT lidar scan handed over early (a SLAM host has it queued, src/slam/slam.cpp:96-104): it is packed into pinned
 * memory now and copied to the device by the next bl_mapping_update* / bl_planner_submit_with_map_update* launch of this
 * ctx, beside that kernel's own work; the bl_pf_update* / bl_mapping_update* call that later brings the same scan then
 * launches no fetch kernel.  Purely an optimisation: a scan that is not the next one used costs only its packing. */
int bl_scan_prefetch(bl_ctx* ctx, const bl_lidar_t* scan);
int bl_mapping_update_finishing_pf(bl_mapping* m, const bl_lidar_t* scan, bl_pf* pf, int64_t pose_utime, bl_grid* map);
/* the same for bl_planner_submit_with_map_update */
int bl_planner_submit_with_map_update_finishing_pf(bl_planner* p, bl_mapping* m, const bl_lidar_t* scan, bl_pf* pf,
                                                   int64_t pose_utime, bl_grid* map, const bl_pose_xyt_t* goal,
                                                   const bl_search_params_t* params);

/* ------------------------------------------------------------------ batched searches, frontiers  
 * n independent search_for_path calls (astar.hpp:58-61) from ONE start on one distance grid, run concurrently (one
 * wavefront each).  Path i is written to out_paths + i*cap_each (at most cap_each poses; out_lens[i] is the true
 * length, 1 = no path); stats, if given, receives {pops, pushes} per search. */
int bl_astar_search_batch(bl_ctx* ctx, const bl_dist* d, const bl_pose_xyt_t* start, const bl_pose_xyt_t* goals, int n,
                          const bl_search_params_t* params, bl_pose_xyt_t* out_paths, int cap_each, int* out_lens,
                          int64_t* stats);
/* distances_(x, y) (obstacle_distance_grid.hpp:63) for n cells given as x0,y0,x1,y1,... in one round trip; a cell
 * outside the grid yields NaN. */
int bl_dist_gather(bl_dist* d, const int32_t* xy_cells, int n, float* out);

/* find_map_frontiers (src/planning/frontiers.hpp:34-36, frontiers.cpp:25-85): the frontiers reachable through free
 * space from the robot cell, in the reference's discovery order, each frontier's cells in its growth order; frontier k
 * = cells offsets[k] .. offsets[k+1] of xy (global x, y per cell). */
typedef struct bl_frontiers bl_frontiers;
int bl_frontiers_find(bl_ctx* ctx, const bl_grid* map, const bl_pose_xyt_t* robot_pose, double min_frontier_length,
                      bl_frontiers** out);
int bl_frontiers_from_host(const int32_t* offsets, int count, const float* xy, bl_frontiers** out);   /* caller-made std::vector<frontier_t> */
int bl_frontiers_count(const bl_frontiers* f);
int bl_frontiers_total_cells(const bl_frontiers* f);
int bl_frontiers_get(const bl_frontiers* f, int32_t* offsets /* count + 1 */, float* xy /* 2 * total_cells */);
int bl_frontiers_stats(const bl_frontiers* f, int* bfs_cells, int* bfs_levels);   /* free-space flood size / depth (diagnostic) */
/* which kernels grew the frontiers of this result (diagnostic, for tests of the fall-backs): 0 the one-workgroup form of grids up to
 * 96 K cells (or a caller-made list), 1 the one-workgroup sweep of larger grids, 2 k_frontier_grow (visited set in LDS, classes from
 * global memory), 3 k_frontier_grow2 (all frontier-class cells of the grid in one LDS set: up to 16 384 of them) */
int bl_frontiers_debug_sweep_kernel(const bl_frontiers* f);
void bl_frontiers_destroy(bl_frontiers* f);

/* ------------------------------------------------------------------ simulator lidar  
 * Lidar._beam_scan (src/sim/lidar.py:106-138) for n beams on a truth world (cells > 0 are occupied, Map.at_xy's index
 * arithmetic without bounds checks included, src/sim/map.py:80-87): beam i starts at (x[i], y[i]) and points along
 * angle[i] (the clamped pose.theta - theta); out_ranges[i] is the marched distance or max_distance.  World origin and
 * resolution are doubles, as the simulator reads them from the .map header. */
int bl_sim_cast_beams(bl_ctx* ctx, const bl_grid* world, double origin_x, double origin_y, double meters_per_cell,
                      const double* x, const double* y, const double* angle, int n, double max_distance, double* out_ranges);

/* ------------------------------------------------------------------ LCM wire codec  
 * The seven message types on the hot path's boundary (the .lcm files under lcmtypes/), LCM 1.4.0 wire format: 8-byte fingerprint, then
 * the members in declaration order, scalars big-endian.  Encoders return the encoded size (buf == NULL: size query) or a
 * negative status; decoders fill caller-owned arrays (capacities in elements) and report the message's counts.  Host
 * code (usable without a GPU) except bl_pf_encode_particles_lcm / bl_grid_encode_lcm, which produce the bytes from
 * device state.  PARITY UNPINNED: no LCM build or LCM-encoded data exists in the reference checkout. */
#define BL_LCM_POSE_XYT 0
#define BL_LCM_ODOMETRY 1
#define BL_LCM_LIDAR 2
#define BL_LCM_PARTICLE 3
#define BL_LCM_PARTICLES 4
#define BL_LCM_OCCUPANCY_GRID 5
#define BL_LCM_ROBOT_PATH 6
#define BL_LCM_TYPE_COUNT 7
uint64_t bl_lcm_fingerprint(int type);
int64_t bl_lcm_encode_pose(int type /* BL_LCM_POSE_XYT or BL_LCM_ODOMETRY */, const bl_pose_xyt_t* pose, uint8_t* buf, int64_t cap);
int64_t bl_lcm_encode_lidar(const bl_lidar_t* scan, const float* intensities /* NULL: zeros */, uint8_t* buf, int64_t cap);
int64_t bl_lcm_encode_particles(int64_t utime, const bl_particle_t* particles, int32_t n, uint8_t* buf, int64_t cap);
int64_t bl_lcm_encode_grid(int64_t utime, float origin_x, float origin_y, float meters_per_cell, int32_t width, int32_t height,
                           const int8_t* cells, uint8_t* buf, int64_t cap);
int64_t bl_lcm_encode_path(int64_t utime, const bl_pose_xyt_t* path, int32_t n, uint8_t* buf, int64_t cap);
int bl_lcm_decode_pose(int type, const uint8_t* buf, int64_t len, bl_pose_xyt_t* out);
int bl_lcm_decode_lidar(const uint8_t* buf, int64_t len, int64_t* utime, int32_t* n, float* ranges, float* thetas, int64_t* times,
                        float* intensities, int32_t cap);
int bl_lcm_decode_particles(const uint8_t* buf, int64_t len, int64_t* utime, int32_t* n, bl_particle_t* out, int32_t cap);
int bl_lcm_decode_grid(const uint8_t* buf, int64_t len, int64_t* utime, float* origin_xy_mpc /* 3 */,
                       int32_t* width_height_ncells /* 3 */, int8_t* cells, int64_t cap);
int bl_lcm_decode_path(const uint8_t* buf, int64_t len, int64_t* utime, int32_t* n, bl_pose_xyt_t* path, int32_t cap);
/* lcm-logger files: one event = sync 0xEDA1DA01, event number, timestamp (us), channel length, data length, channel, data */
int64_t bl_lcm_log_event_size(int32_t channel_len, int32_t data_len);
int64_t bl_lcm_log_write_event(int64_t event_number, int64_t timestamp_us, const char* channel, const uint8_t* data, int32_t data_len,
                               uint8_t* buf, int64_t cap);
/* returns the event's total size, 0 if buf[0..len) does not hold a whole event yet, < 0 if there is no event at buf */
int64_t bl_lcm_log_read_event(const uint8_t* buf, int64_t len, int64_t* event_number, int64_t* timestamp_us, int64_t* channel_off,
                              int32_t* channel_len, int64_t* data_off, int32_t* data_len);
/* particles() + encode (slam.cpp:265-268) and toLCM() + encode (slam.cpp:285-289) from device state, one D2H into buf */
int64_t bl_pf_encode_particles_lcm(bl_pf* pf, int64_t utime, uint8_t* buf, int64_t cap);
int64_t bl_grid_encode_lcm(bl_grid* grid, int64_t utime, uint8_t* buf, int64_t cap);

/* The MotionPlanner members plan_path_to_frontier reads (motion_planner.hpp:153-165). */
typedef struct {
    double robot_radius;               /* params_.robotRadius */
    bl_search_params_t search;         /* searchParams_ */
    int32_t num_frontiers;             /* setNumFrontiers() */
    bl_pose_xyt_t prev_goal;           /* setPrevGoal() */
} bl_motion_planner_t;
/* plan_path_to_frontier (frontiers.hpp:50-53, frontiers.cpp:104-214): closest frontier, its middle cell, then the
 * expanding-square sweep of candidate goals -- every ring's planPath calls run as one batch of searches.  An empty
 * frontier list gives *out_len = 0 (the reference's empty path); a sweep that never finds a goal gives the 1-pose path
 * (DESIGN.md D8).  stats, if given: {pops, pushes, searches run}. */
int bl_plan_path_to_frontier(bl_ctx* ctx, const bl_frontiers* frontiers, const bl_pose_xyt_t* robot_pose, bl_dist* dist,
                             const bl_motion_planner_t* planner, bl_pose_xyt_t* out_path, int cap, int* out_len,
                             bl_pose_xyt_t* chosen_goal, int64_t* stats);

/* ------------------------------------------------------------------ navigation field (no reference counterpart)
 * The exact cost-to-go of every cell to a set of goal cells, and cheapest paths read off it: one field answers every query against
 * its goals -- the path from any start, the cost at any cell, the nearest of many goals.  (bl_astar_search stays the reference's
 * search, bit for bit; that search is not a shortest-path search and its paths are 4-connected.)
 *   Inputs: a transformed bl_dist -- n(c), the integer L1 distance of cell c to the nearest non-free cell (0xFFFF: none), and the
 *     float table f[n] the distance grid maps it through --, the parameters below, and a list of goal cells.
 *   Per-distance tables, built once per compute on the host in double, d = (double)f[n], n = 0 .. width + height:
 *     traversable(n): n != 0xFFFF and d > minDistanceToObstacle * 1.000001 -- isValid of bl_astar_search, formed by
 *       the host code that fills the search's cost table: a cell the search calls invalid is not traversable here, every cell of a
 *       map without any non-free cell included.
 *     penalty(n): 0 when n is not traversable, d >= maxDistanceWithCost or maxDistanceWithCost <= minDistanceToObstacle; otherwise
 *       (int32)floor(obstacle_gain * pow((maxD - d) / (maxD - minD), distanceCostExponent)), the host's pow.  With
 *       distanceCostExponent >= 0 (required) it lies in [0, obstacle_gain].
 *   Moves: 8-connected, inside the grid, between traversable cells; a straight move costs 10, a diagonal one 14.  The diagonal
 *     (dx, dy) from c is allowed only if c + (dx, 0) and c + (0, dy) are traversable as well: no corner is cut.
 *   Goal set: every traversable cell within Chebyshev distance reach_cells of a listed cell that lies inside the grid; its label is
 *     the lowest index of such a listed cell.  Listed cells outside the grid contribute nothing.
 *   Field (uint32 per cell, row-major): 0 on the goal set; elsewhere penalty(n(c)) + min over the allowed moves c -> c' of
 *     (step + field(c')); 0xFFFFFFFF (UNREACHED) where c is not traversable or not connected to the goal set.  This is the minimum
 *     over paths of the step costs plus the penalties of the path's cells outside the goal set; steps cost at least 10, so the
 *     solution is unique and does not depend on the order it is computed in.  width * height * (14 + obstacle_gain) > 2^32 - 2 is
 *     refused (BL_ERR_ARG): no cost can wrap.  A compute that returns an error leaves the handle without a field (the readers
 *     return BL_ERR_STATE), whatever it held before.
 *   Path from a start pose: the start cell is global_position_to_grid_cell of the pose, as the search finds it.  out[0] is the start
 *     pose as given.  From cell c the path takes the allowed move minimising step + field(c'), ties by the order (+x), (-x), (+y),
 *     (-y), (+x+y), (-x+y), (+x-y), (-x-y), until it stands on the goal set.  Pose k >= 1: x, y as bl_astar_search writes a path cell
 *     ((float)((double)origin + (double)cell * (double)meters_per_cell)), theta = atan2f(dy, dx) of the move into it, utime the
 *     start's.  Length 1 is "no path": the start is off the grid, not traversable, UNREACHED, or on the goal set already.  Per path
 *     also: the label of the goal-set cell it ends on (-1 if it ends on none) and field(start) (UNREACHED off the grid or on a cell
 *     that is not traversable).
 * How it is computed (bl_navfield.hip): tiles of 32 x 32 cells relaxed to their fixed point in LDS, round after round of the tiles
 * whose halo got lower; no workgroup waits for another, and the host ends the rounds when a round leaves no tile listed.  At most
 * (traversable cells) + 1 rounds can list a tile; beyond that: BL_ERR_STATE.
 * Calls are stream-ordered on the ctx stream and synchronous on return.  The bl_dist must belong to the same ctx and outlive the
 * field; bl_navfield_paths reads its distances again, so it answers for the field only until that grid is transformed again. */
typedef struct bl_navfield_params_t {
    double minDistanceToObstacle;      /* bl_search_params_t's three, the same meaning of distance */
    double maxDistanceWithCost;
    double distanceCostExponent;       /* >= 0, finite */
    int32_t obstacle_gain;             /* 0 .. 4095 (default 50): the penalty of a cell right at minDistanceToObstacle */
    int32_t reach_cells;               /* 0 .. 1024; 0: a goal is exactly the listed cell */
} bl_navfield_params_t;                /* 32 bytes */
typedef struct bl_navfield bl_navfield;
int bl_navfield_create(bl_ctx* ctx, bl_navfield** out);               /* buffers grow on demand */
void bl_navfield_destroy(bl_navfield* nf);
int bl_navfield_compute(bl_navfield* nf, const bl_dist* dist, const bl_navfield_params_t* params, const int32_t* goal_xy_cells /* x0,y0,x1,y1,... */,
                        int n_goals);
/* one goal: the cell of a pose (off the grid: nothing is reached) */
int bl_navfield_compute_to_pose(bl_navfield* nf, const bl_dist* dist, const bl_navfield_params_t* params, const bl_pose_xyt_t* goal);
/* n independent descents in one launch.  Path i goes to out_paths + i * cap_each (at most cap_each poses; out_lens[i] is the true
 * length); out_goal / out_cost (optional): the label reached and field(start) per path. */
int bl_navfield_paths(bl_navfield* nf, const bl_pose_xyt_t* starts, int n, bl_pose_xyt_t* out_paths, int cap_each, int* out_lens,
                      int32_t* out_goal, uint32_t* out_cost);
int bl_navfield_gather(bl_navfield* nf, const int32_t* xy_cells, int n, uint32_t* out);   /* field at n cells; off the grid: UNREACHED */
int bl_navfield_download(bl_navfield* nf, uint32_t* cells);           /* width * height words */
int bl_navfield_shape(const bl_navfield* nf, int* width, int* height);
void* bl_navfield_device_ptr(bl_navfield* nf);                        /* uint32_t* in HBM (NULL before the first compute) */
/* the tables of the last compute, *n = width + height + 1 entries each (either array may be NULL) */
int bl_navfield_tables(bl_navfield* nf, uint8_t* traversable, int32_t* penalty, int* n);
/* of the last compute, five counts: rounds that relaxed a tile, sweeps over a tile in LDS, traversable cells, reached cells,
 * goal-set cells */
int bl_navfield_stats(bl_navfield* nf, int64_t* out);

/* ------------------------------------------------------------------ view gain (no reference counterpart)
 * How much unknown map a sensor standing on a candidate cell could see: the number of distinct unknown cells that a fan of rays
 * cast from the cell reaches.  All of it is integer arithmetic on the int8 log-odds cells of a bl_grid.
 *   Cell classes of a log-odds value v: blocking when v > occupied_above (default 0); unknown when unknown_lo <= v <= unknown_hi
 *     (defaults 0 and 0); anything else is seen through.  Blocking is tested first.
 *   Ray table, built once per parameter set on the host in double: ray k of K = n_rays ends at the offset
 *     (lround(R * cos(t)), lround(R * sin(t))), t = 2.0 * M_PI * k / K evaluated left to right, R = radius_cells; the host's cos, sin
 *     and lround.  1 <= R <= 255, 1 <= K <= 4096.  A ray whose end is (0, 0) visits nothing.
 *   Line: the all-integer Bresenham walk from (0, 0) to the end offset (ex, ey), start cell excluded, end cell included:
 *     dx = |ex|, dy = |ey|, sx = sign(ex), sy = sign(ey), err = dx - dy, (x, y) = (0, 0); until (x, y) = (ex, ey):
 *     e2 = 2 * err; if e2 >= -dy { err -= dy; x += sx; }  if e2 <= dx { err += dx; y += sy; }  then visit (x, y).
 *     The walk is relative to the candidate: the same for every candidate.
 *   Seen set of a candidate cell c, taking the cells c + (x, y) of each ray in order: the ray ends at the first cell outside the
 *     grid, and at the first blocking cell, which is not seen; every unknown cell before that point is seen.  Unknown cells do not
 *     stop a ray (the optimistic rule).  The candidate's own cell is never examined, whatever it holds.
 *   Gain: gain(c) = the number of distinct cells in the seen set, uint32.  Rays overlap near the candidate, so this is not a sum
 *     over rays; it does not depend on the order the rays are taken in.  A candidate outside the grid has gain 0.
 * How it is computed (bl_viewgain.hip): one workgroup per candidate, a bitmap of the (2R + 1)^2 window in LDS, the rays dealt over
 * the threads.  Calls are stream-ordered on the ctx stream and synchronous on return; the bl_grid must belong to the same ctx. */
typedef struct bl_viewgain_params_t {
    int32_t radius_cells;              /* R, 1 .. 255 */
    int32_t n_rays;                    /* K, 1 .. 4096 */
    int32_t occupied_above;            /* -128 .. 127 (default 0) */
    int32_t unknown_lo;                /* -128 <= unknown_lo <= unknown_hi <= 127 (defaults 0, 0) */
    int32_t unknown_hi;
} bl_viewgain_params_t;                /* 20 bytes */
typedef struct bl_viewgain bl_viewgain;
int bl_viewgain_create(bl_ctx* ctx, bl_viewgain** out);               /* buffers grow on demand */
void bl_viewgain_destroy(bl_viewgain* vg);
/* builds and uploads the ray table; BL_ERR_ARG for parameters out of range (the handle then has none) */
int bl_viewgain_set_params(bl_viewgain* vg, const bl_viewgain_params_t* params);
/* the table the kernels use: *n = n_rays, xy (optional) = x0, y0, x1, y1, ...; BL_ERR_STATE before set_params */
int bl_viewgain_ray_ends(bl_viewgain* vg, int32_t* xy, int* n);
/* gain of n candidate cells (x0, y0, x1, y1, ...) in one launch; n == 0 is fine; BL_ERR_STATE before set_params */
int bl_viewgain_compute(bl_viewgain* vg, const bl_grid* map, const int32_t* xy_cells, int n, uint32_t* out_gain);
/* the seen set of one candidate: (2R + 1)^2 bytes, 0 / 1, row-major, the window around the cell (byte (dy + R) * (2R + 1) + dx + R) */
int bl_viewgain_debug_seen(bl_viewgain* vg, const bl_grid* map, int x, int y, uint8_t* out);

/* ------------------------------------------------------------------ Rao-Blackwellized grid SLAM (FastSLAM on grids; no reference counterpart)
 * P particles (1 .. BL_RBSLAM_MAX_PARTICLES), each with a pose, a parent pose, a cumulative score c_p (int64, half-units of the
 * sensor model's log-odds score) and its OWN width x height int8 map; all maps share one frame.  Every piece below is one the
 * library already defines for one map and one filter, so that tests/rb_slam_model.py -- the same definition over the reference's
 * per-particle entry points -- agrees with the device bit for bit.
 *
 * One bl_rbslam_update(odometry, scan, rand_value, noise):
 *   1. Moved?  ActionModel::updateAction's rule on the odometry (action_model.cpp:22-75), host scalars, as bl_pf_update.
 *   2. If moved and a resampling is DUE (rule below): low-variance resampling of the P particles by the integer-prefix rule with
 *      M = P on the weight units u_p: T_m = (r + m / P) * S in double, r = (rand_value / RAND_MAX) / P, S = sum u; the source of
 *      child m is the first i with T_m <= (double)prefix_i (prefix = the running uint64 sum of u), clamped to P - 1.  A child takes
 *      its source's pose, parent pose AND map.  All cumulative scores are reset to 0.
 *   3. If moved, action: ActionModel::applyAction per particle (action_model.cpp:78-103).  noise: a HOST array of 3 P floats
 *      (sampled rot1, trans, rot2 per particle; the parity mode), or NULL: Philox from bl_rbslam_set_noise_seed's seed, the
 *      counters and arithmetic of bl_pf_update.  The parent pose becomes the old pose (with its utime); the pose's utime becomes the
 *      odometry's.
 *   4. If moved, weigh: h_p = SensorModel::likelihood (sensor_model.cpp:14-59) of the scan for particle p against ITS OWN map,
 *      in half-units (an exact integer: a ray scores 2 * odds, o1 or o2), the moving scan interpolated between parent pose and pose
 *      by the rays' time stamps (interpolate_pose_by_time; equal utimes: the pose itself).  c_p = min(c_p + h_p, BL_RBSLAM_SCORE_MAX).
 *      Weight units: u_p = max(1000 * c_p, 2) -- the filter's unit of 0.0005 with its floor of 0.001.  Adding log-odds scores over the
 *      updates since the last resampling is the log-domain product of the weights; with a resampling on every update u_p is exactly
 *      the reference filter's weight.
 *      Saturation: c_p <= 2^33, so u_p < 2^43, S <= 4096 u < 2^55 and Q = sum u^2 < 2^98; with num, den < 2^16 both sides of the test
 *      below stay under 2^126: 128-bit integers cannot overflow.  (A scan of 8192 rays scores at most 2^21 half-units.)
 *   5. Best particle: the largest u_p, ties to the lowest index.  The SLAM pose of the update is its pose; best_map is its map.
 *   6. Map: every particle's map receives Mapping::updateMap(scan, pose_p, map_p) (mapping.cpp:17-127) with
 *      previousPose_ = parent_pose_p: v' = max(-128, min(127, v + hit * H) - miss * M) for a cell that ends H rays and is crossed by M,
 *      over the rays with range <= max_laser_distance; rays that leave the grid update the cells inside it.  The very FIRST update
 *      after bl_rbslam_init_at_pose latches and changes no cell (the reference's initialized_).  Not moved: steps 2-5 are skipped and
 *      the scan is integrated with previousPose_ = pose_p, i.e. Mapping::updateMap(scan, pose_p, map_p) on a mapper whose previous
 *      update was at pose_p.
 * Resampling is DUE before the action of a moved update iff den * S^2 <= num * P * Q, in exact integers, S and Q over the units the
 * last weighing left.  num / den = 1 / 1 resamples on every moved update (Cauchy-Schwarz); the default 1 / 2 is N_eff <= P / 2.
 * Nothing is due before the first weighing (bl_rbslam_set_particles with scores counts as one).
 * Map copies of a resampling: a particle -> slot table; the first child of a source keeps its slot, the k-th other child (in order
 * of index) is copied into the slot of the k-th particle that died, all copies in one launch.  Only the order of results is the
 * contract.  Everything is stream-ordered on the ctx stream; bl_rbslam_update synchronises once, to hand `result` back.
 * Limits: the maps take P * ((width * height + 15) & ~15) bytes; more than BL_RBSLAM_MAX_MAP_BYTES: BL_ERR_ARG.  4 GiB holds 4096
 * maps of 1000 x 1000 cells, a small part of the device's memory, which other objects of the process share.  width, height <= 65535;
 * at most 8192 rays per scan. */
#define BL_RBSLAM_MAX_PARTICLES 4096
#define BL_RBSLAM_MAX_MAP_BYTES (4ull << 30)
#define BL_RBSLAM_SCORE_MAX (1ll << 33)
typedef struct bl_rbslam_result_t {
    int32_t moved, resampled;          /* of this update */
    int32_t best, pad;                 /* the best particle as of the last weighing (0 before the first) */
    bl_pose_xyt_t best_pose;           /* its pose, utime = the particles' pose utime */
    uint64_t S, Q_lo, Q_hi;            /* sum u and sum u^2 (two words) as of the last weighing */
} bl_rbslam_result_t;                  /* 64 bytes */
typedef struct bl_rbslam bl_rbslam;
int bl_rbslam_create(bl_ctx* ctx, int num_particles, int width, int height, float meters_per_cell, float cells_per_meter,
                     float origin_x, float origin_y, float max_laser_distance, int8_t hit_odds, int8_t miss_odds, bl_rbslam** out);
void bl_rbslam_destroy(bl_rbslam* rb);
int bl_rbslam_set_resampling(bl_rbslam* rb, uint32_t num, uint32_t den);      /* 1 .. 65535 each; default 1 / 2 */
int bl_rbslam_set_noise_seed(bl_rbslam* rb, uint64_t seed);
/* poses drawn as bl_pf_init_at_pose draws them (the last particle is the pose itself), maps zero, scores zero, the ActionModel and the
 * map latch reset */
int bl_rbslam_init_at_pose(bl_rbslam* rb, const bl_pose_xyt_t* pose, uint64_t seed);
/* poses and parent poses of all P particles (utimes: particle 0's); cum_scores (P values in 0 .. BL_RBSLAM_SCORE_MAX) or NULL: zeros,
 * and then nothing is due until the next weighing.  Maps, ActionModel and latch are left as they are.  BL_ERR_STATE before init. */
int bl_rbslam_set_particles(bl_rbslam* rb, const bl_particle_t* particles, const int64_t* cum_scores);
/* any of the three may be NULL; weight = u_p / S */
int bl_rbslam_get_particles(bl_rbslam* rb, bl_particle_t* out, int64_t* cum_scores, uint64_t* units);
/* BL_ERR_STATE before bl_rbslam_init_at_pose; result may be NULL */
int bl_rbslam_update(bl_rbslam* rb, const bl_pose_xyt_t* odometry, const bl_lidar_t* scan, int rand_value, const float* noise,
                     bl_rbslam_result_t* result);
int bl_rbslam_map_download(bl_rbslam* rb, int p, int8_t* cells);              /* particle p's map, width * height bytes */
int bl_rbslam_map_upload(bl_rbslam* rb, int p, const int8_t* cells);
/* the best particle's map, device to device, into an ordinary grid of the same shape and ctx (it takes the frame): BL_ERR_ARG otherwise */
int bl_rbslam_best_map(bl_rbslam* rb, bl_grid* dst);
/* of the last moved update: the source of every particle (m itself when it did not resample) and h_p; either may be NULL */
int bl_rbslam_debug_last(bl_rbslam* rb, int32_t* resample_idx, int32_t* likelihood_half_units);

/* ---- scan-matched proposals (GMapping's structure; off by default).  With matching on, a MOVED update gains a step between the
 * action and the weighing:
 *   3b. For every particle p, "correlative scan matching" above, word for word, with map = p's OWN map and centre c = p's pose as
 *       step 3 left it: valid rays 0.15f < range < max_range (at most BL_RBSLAM_MATCH_MAX_RAYS of them: more is BL_ERR_ARG, refused
 *       before the ActionModel latches the odometry, so the object is as before the call), theta_k = c.theta + (float)dk * dtheta,
 *       scoreRay's endpoint cells, score(di, dj, dk) = sum of max(0, L_p[ey + dj][ex + di]) with 0 outside the grid, the best
 *       candidate by the 64-bit key (score, then smallest di*di + dj*dj, |dk|, dk, dj, di).  The scan is taken as rigid at the pose:
 *       the rays' time stamps play no part in the match.
 *       If score >= min_score and (di, dj, dk) != (0, 0, 0), p's pose becomes x = (float)((double)c.x + di * (double)meters_per_cell),
 *       y likewise with dj, theta = wrap_to_pi(theta_dk); otherwise it stays bit for bit as it was.  The centre wins every tie it is
 *       part of, so an empty or all-free map moves nobody.  The utime and the parent pose are untouched.
 *   Steps 4-6 run on the new pose: the weighing and the map update interpolate from the parent pose to the matched pose.
 * A not-moved update matches nothing; a window of 0, 0, 0 leaves every output of the update equal to matching off.
 * One launch for all particles, a workgroup each, stream-ordered like the rest.  The map cells a particle's candidates can reach lie in
 * the window  centre cell +- (reach + n + 1)  per axis (n = nx or ny; centre cell = the truncated grid position of c), clipped to the
 * grid, reach = ceilf(longest valid range * cells_per_meter) in float.  Path 0: the positive part of that window is staged in LDS;
 * path 1: the map is read directly.  The path is one for the whole launch and decided on the host from the bound of the window:
 *   bw = min(2 * (reach + nx + 1) + 1 + 3, width), bh = min(2 * (reach + ny + 1) + 1, height);
 *   path 0 iff ((bw + 3) & ~3) * bh <= BL_RBSLAM_MATCH_WINDOW_BYTES.
 * (+ 3: with width % 4 == 0 the window's first column steps down to a multiple of four.  8 m at 5 cm with n = 8: 344 * 339 bytes.) */
#define BL_RBSLAM_MATCH_MAX_N 8
#define BL_RBSLAM_MATCH_MAX_NTHETA 16
#define BL_RBSLAM_MATCH_MAX_RAYS 4096
#define BL_RBSLAM_MATCH_WINDOW_BYTES (120 * 1024)
typedef struct bl_rbslam_match_params_t {
    int32_t nx, ny;          /* half window in cells, 0 .. BL_RBSLAM_MATCH_MAX_N                                      */
    int32_t ntheta;          /* half window in heading steps, 0 .. BL_RBSLAM_MATCH_MAX_NTHETA                         */
    float   dtheta;          /* heading step in radians, > 0                                                          */
    float   max_range;       /* rays with range >= max_range are skipped                                              */
    int32_t min_score;       /* a best score below this leaves the pose where the action put it: accepted = 0         */
} bl_rbslam_match_params_t;  /* 24 bytes */
/* NULL: off (the default).  BL_ERR_ARG: a limit exceeded, dtheta <= 0 or NaN; the previous setting then stays in force. */
int bl_rbslam_set_scan_matching(bl_rbslam* rb, const bl_rbslam_match_params_t* params);
/* of the last moved update with matching on since bl_rbslam_init_at_pose, P entries each, any may be NULL: the best candidate, its
 * score, the score of (0, 0, 0), the candidates sharing the best score, score >= min_score.  BL_ERR_STATE if there was none. */
int bl_rbslam_debug_match(bl_rbslam* rb, int32_t* di, int32_t* dj, int32_t* dk, int32_t* score, int32_t* score_centre,
                          int32_t* ties, int32_t* accepted);
/* which path the last matched update took: 0 the map window staged in LDS, 1 the map read directly; -1 before the first */
int bl_rbslam_debug_match_path(const bl_rbslam* rb);

/* ------------------------------------------------------------------ the exploration step, asynchronously  (src/planning/exploration.cpp:277-369)
 * Exploration::executeExploringMap on every published map: planner_.setMap, find_map_frontiers, and -- when the robot is within
 * 0.5 m of currentTarget_ or has none -- plan_path_to_frontier; then the status / next-state rule (:332-368; D10).  A submission
 * snapshots the map and the device-resident pose on ctx's stream; one of `lanes` side streams runs the distance transform and the
 * frontier search against the snapshot; bl_explorer_fetch hands back the steps in submission order and applies the rule with the
 * state consecutive steps share (currentTarget_, currentPath_), running plan_path_to_frontier on that lane when it is due.  At
 * most `lanes` submissions may be pending.  bl_explorer_submit / bl_explorer_pending on one thread and bl_explorer_fetch on
 * another (the reference's exploration PROCESS beside its SLAM process) may run concurrently; bl_explorer_pending counts the
 * submission a fetch is still working on. */
typedef struct bl_explorer bl_explorer;
typedef struct {
    int32_t next_state;      /* exploration_status_t: 1 EXPLORING_MAP, 2 RETURNING_HOME, 4 FAILED_EXPLORATION */
    int32_t status;          /* 0 IN_PROGRESS, 1 COMPLETE, 2 FAILED */
    int32_t num_frontiers;   /* frontiers_.size() */
    int32_t frontier_cells;
    int32_t planned;         /* 1: plan_path_to_frontier ran in this step */
    int32_t path_length;     /* currentPath_.path_length after the step */
    int64_t pops, pushes, searches;   /* of this step's plan_path_to_frontier */
    int32_t bfs_cells, bfs_levels;    /* free cells the frontier search flooded, and its depth */
    bl_pose_xyt_t pose;      /* currentPose_ of the step (the snapshot's) */
    bl_pose_xyt_t target;    /* currentTarget_ after the step */
    float frontiers_ms;      /* device time of find_map_frontiers' kernels */
    float plan_ms;           /* host wall time of plan_path_to_frontier (0 when it did not run) */
} bl_explore_result_t;
int bl_explorer_create(bl_ctx* ctx, int lanes, double robot_radius, bl_explorer** out);  /* lanes 1..16; MotionPlannerParams::robotRadius (a double: motion_planner.hpp:27-35) */
void bl_explorer_destroy(bl_explorer* e);
int bl_explorer_set_state(bl_explorer* e, const bl_pose_xyt_t* target, const bl_pose_xyt_t* prev_goal);   /* currentTarget_ / setPrevGoal; null: unchanged */
int bl_explorer_submit(bl_explorer* e, const bl_grid* map, const void* d_pose);          /* d_pose: bl_pose_xyt_t in HBM (e.g. bl_pf_pose_device_ptr) */
int bl_explorer_pending(const bl_explorer* e);
int bl_explorer_fetch(bl_explorer* e, bl_explore_result_t* out, bl_pose_xyt_t* out_path, int cap);   /* out_path: currentPath_, up to cap poses */
int bl_explorer_frontiers(const bl_explorer* e, bl_frontiers** out);                     /* frontiers_ of the last fetched step (caller destroys) */

/* ------------------------------------------------------------------ local planner (no reference counterpart for the algorithm)
 * The velocity command of the next control period, by rollout over a navigation field: of the (v, w) pairs a robot can reach within
 * dt_control, the one whose simulated arc ends lowest on the field without touching a cell that is not traversable.  The reference
 * ends in src/mbot/motion_controller.cpp, a rotate-translate-rotate waypoint follower that never looks at the map; the command has
 * the shape of its lcmtypes/mbot_motor_command_t.lcm {utime, trans_v, angular_v}.
 *   Inputs: a computed bl_navfield -- its uint32 field, traversable(n) and penalty(n) of its last compute, n(c) and the frame of its
 *     bl_dist --, n states {pose, v, w} (the velocities the robot has now) and the parameters below.
 *   Candidate tables, per state, on the host in double, narrowed to float once:
 *     v_lo = max(v_min, v - acc_v * dt_control), v_hi = min(v_max, v + acc_v * dt_control); if v_lo > v_hi both become v clamped to
 *     [v_min, v_max].  v_i = v_lo + (v_hi - v_lo) * i / (n_v - 1), evaluated left to right; n_v == 1: v_0 = v_hi.  The same for w_j
 *     with the limits -w_max and w_max, acc_w and n_w.  Candidate c = j * n_v + i.
 *   Rollout of candidate (i, j), float arithmetic, one rounding per operation: (x, y) of the pose, theta = wrap_to_pi(pose.theta),
 *     s = v_i * dt_sim, dth = w_j * dt_sim.  For k = 1 .. n_steps: (cs, sn) = cosf, sinf of theta (glibc's, bit for bit: bl_math.h);
 *     x = x + s * cs; y = y + s * sn; theta = wrap_to_pi(theta + dth); the visited cell is global_position_to_grid_cell of (x, y),
 *     inside the grid by the test bl_navfield_paths applies to a start pose.
 *   Admissible: every visited cell is inside the grid and traversable, and the last one, e, has field(e) != UNREACHED.  Then, in int64,
 *     cost = w_field * field(e) + w_heading * h + w_clear * (sum over k of penalty(n(cell_k))) + w_speed * (n_v - 1 - i)
 *     h = 0 when field(e) == 0; otherwise with d the move bl_navfield_paths would take from e (same allowed moves, same tie order) and
 *     a_d its angle as a float constant ((float) of 0, pi, pi/2, -pi/2, pi/4, 3 pi/4, -pi/4, -3 pi/4 in double),
 *     h = (int32)floorf(fabsf((float)angle_diff((double)theta_end, (double)a_d)) * (float)(1024 / pi)); 1024 when e has no allowed move
 *     to a reached cell.
 *   Result per state: the admissible candidate with the least key (cost, c) -- ties to the lowest c --: trans_v = v_i, angular_v = w_j,
 *     index = c, cost, n_admissible.  Flags, each with the command (0, 0) and index -1:
 *       REACHED    the pose's own cell has field 0; nothing is rolled out; cost 0, n_admissible 0
 *       OFF_FIELD  the pose is off the grid, on a cell that is not traversable, or on an UNREACHED cell; cost INT64_MAX, n_admissible 0
 *       BLOCKED    no candidate is admissible; cost INT64_MAX
 *     The minimum is over exact integer keys: the result does not depend on the launch shape.
 *   Refused with BL_ERR_ARG: by bl_localplan_set_params a non-finite value, v_min > v_max, w_max < 0, dt_control <= 0, dt_sim <= 0, a
 *     count or a weight outside its range; by the calls that see the field (double)max(|v_min|, |v_max|) * (double)dt_sim >
 *     (double)meters_per_cell -- a step may never skip a cell --, a state with a non-finite member and a state whose
 *     fabsf(pose.theta) > BL_LOCALPLAN_MAX_THETA: 65536 rad is 10 432 steps of wrap_to_pi (each rounded to float), below the 2^16 steps after which bl_math.h
 *     cuts that loop, so every accepted heading wraps exactly as the reference's loop would.
 * How it is computed (bl_localplan.hip): a workgroup takes one state and a run of consecutive j.  The headings theta_k of a (state, j)
 * do not depend on i: they are formed once, their (cos, sin) once per (j, k) into LDS, and the n_v speeds of that j read them back as
 * broadcasts.  A rollout moves at most ceil(max|v| * dt_sim * n_steps * cells_per_meter) cells from the pose per axis; the costs
 * (-1, or the penalty) of the window of that reach around the pose's cell are staged in LDS when it is small enough:
 *   R = (int)ceil((double)max(|v_min|, |v_max|) * (double)dt_sim * n_steps * (double)cells_per_meter) + 2;
 *   path 0 (staged) iff (2 R + 1) * (2 R + 1) * 2 <= BL_LOCALPLAN_WINDOW_BYTES, path 1 (the grids read through L2) otherwise.
 * A cell outside the window is read from the grids on either path, so the rule decides speed only.  Per workgroup the least key,
 * a second kernel takes the least of those per state.  bl_localplan_commands is one launch sequence for all states, stream-ordered
 * on the ctx stream, with one synchronisation, at the return. */
#define BL_LOCALPLAN_WINDOW_BYTES (48 * 1024)
#define BL_LOCALPLAN_MAX_NV 64
#define BL_LOCALPLAN_MAX_NW 1025
#define BL_LOCALPLAN_MAX_STEPS 255
#define BL_LOCALPLAN_MAX_WEIGHT 65535
#define BL_LOCALPLAN_MAX_THETA 65536.0f
#define BL_LOCALPLAN_REACHED 1
#define BL_LOCALPLAN_OFF_FIELD 2
#define BL_LOCALPLAN_BLOCKED 4
typedef struct bl_localplan_state_t {
    bl_pose_xyt_t pose;
    float v, w;                        /* the velocities the robot has now */
} bl_localplan_state_t;                /* 32 bytes */
typedef struct bl_localplan_params_t {
    float v_min, v_max;                /* m/s; v_min < 0 allows reversing */
    float w_max;                       /* rad/s, >= 0 */
    float acc_v, acc_w;                /* m/s^2, rad/s^2 */
    float dt_control, dt_sim;          /* s, > 0: the control period and the integration step */
    int32_t n_v, n_w, n_steps;         /* 1 .. 64, 1 .. 1025, 1 .. 255 */
    int32_t w_field, w_heading, w_clear, w_speed;   /* 0 .. 65535 each */
} bl_localplan_params_t;               /* 56 bytes */
typedef struct bl_localplan_result_t {
    float trans_v, angular_v;          /* mbot_motor_command_t's two */
    int32_t index;                     /* c of the winner, -1 with any flag */
    int32_t n_admissible;
    int64_t cost;
    int32_t flags, pad;
} bl_localplan_result_t;               /* 32 bytes */
typedef struct bl_localplan bl_localplan;
int bl_localplan_create(bl_ctx* ctx, bl_localplan** out);             /* buffers grow on demand */
void bl_localplan_destroy(bl_localplan* lp);
int bl_localplan_set_params(bl_localplan* lp, const bl_localplan_params_t* params);   /* refused: the handle keeps what it had */
/* BL_ERR_STATE before set_params and for a field handle without a field; n == 0 is fine */
int bl_localplan_commands(bl_localplan* lp, bl_navfield* nf, const bl_localplan_state_t* states, int n, bl_localplan_result_t* results);
/* the n_v * n_w costs of one state's candidates, INT64_MAX for an inadmissible one, rolled out whatever the state's flags would be */
int bl_localplan_debug_costs(bl_localplan* lp, bl_navfield* nf, const bl_localplan_state_t* state, int64_t* out);
/* the n_steps poses (x, y, theta after step k; utime the state's) of candidate c, visited cells admissible or not */
int bl_localplan_debug_rollout(bl_localplan* lp, bl_navfield* nf, const bl_localplan_state_t* state, int c, bl_pose_xyt_t* out);
/* the candidate tables of one state: n_v and n_w floats (either may be NULL); host arithmetic only */
int bl_localplan_tables(bl_localplan* lp, const bl_localplan_state_t* state, float* v, float* w);
/* which path the last launch took: 0 the window staged in LDS, 1 the grids read directly; -1 before the first */
int bl_localplan_debug_path(const bl_localplan* lp);
/* device time of the last bl_localplan_commands' kernels (HIP events around the launches); BL_ERR_STATE before the first */
int bl_localplan_last_device_ms(const bl_localplan* lp, float* ms);

/* ------------------------------------------------------------------ path shortcutting (no reference counterpart)
 * Any-angle waypoints from a grid path: the cheapest chain of straight segments between cells of the path, each segment running
 * over cells with enough clearance only.  bl_astar_search, bl_navfield_paths and bl_plan_path_to_frontier emit a pose per grid
 * cell, as the reference's makePath does (src/planning/astar.cpp:235-274), and src/mbot/motion_controller.cpp turns, drives and
 * stops once per pose.  Done exactly this is all-pairs line of sight over the path plus a shortest path over the visibility graph,
 * not greedy string pulling.  Everything that is compared is an integer.
 *   Inputs: a transformed bl_dist -- n(c) and the float table f[n], as the navigation field reads them --, the parameters below and
 *     P paths of cells; path p has m_p cells (x_k, y_k), all inside the grid (a cell off the grid: BL_ERR_ARG).
 *   ok(c): n(c) != 0xFFFF and (double)f[n(c)] > clearance * 1.000001 -- the field's traversable(n) with clearance in place of
 *     minDistanceToObstacle, formed as a per-n table on the host by the same code.
 *   Cover of a pair (a, b), DX = x_b - x_a, DY = y_b - y_a: every cell (x_a + u, y_a + v) of the bounding box of the two cells with
 *     2 * |u * DY - v * DX| <= |DX| + |DY|.  This is exactly the set of cells whose closed square meets the segment between the two
 *     cell centres (the supercover: both cells at a corner crossing); tests/test_path_shortcut_model_cpu.py checks it against
 *     rational segment / square clipping.  It is the same set from either end.
 *   Edges: (i, j) is an edge iff 0 < j - i <= max_span and either j == i + 1 or every cell of cover(i, j) is ok.  The input path's
 *     own steps are always edges, whatever clearance is.
 *   Length: L(i, j) = floor(sqrt(2^20 * (DX^2 + DY^2))), the exact integer square root (width + height < 65535, so the argument
 *     is below 2^52).  A straight cell step is 1024, (3, 4) is exactly 5120.
 *   Cost: cost[0] = 0; cost[j] = min over edges (i, j) of cost[i] + L(i, j) + waypoint_cost, in int64; pred[j] the minimising i, ties
 *     to the SMALLEST i.
 *   Result per path: the kept indices 0 = k_0 < ... < k_r = m - 1 read back from pred, their count, cost[m - 1], and the input
 *     path's own cost: the sum over (i, i + 1) of L(i, i + 1) + waypoint_cost.  m == 0: count 0, both costs 0; m == 1: count 1, both
 *     costs 0.  The minimum is over exact integers: the result does not depend on the launch shape.  max_span == 1 returns every path
 *     unchanged, and so does a clearance that no cell satisfies.
 *   Refused with BL_ERR_ARG: by bl_shortcut_set_params a clearance that is not finite, max_span outside 1 .. BL_SHORTCUT_MAX_POINTS,
 *     waypoint_cost outside 0 .. BL_SHORTCUT_MAX_WAYPOINT_COST (the handle keeps what it had); by the calls more than
 *     BL_SHORTCUT_MAX_PATHS paths, a path of more than BL_SHORTCUT_MAX_POINTS cells, offsets that do not start at 0 or decrease, a
 *     cell or a pose off the grid, a bl_dist of another ctx.  BL_ERR_STATE before bl_shortcut_set_params.
 *   Pose form (bl_shortcut_poses): cell k is global_position_to_grid_cell of pose k, inside the grid by the test bl_navfield_paths
 *     applies to a start pose.  Kept poses keep x, y and utime bit for bit; pose 0 keeps its theta; a kept pose k_s, s >= 1, gets
 *     theta = (float)atan2((double)DY, (double)DX) of the cell difference to the previous kept pose (the host's libm, on the host);
 *     where both differences are 0 it keeps its own theta.  Pose 0 (a robot pose) may lie up to half a cell from its cell's
 *     centre; the cover is taken from the centre, so the first segment is checked as if the robot stood there.
 * How it is computed (bl_shortcut.hip): k_sc_visible, one launch for all paths, fills a bit matrix vis[path][j][bit j - i]; a wave
 * takes one j and 64 consecutive spans j - i, walks from cell j along the major axis -- per major step the covered minor cells are at
 * most 3, found from a carried cross product, no division -- and leaves at the first cell that is not ok.  The ok bits of a path's
 * bounding box (bw x bh cells) are staged in LDS, rows padded to 32 bits:
 *   path 0 (staged) iff ((bw + 31) / 32 * 4) * bh <= BL_SHORTCUT_WINDOW_BYTES for every path of the call, path 1 (n(c) and the table
 *   read through L2) otherwise.  The rule decides speed only.
 * k_sc_dp, a workgroup per path: cost[] in LDS, j serial, the lanes take the i of the window, L by a double sqrt corrected by
 * integer compares, the least key (cost, i) by wave shuffles and one LDS hop; its last thread walks pred and writes the kept
 * indices ascending.  No atomics.  Calls are stream-ordered on the ctx stream, with one synchronisation, at the return. */
#define BL_SHORTCUT_WINDOW_BYTES (64 * 1024)
#define BL_SHORTCUT_MAX_POINTS 8192
#define BL_SHORTCUT_MAX_PATHS 4096
#define BL_SHORTCUT_MAX_WAYPOINT_COST 1048576
typedef struct bl_shortcut_params_t {
    double clearance;                  /* metres, finite: a segment runs over cells farther than this from any obstacle */
    int32_t max_span;                  /* 1 .. BL_SHORTCUT_MAX_POINTS: the longest j - i of an edge */
    int32_t waypoint_cost;             /* 0 .. BL_SHORTCUT_MAX_WAYPOINT_COST, in 1/1024 cell: what one more waypoint is worth */
} bl_shortcut_params_t;                /* 16 bytes */
typedef struct bl_shortcut bl_shortcut;
int bl_shortcut_create(bl_ctx* ctx, bl_shortcut** out);               /* buffers grow on demand */
void bl_shortcut_destroy(bl_shortcut* sc);
int bl_shortcut_set_params(bl_shortcut* sc, const bl_shortcut_params_t* params);   /* refused: the handle keeps what it had */
/* P paths: path p is the cells xy[2 * k], xy[2 * k + 1] for k = offsets[p] .. offsets[p + 1] - 1 (offsets[0] == 0).  out_keep has
 * room for offsets[P] indices: path p's kept indices (into its own cells) start at out_keep[offsets[p]], out_counts[p] of them.
 * out_cost: 2 per path, the shortened path's cost and the input path's. */
int bl_shortcut_cells(bl_shortcut* sc, const bl_dist* dist, const int32_t* xy, const int32_t* offsets, int P, int32_t* out_keep,
                      int32_t* out_counts, int64_t* out_cost);
/* P paths of poses: path p is paths[p * cap_each .. + lens[p]); the kept poses go to out_paths + p * cap_each, out_lens[p] of them.
 * out_cost (optional) as above. */
int bl_shortcut_poses(bl_shortcut* sc, const bl_dist* dist, const bl_pose_xyt_t* paths, int cap_each, const int* lens, int P,
                      bl_pose_xyt_t* out_paths, int* out_lens, int64_t* out_cost);
/* the edges of one path of m <= 512 cells: out[j * m + i] = 1 iff (i, j) is an edge, 0 elsewhere (m * m bytes) */
int bl_shortcut_debug_visible(bl_shortcut* sc, const bl_dist* dist, const int32_t* xy, int m, uint8_t* out);
/* which path the last k_sc_visible launch took: 0 the window staged in LDS, 1 the grids read directly; -1 before the first */
int bl_shortcut_debug_path(const bl_shortcut* sc);
/* device time of the last bl_shortcut_cells / bl_shortcut_poses, and of its k_sc_visible launches alone (ms_visible may be NULL):
 * HIP events around the launches; BL_ERR_STATE before the first */
int bl_shortcut_last_device_ms(const bl_shortcut* sc, float* ms, float* ms_visible);

/* ------------------------------------------------------------------ likelihood field (no reference counterpart)
 * A smoothed map for whatever scores ray end points: every cell holds a Gaussian of its distance to the nearest occupied cell
 * (Probabilistic Robotics 6.4; AMCL's likelihood-field model).  The sensor model of bl_pf_update* and the scan matcher score a
 * ray by the one cell its end point falls into; on a map whose walls are a cell or two thick that score is a needle around the
 * true pose and a noisy plateau everywhere else.  On the field it falls off smoothly over max_cells cells.
 *   Sources: the cells of the map with log-odds >= occ_min.  (The Euclidean distance grid's sources are log-odds >= 0: here an
 *     unknown cell at 0 must not attract rays.)  Cells off the grid are no sources.
 *   Code: d2(c) = the minimum over the sources of dx^2 + dy^2, in exact integers; code(c) = d2 when d2 <= R^2, else
 *     FAR = R^2 + 1 (R = max_cells).  A map without a source has code FAR everywhere.
 *   Table: T[k] = (int8) floor(peak * exp(-(k * m^2) / (2 s^2)) + 0.5) for k = 0 .. R^2, with m = (double)meters_per_cell of the
 *     map and s = (double)sigma, formed in double on the host with the C library's exp;  T[R^2 + 1] = 0.  R^2 + 2 entries;
 *     T[0] = peak.
 *   Field: field(c) = T[code(c)]: 0 .. peak, never negative.  A map without a source gives 0 everywhere.
 *   Result: a bl_grid owned by the handle, with the map's shape and the map's frame (metres per cell, cells per metre, origin) as
 *     of the call.  The grid object stays the same from call to call while the shape stays the same; a compute on a map of
 *     another shape destroys it and makes a new one (pointers to the old one dangle).  Every compute starts a new lineage of that
 *     grid and marks its zero-framed mirror stale, as an upload does: a filter update after a recompute scores the new field.
 *   It is an int8 grid like any other, and everything that scores ray end points against a const bl_grid* takes it as it
 *     stands: bl_pf_update / bl_pf_update_begin (a value v > 0 scores as the log-odds v does) and bl_scanmatch_match,
 *     _match_prior and _match_wide (they score max(cell, 0)).
 *   What the field is NOT: a map.  It has no free / unknown distinction -- every cell away from a wall is 0, which an occupancy
 *     grid reads as "unknown" -- and no negative cell.  bl_pf_init_uniform, bl_pf_set_recovery, bl_mapping_update*, the
 *     frontiers, the view gain and the distance grids keep taking the real map; nothing enforces this.
 *   bl_lfield_compute is three launches on the ctx stream (the source word's reset, a row pass, a column pass that ends in the
 *     table look-up) and waits for nothing on the host, except that a compute whose table differs from the last one's (other
 *     parameters, another meters_per_cell) first waits for that earlier table's upload.  Integers only on the device.
 *   Refused with BL_ERR_ARG: by bl_lfield_set_params a sigma that is not finite or not > 0, max_cells outside
 *     1 .. BL_LFIELD_MAX_CELLS, occ_min or peak outside 1 .. 127 (the handle keeps what it had); by bl_lfield_compute a null
 *     pointer, a map of another ctx, a map wider than 65536 cells.  BL_ERR_STATE: compute before bl_lfield_set_params, table and
 *     last_device_ms before the first compute. */
#define BL_LFIELD_MAX_CELLS 64
typedef struct bl_lfield_params_t {
    float sigma;                       /* metres, finite, > 0 */
    int32_t max_cells;                 /* R: 1 .. BL_LFIELD_MAX_CELLS */
    int32_t occ_min;                   /* 1 .. 127: a cell is a source when its log-odds is >= occ_min */
    int32_t peak;                      /* 1 .. 127: the field's value on a source */
} bl_lfield_params_t;                  /* 16 bytes */
typedef struct bl_lfield bl_lfield;
int bl_lfield_create(bl_ctx* ctx, bl_lfield** out);
void bl_lfield_destroy(bl_lfield* lf);                                 /* destroys the field grid with it */
int bl_lfield_set_params(bl_lfield* lf, const bl_lfield_params_t* params);   /* refused: the handle keeps what it had */
int bl_lfield_compute(bl_lfield* lf, const bl_grid* map);
const bl_grid* bl_lfield_grid(const bl_lfield* lf);                    /* NULL before the first compute */
/* the table of the last compute: *n = R^2 + 2, and those n entries to T unless T is NULL (room for up to 4098) */
int bl_lfield_table(const bl_lfield* lf, int8_t* T, int* n);
/* device time of the last bl_lfield_compute: HIP events around its launches (waits for that compute to finish) */
int bl_lfield_last_device_ms(const bl_lfield* lf, float* ms);

/* ------------------------------------------------------------------ obstacle layer (no reference counterpart)
 * What the scan sees and the map does not.  Every planner reads a bl_dist, which comes from a bl_grid: whatever stands in mapped
 * free space -- a box, a person, a second robot -- does not exist for them when the map is a loaded one, and under SLAM appears only
 * after enough scans and stays behind as a trail.  The layer is the fast, transient state beside the slow map: the beam model's
 * "short reading" (a return that ends in mapped free space with nothing mapped in front of it) found by casting the scan against
 * the static map, a per-cell hit / clear / expire state, and an int8 grid composed of map and layer that goes wherever the map
 * went.
 *   State, for a layer of width x height cells: count (uint8) and last (uint32, 0 = never hit) per cell, one update counter n
 *     (uint32, 0 at creation).  A map of another shape is refused (BL_ERR_ARG).
 *   bl_obslayer_update(layer, map, scan, pose) sets n = n + 1 and then:
 *   a. Rays.  The valid rays are the scan matcher's: 0.15f < range < max_range.  Geometry is the scan matcher's at heading step 0,
 *     one pose for the whole scan (no moving-scan interpolation), float32 with one rounding per operation:
 *       (px, py) = ((float)(((double)x - origin_x) * cells_per_meter), likewise y)           the matcher's grid position
 *       a = wrap_to_pi(theta - theta_r);  fx = (range * cosf(a)) * cells_per_meter + px;  fy likewise with sinf
 *       has = |fx| < 2^30 and |fy| < 2^30;  start cell s = (trunc(px), trunc(py));  end cell e = (trunc(fx), trunc(fy)).
 *   b. Walk.  Cells k = 0 .. K - 1, K = max(|dx|, |dy|), of the reference's Bresenham variant from s to e (mapping.cpp:101-127),
 *     start included, end excluded: the major axis advances k, the minor floor((2 k dmin + dmaj) / (2 dmaj)).  A static cell is
 *     occupied iff its log-odds is >= occ_min.  Cells outside the grid are skipped everywhere: neither occupied nor cleared.
 *     first = the least k whose cell is inside the grid and occupied, else K.
 *   c. Class, of every ray of the scan in scan order:
 *       BL_OBS_OFF 0        not valid, or has false
 *       BL_OBS_EXPLAINED 1  some occupied cell of the grid lies within Chebyshev distance tol_cells of e (e itself may lie outside)
 *       BL_OBS_THROUGH 3    not explained and first < K: the return contradicts map and pose; it contributes nothing
 *       BL_OBS_NOVEL 2      not explained, first == K, e inside the grid
 *       BL_OBS_OUTSIDE 4    not explained, first == K, e outside the grid
 *   d. Sets and transition.  C = the in-grid walk cells k < first of the rays of class 1, 2 and 4;  Hs = the end cells of the
 *     class-2 rays.  Both are sets (a cell hit by five rays is hit once), so the transition depends neither on the order of the
 *     rays nor on the launch shape:
 *       c in Hs:      count = (last != 0 and n - last < ttl_scans) ? min(count + 1, 255) : 1;  last = n     (a hit beats a clear)
 *       c in C \ Hs:  count = 0;  last = 0
 *       otherwise unchanged.
 *     live(c) = count >= min_hits and last != 0 and n - last < ttl_scans, with the current n (n - last in uint32 arithmetic).
 *     Rays at or beyond max_range neither hit nor clear: expiry is what removes an obstacle that left with nothing behind it.
 *   bl_obslayer_compose(layer, map, out): out(c) = 127 where live(c), else map(c).  `out` is another bl_grid of the same shape; it
 *     takes the map's frame.  Every compose starts a new lineage of `out` and marks its zero-framed mirror stale, as an upload does,
 *     so an incremental bl_dist_set_distances and the filter's mirror never see the previous composition.
 *   Refused with BL_ERR_ARG: by bl_obslayer_set_params a max_range that is not finite or not > 0.15, occ_min outside 1 .. 127,
 *     tol_cells outside 0 .. 16, ttl_scans outside 1 .. 65535, min_hits outside 1 .. 255 (the handle keeps what it had); by
 *     bl_obslayer_update a map of another shape or ctx, ceil((double)max_range * cells_per_meter) > 4096, more than 4096 valid
 *     rays, a pose member that is not finite (n and the state are untouched); by bl_obslayer_compose an `out` that is the map or
 *     of another shape.  BL_ERR_STATE: update, compose, stats and live_cells before bl_obslayer_set_params; update when
 *     n == 2^32 - 1 (n and the state are untouched; bl_obslayer_reset starts over); last_device_ms for a call not yet made.
 *   Calls are stream-ordered on the ctx stream and wait for nothing on the host, except that an update first waits for the
 *     previous update's scan to have left its pinned block; the readers (classes, stats, live_cells, download) synchronise.
 *   What the layer is not: a tracker (no velocities), and nothing here touches the map update, the filter, the navigation field or
 *     the local planner -- they take the composed grid as they take any bl_grid. */
#define BL_OBSLAYER_MAX_RAYS 4096
#define BL_OBSLAYER_MAX_REACH 4096     /* cells: ceil(max_range * cells_per_meter) */
#define BL_OBSLAYER_MAX_TOL 16
#define BL_OBS_OFF 0
#define BL_OBS_EXPLAINED 1
#define BL_OBS_NOVEL 2
#define BL_OBS_THROUGH 3
#define BL_OBS_OUTSIDE 4
typedef struct bl_obslayer_params_t {
    float max_range;                   /* metres, finite, > 0.15 */
    int32_t occ_min;                   /* 1 .. 127: a static cell is occupied when its log-odds is >= occ_min */
    int32_t tol_cells;                 /* 0 .. 16: a return this close (Chebyshev) to an occupied cell is the map's */
    int32_t ttl_scans;                 /* 1 .. 65535: a cell not hit for this many updates is dead */
    int32_t min_hits;                  /* 1 .. 255: hits in a row (none expired, none cleared) before a cell is live */
} bl_obslayer_params_t;                /* 20 bytes: offsets 0, 4, 8, 12, 16 */
typedef struct bl_obslayer_stats_t {
    uint32_t n;                        /* the update counter */
    int32_t valid_rays;                /* of the last update */
    int32_t rays_by_class[5];          /* of the last update, indexed by BL_OBS_* */
    int32_t hit_cells;                 /* |Hs| of the last update (0 after a reset or an upload) */
    int32_t cleared_cells;             /* |C \ Hs| of the last update (0 after a reset or an upload) */
    int32_t live_cells;                /* with the current n */
} bl_obslayer_stats_t;                 /* 40 bytes: offsets 0, 4, 8, 28, 32, 36 */
typedef struct bl_obslayer bl_obslayer;
int bl_obslayer_create(bl_ctx* ctx, int width, int height, bl_obslayer** out);
void bl_obslayer_destroy(bl_obslayer* layer);
int bl_obslayer_set_params(bl_obslayer* layer, const bl_obslayer_params_t* params);   /* refused: the handle keeps what it had */
int bl_obslayer_reset(bl_obslayer* layer);                             /* all cells never hit, n = 0 */
int bl_obslayer_update(bl_obslayer* layer, const bl_grid* map, const bl_lidar_t* scan, const bl_pose_xyt_t* pose);
int bl_obslayer_compose(bl_obslayer* layer, const bl_grid* map, bl_grid* out_grid);
/* the classes of the last update's rays, in scan order: *n_rays = the scan's num_ranges (0 before the first update and after a
 * reset), and that many bytes to `out` unless it is NULL */
int bl_obslayer_classes(bl_obslayer* layer, uint8_t* out, int* n_rays);
int bl_obslayer_stats(bl_obslayer* layer, bl_obslayer_stats_t* out);
/* the live cells in row-major order (y, then x) as x, y pairs: *count = how many there are, the first min(cap, *count) to xy */
int bl_obslayer_live_cells(bl_obslayer* layer, int32_t* xy, int cap, int* count);
/* the state: width * height entries each, row-major; any pointer may be NULL */
int bl_obslayer_download(bl_obslayer* layer, uint8_t* count, uint32_t* last, uint32_t* n);
/* Replaces the state.  For tests and for restoring a saved layer: saturation (count 255), expiry (n - last around ttl_scans) and the
 * counter's end (n = 2^32 - 1) are reached through it, not by millions of updates.  The sets of the last update are forgotten. */
int bl_obslayer_upload(bl_obslayer* layer, const uint8_t* count, const uint32_t* last, uint32_t n);
/* device time of the last update and of the last compose: HIP events around their launches (waits for them); either may be NULL */
int bl_obslayer_last_device_ms(const bl_obslayer* layer, float* update_ms, float* compose_ms);

/* ------------------------------------------------------------------ obstacle tracks (no reference counterpart)
 * Velocities for what the obstacle layer sees.  The layer says where a thing that the map lacks IS; a planner that rolls out ahead
 * over a grid frozen at the scan's instant avoids a walking person only once they stand in its way.  The tracks group the layer's
 * live cells into blobs, follow the blobs from update to update and paint where the moving ones are heading.
 * Integers throughout; tests/obstacle_tracks_model.py restates this comment.  Every parameter is an untuned knob.
 *   bl_obstracks_update(tr, layer) is called once after each bl_obslayer_update and reads the layer's state on the device.
 *   a. Blobs.  The live cells are the layer's live(c) at its current n.  A blob is a connected component of live cells under
 *     8-connectivity; its representative is the live cell of least flat index y * W + x; the blob's rank is the row-major order of
 *     the representatives.  Per blob: area A, sum_x, sum_y (int64), bounding box, centroid in 1/256 cell
 *     cx = floor(256 * sum_x / A) + 128, cy likewise.  eligible = min_cells <= A <= max_cells.  The first
 *     BL_OBSTRACKS_MAX_BLOBS blobs by rank are kept, the rest counted as dropped (their cells have label -1).
 *   b. Tracks.  BL_OBSTRACKS_MAX_TRACKS slots; a slot is free when its id is 0.  Per track: id (from 1, never reused), position
 *     (px, py) and velocity (vx, vy) in 1/256 cell, the velocity per update, hits and missed (both saturate at 65535), area and box
 *     of the last matched blob.  pred = pos + vel.
 *   c. Association: gated greedy nearest neighbour.  Candidates are (occupied slot i, eligible kept blob of rank j) with
 *     |pred_i - c_j|^2 = d2 <= (256 * gate_cells)^2; they are taken in ascending order of the key (d2, i, j), a pair being accepted
 *     when both ends are still free.
 *   d. Transition, in this order.  Matched, with r = c - pred per component: pos = pred + floor(alpha * r / 256),
 *     vel = clamp(vel + floor(beta * r / 256), -1023, 1023), hits + 1, missed = 0, box and area from the blob (floor rounds towards
 *     minus infinity).  Unmatched track: pos = pred, missed + 1; the slot is freed when missed > max_missed.  Births: each unmatched
 *     eligible kept blob, in rank order, takes the lowest free slot (one freed in this update included) with pos = its centroid,
 *     vel = 0, hits = 1, missed = 0 and the next id; blobs left without a slot are counted (unborn).
 *     Flags, set by every update for every occupied slot: BL_OBSTRACK_CONFIRMED hits >= confirm_hits, BL_OBSTRACK_MOVING
 *     vx^2 + vy^2 >= min_speed^2, BL_OBSTRACK_MATCHED and BL_OBSTRACK_BORN by what this update did with the slot.
 *   e. Order of calls.  The tracker remembers the layer's n.  An update is refused (BL_ERR_STATE) unless the layer's n is the
 *     remembered value + 1 or the tracker is fresh (created, reset, or uploaded as fresh).  After bl_obslayer_reset or
 *     bl_obslayer_upload the caller resets the tracker.
 *   Two refusals depend on what only the device knows, and the update waits for nothing on the host: they are found on the device,
 *     the update returns BL_OK, the tracks and the id counter stay as they were, there are no blobs (every label -1), and
 *     bl_obstracks_stats reports refused = BL_OBSTRACKS_REFUSED_CELLS (more than BL_OBSTRACKS_MAX_CELLS live cells) or
 *     BL_OBSTRACKS_REFUSED_IDS (a birth would need id 2^32 - 1; reached through upload, not by running).  The remembered n advances.
 *   f. bl_obstracks_compose(tr, layer, map, out, c): bl_obslayer_compose(layer, map, out) itself -- out(c) = 127 where live(c), else
 *     map(c), a new lineage, the mirror stale -- and then, for every live cell (x, y) of the last update whose blob was matched to or
 *     born as a track that is CONFIRMED and MOVING, for s = 1 .. 4 * horizon: the cell
 *     (x + floor((s * vx + 512) / 1024), y + floor((s * vy + 512) / 1024)) becomes 127 when it lies inside the grid and not
 *     within Chebyshev distance keep_clear of (robot_x, robot_y) (keep_clear -1: nothing is skipped).  Live cells are painted
 *     wherever they are.  Plain stores of one value.  horizon 0 is bl_obslayer_compose byte for byte.  With horizon > 0 the layer's n
 *     must be the remembered one (BL_ERR_STATE); after a reset or an upload and before the next update nothing is stamped.
 *   Refused with BL_ERR_ARG: parameters outside their ranges below (the handle keeps what it had); a layer of another shape or
 *     ctx; by upload an occupied slot whose id is not below next_id or is shared, |vx| or |vy| > 1023, |px| or |py| > 2^30, hits
 *     outside 1 .. 65535, missed outside 0 .. 255, next_id 0.  BL_ERR_STATE: update and compose before set_params on either handle,
 *     the order of calls, last_device_ms for a call not yet made.
 *   Calls are stream-ordered on the ctx stream; update and compose wait for nothing on the host; the readers synchronise. */
#define BL_OBSTRACKS_MAX_BLOBS 1024
#define BL_OBSTRACKS_MAX_CELLS 65536
#define BL_OBSTRACKS_MAX_TRACKS 256
#define BL_OBSTRACKS_MAX_HORIZON 64
#define BL_OBSTRACKS_MAX_KEEP_CLEAR 64
#define BL_OBSTRACKS_REFUSED_CELLS 1
#define BL_OBSTRACKS_REFUSED_IDS 2
#define BL_OBSTRACK_CONFIRMED 1
#define BL_OBSTRACK_MOVING 2
#define BL_OBSTRACK_MATCHED 4
#define BL_OBSTRACK_BORN 8
typedef struct bl_obstracks_params_t {
    int32_t min_cells;                 /* 1 .. 65536 */
    int32_t max_cells;                 /* min_cells .. 65536 */
    int32_t gate_cells;                /* 1 .. 64 */
    int32_t alpha;                     /* 0 .. 256: position gain in 1/256 */
    int32_t beta;                      /* 0 .. 256: velocity gain in 1/256 */
    int32_t confirm_hits;              /* 1 .. 255 */
    int32_t max_missed;                /* 0 .. 255 */
    int32_t min_speed;                 /* 0 .. 1023, 1/256 cell per update */
} bl_obstracks_params_t;               /* 32 bytes: offsets 0, 4, 8, 12, 16, 20, 24, 28 */
typedef struct bl_obstracks_compose_t {
    int32_t horizon;                   /* 0 .. 64 updates ahead, four sub-steps each */
    int32_t robot_x, robot_y;          /* the robot's cell (any value; read only when keep_clear >= 0) */
    int32_t keep_clear;                /* -1 .. 64 */
} bl_obstracks_compose_t;              /* 16 bytes: offsets 0, 4, 8, 12 */
typedef struct bl_obstrack_t {
    uint32_t id;                       /* 0: the slot is free */
    int32_t px, py, vx, vy;            /* 1/256 cell; the velocity per update */
    int32_t hits, missed;
    int32_t area, x0, y0, x1, y1;      /* of the last matched blob (box inclusive) */
    int32_t flags;                     /* BL_OBSTRACK_* */
    int32_t slot;
} bl_obstrack_t;                       /* 56 bytes: offsets 0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44, 48, 52 */
typedef struct bl_obsblob_t {
    int64_t sum_x, sum_y;
    int32_t area, x0, y0, x1, y1;      /* box inclusive */
    int32_t cx, cy;                    /* 1/256 cell */
    int32_t eligible;                  /* 0 or 1 */
    int32_t track;                     /* the slot it was matched to or born as, else -1 */
    int32_t rep;                       /* flat index of the representative */
} bl_obsblob_t;                        /* 56 bytes: offsets 0, 8, 16, 20, 24, 28, 32, 36, 40, 44, 48, 52 */
typedef struct bl_obstracks_stats_t {
    uint32_t n;                        /* the remembered layer counter */
    uint32_t next_id;
    int32_t live_cells;                /* of the last update */
    int32_t blobs, eligible, dropped;  /* all blobs; eligible among the kept; beyond BL_OBSTRACKS_MAX_BLOBS */
    int32_t matched, born, deleted, unborn;
    int32_t tracks, confirmed;         /* occupied slots, and the confirmed among them */
    int32_t refused;                   /* 0, or BL_OBSTRACKS_REFUSED_* of the last update */
    int32_t rounds;                    /* mutual-best rounds of the last update that accepted a pair */
} bl_obstracks_stats_t;                /* 56 bytes: offsets 0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44, 48, 52 */
typedef struct bl_obstracks_state_t {
    uint32_t n;                        /* the remembered layer counter */
    uint32_t next_id;                  /* >= 1 */
    int32_t fresh;                     /* 1: the next update takes any n */
    int32_t reserved;                  /* 0 */
} bl_obstracks_state_t;                /* 16 bytes: offsets 0, 4, 8, 12 */
typedef struct bl_obstracks bl_obstracks;
int bl_obstracks_create(bl_ctx* ctx, int width, int height, bl_obstracks** out);
void bl_obstracks_destroy(bl_obstracks* tr);
int bl_obstracks_set_params(bl_obstracks* tr, const bl_obstracks_params_t* params);   /* refused: the handle keeps what it had */
int bl_obstracks_reset(bl_obstracks* tr);                              /* no tracks, no blobs, ids from 1 again, fresh */
int bl_obstracks_update(bl_obstracks* tr, bl_obslayer* layer);
int bl_obstracks_compose(bl_obstracks* tr, bl_obslayer* layer, const bl_grid* map, bl_grid* out_grid, const bl_obstracks_compose_t* c);
/* The composition that leaves the moving obstacles out (for bl_localplan_commands_moving below, which times them itself):
 * out(c) = 127 where live(c), unless the cell's blob of the last update was matched to or born as a track that is CONFIRMED and
 * MOVING -- bl_obstracks_compose's predicate: label, blob, slot, flags --; those cells, like every other cell, are map(c).  Lineage
 * and mirror as bl_obslayer_compose.  The layer's n must be the remembered one (BL_ERR_STATE) unless the tracker is fresh; after a
 * reset or an upload and before the next update there are no blobs and it is bl_obslayer_compose byte for byte.  The refusals are
 * bl_obstracks_compose's; it waits for nothing on the host. */
int bl_obstracks_compose_static(bl_obstracks* tr, bl_obslayer* layer, const bl_grid* map, bl_grid* out_grid);
/* the occupied slots in slot order: *count = how many, the first min(cap, *count) to out */
int bl_obstracks_tracks(bl_obstracks* tr, bl_obstrack_t* out, int cap, int* count);
/* the kept blobs of the last update in rank order: *count = how many, the first min(cap, *count) to out */
int bl_obstracks_blobs(bl_obstracks* tr, bl_obsblob_t* out, int cap, int* count);
/* per live cell of the last update, in the layer's row-major list order: its blob's rank, -1 when the blob was dropped */
int bl_obstracks_labels(bl_obstracks* tr, int32_t* out, int cap, int* count);
int bl_obstracks_stats(bl_obstracks* tr, bl_obstracks_stats_t* out);
/* the whole state: all BL_OBSTRACKS_MAX_TRACKS slots and the counters.  The blobs belong to an update: an upload forgets them. */
int bl_obstracks_download(bl_obstracks* tr, bl_obstrack_t* slots, bl_obstracks_state_t* state);
int bl_obstracks_upload(bl_obstracks* tr, const bl_obstrack_t* slots, const bl_obstracks_state_t* state);
/* device time of the last update and of the last compose: HIP events around their launches (waits for them); either may be NULL */
int bl_obstracks_last_device_ms(const bl_obstracks* tr, float* update_ms, float* compose_ms);

/* ------------------------------------------------------------------ local planner, moving obstacles (no reference counterpart)
 * bl_localplan_commands with the rollout timed against the tracked moving obstacles: step k of a rollout is a time, and a candidate
 * is refused when its cell at step k lies in a moving track's box AT step k.  bl_obstracks_compose stamps the whole
 * sweep of a moving track into the grid as a wall that stands from the first step to the last; here the field is computed over
 * bl_obstracks_compose_static, which leaves the moving obstacles out, and the rollout meets them where they will be.
 * tests/local_plan_moving_model.py restates this comment.  Integers for everything compared.
 *   The kernel reads the tracker's BL_OBSTRACKS_MAX_TRACKS slots on the device and nothing else of it: no blobs, no labels.  The
 *     slots are those the last bl_obstracks_update or bl_obstracks_upload left, flags included.
 *   A slot is used when id != 0, it is CONFIRMED and MOVING, and it is MATCHED or BORN (a coasting track's box is stale) -- the flags
 *     as they stand in the slot.
 *   The box of a used slot: x0, y0, x1, y1 each clamped to [-2^30, 2^30] first (so that no uploadable slot overflows), then with
 *     q = steps_per_update, t = k + lead_steps for the rollout step k = 1 .. n_steps:
 *       ox = floor((t * vx + 128 * q) / (256 * q)), oy likewise      (floor towards minus infinity; |t * vx| < 2^20)
 *       [x0 + ox - margin_cells, x1 + ox + margin_cells] x [y0 + oy - margin_cells, y1 + oy + margin_cells]
 *   A candidate is admissible when, in addition to bl_localplan_commands' rule, no visited cell cell_k lies in any used slot's box
 *     at step k.  Everything else is the local planner's definition word for word: the tables, the float arc, the cost, the key
 *     (cost, c), REACHED and OFF_FIELD decided on the pose's own cell alone before anything is rolled out (a box over the pose's cell
 *     gives BLOCKED, not OFF_FIELD), BLOCKED, n_admissible, the refusals.  With no used slot the results are
 *     bl_localplan_commands' byte for byte.
 *   Refused with BL_ERR_ARG beyond bl_localplan_commands' refusals: steps_per_update outside 1 .. 255, margin_cells outside
 *     0 .. 64, lead_steps outside 0 .. 255, reserved != 0, a tracker of another ctx or of another shape than the field's grid.
 *     BL_ERR_STATE before the tracker's bl_obstracks_set_params.  n == 0 is fine.  One synchronisation, at the return.
 *   bl_localplan_debug_costs_moving: costs as bl_localplan_debug_costs under the moving rule; first_hit[c] the least k whose visited
 *     cell lies in a used box, 0 when there is none -- looked for at every k whose pose has a cell, whether or not another rule has
 *     already refused the candidate.  Either pointer may be NULL.
 * How it is computed (k_lp_rollout<STAGED, MOVING>): per workgroup a lane per slot decides used and can-reach -- the box swept over
 * k = 1 .. n_steps (the offsets are monotone in k, so the two ends bound it) meets the square of half side R around the window's
 * centre, R the window rule's --; the kept slots are compacted in slot order into LDS.  A visited cell outside that square (the
 * bound on the reach is floating point) is tested against all used slots, so the cull decides speed only.  Box positions:
 *   path 0 (table) iff kept * n_steps * 8 <= BL_LOCALPLAN_MOVING_BYTES: the kept boxes at every step, clamped to the square, as
 *     4 x int16 in LDS, filled once per workgroup; a candidate's step reads one entry per box;
 *   path 1 (per step) otherwise: the floor divisions are done per candidate, step and box;
 *   path 2: no used slot was kept.
 * bl_localplan_debug_moving_path: the path of the last moving call (of its first state that was rolled out; 2 when none was), -1
 * before the first. */
#define BL_LOCALPLAN_MOVING_BYTES (10 * 1024)
#define BL_LOCALPLAN_MAX_MARGIN 64
typedef struct bl_localplan_moving_t {
    int32_t steps_per_update;          /* 1 .. 255: rollout steps of dt_sim in one tracker update */
    int32_t margin_cells;              /* 0 .. 64 */
    int32_t lead_steps;                /* 0 .. 255: rollout steps already elapsed since the tracker's last update */
    int32_t reserved;                  /* 0 */
} bl_localplan_moving_t;               /* 16 bytes: offsets 0, 4, 8, 12 */
int bl_localplan_commands_moving(bl_localplan* lp, bl_navfield* nf, bl_obstracks* tr, const bl_localplan_moving_t* m,
                                 const bl_localplan_state_t* states, int n, bl_localplan_result_t* results);
int bl_localplan_debug_costs_moving(bl_localplan* lp, bl_navfield* nf, bl_obstracks* tr, const bl_localplan_moving_t* m,
                                    const bl_localplan_state_t* state, int64_t* costs, int32_t* first_hit);
int bl_localplan_debug_moving_path(const bl_localplan* lp);

/* ------------------------------------------------------------------ sampling local planner (no reference counterpart)
 * Model-predictive path-integral control (MPPI) over a navigation field: K perturbed control SEQUENCES of T periods are drawn around a
 * nominal sequence, each is rolled out by the local planner's unicycle step, and the softmin-weighted average of the admissible ones
 * is the new sequence, warm-started from the previous tick.  bl_localplan_commands scores constant (v, w) arcs; a
 * sequence can turn on the spot and then drive, or slow down, let a tracked box cross and accelerate.  tests/mppi_model.py restates
 * this comment.  Everything compared or summed is an integer: the result depends on no launch shape and no reduction order.
 *   Fixed point: controls are int32 in units of 2^-16 (m/s, rad/s).  q16(x) = (int32)lrint((double)x * 65536.0), ties to even.
 *   Derived once on the host: vmin_q, vmax_q, wmax_q, nv_q, nw_q by q16 of v_min, v_max, w_max, noise_v, noise_w;
 *     av_q = (int32)lrint((double)acc_v * (double)dt_sim * n_sub * 65536.0), aw_q likewise from acc_w: the change a control period allows.
 *   Refused with BL_ERR_ARG by bl_mppi_set_params: a non-finite value, v_min > v_max, w_max < 0, a noise < 0, an acc < 0, dt_sim <= 0,
 *     any of the seven derived values with magnitude >= 2^21, n_samples outside 1 .. 16384, horizon outside 1 .. 64, n_sub outside
 *     1 .. 16, horizon * n_sub > 255, lambda outside 1 .. 2^30, a weight outside 0 .. 65535; by the calls that see the field
 *     (double)max(|v_min|, |v_max|) * (double)dt_sim > (double)meters_per_cell (a step may not skip a cell); a state the local planner
 *     refuses, or one with |q16(v)| or |q16(w)| >= 2^21.  `pad` is not read.
 *   Sequences, in and out, are int32 [n][T][2], channel 0 v and 1 w.  A NULL seq_in is all zeros.
 *   Sample k = 0 .. K-1 of a state, control period t = 0 .. T-1:
 *     (a0, a1, a2, a3) = bl_philox4x32 of counter (k, t, state.stream, state.tick) and key (seed low word, seed high word)
 *     e_v = lo16(a0) + hi16(a0) + lo16(a1) + hi16(a1) - 131070, e_w the same of a2, a3: Irwin-Hall of four, -131070 .. 131070, so the
 *       perturbation's standard deviation is about 0.2887 * noise
 *     raw = u_in[t] + (((int64)e * noise_q) >> 17), the shift arithmetic (floor), raw an int64.  Sample 0 has e = 0 (the nominal);
 *       when K >= 2, sample 1 has raw = 0 (brake).
 *     the clamp chain, per channel, prev = q16(state.v) (or w) before t = 0: lo = max(limit_lo, prev - a_q), hi = min(limit_hi,
 *       prev + a_q); if lo > hi both become prev clamped to the limits; q = min(max(raw, lo), hi); prev = q.  The limits are
 *       vmin_q, vmax_q and -wmax_q, wmax_q.
 *   Rollout of a sequence, the local planner's step word for word: theta = wrap_to_pi(pose.theta); per period v = (float)q_v * 2^-16f,
 *     s = v * dt_sim, dth = (float)q_w * 2^-16f * dt_sim, then n_sub steps of (cs, sn) = cosf, sinf of theta; x = x + s * cs;
 *     y = y + s * sn; theta = wrap_to_pi(theta + dth); the visited cell by global_position_to_grid_cell.  T * n_sub steps in all.
 *   Admissible as in bl_localplan_commands: every visited cell inside and traversable, field(e) != UNREACHED at the last one.
 *     cost = w_field * field(e) + w_heading * h + w_clear * (sum of penalties), int64, h the local planner's heading term.
 *   Weights: (c_min, best) the least key (cost, k) over admissible samples; idx = min((cost_k - c_min) * 16 / lambda, 256);
 *     W_k = table[idx], 0 for an inadmissible sample; table[0] = 2^24, table[i] = (table[i-1] * 4034748382) >> 32 for i <= 255
 *     (the constant is floor(2^32 e^(-1/16)); the recurrence is the definition), table[256] = 0.  S = sum W and Q = sum W^2 in uint64;
 *     per (t, channel) N = sum W_k q_k in int64; a = floor((2 N + S) / (2 S)), floor towards minus infinity.
 *   Output: a through the clamp chain (raw = a) is the candidate sequence; it is rolled out; if admissible it is seq_out and cost_out
 *     its cost; otherwise seq_out is sample best's sequence, cost_out = cost_best and flags = BL_MPPI_FELL_BACK.  (The average of two
 *     ways round a pillar goes through the pillar.)  trans_v, angular_v = seq_out[0] * 2^-16.
 *   REACHED, OFF_FIELD, BLOCKED: the local planner's rules and values, decided on the pose's own cell before anything is drawn
 *     (BLOCKED: no admissible sample); each with the command (0, 0), a zero seq_out, index_best -1, zero weight sums; both costs 0
 *     with REACHED and INT64_MAX with the other two; n_admissible 0.
 *   Moving obstacles: tr and m are both NULL or both set (else BL_ERR_ARG).  Set: bl_localplan_commands_moving's admissibility rule
 *     word for word -- used slots, the clamped box, ox / oy by floor division, the margin -- with k = 1 .. T * n_sub the integration
 *     step, applied to the samples and to the candidate sequence's rollout; that call's refusals.  With no used slot the results are
 *     the static call's byte for byte.
 *   bl_mppi_debug_samples: the K costs of one state (INT64_MAX: inadmissible), rolled out whatever the state's flags would be;
 *     first_hit[k] as bl_localplan_debug_costs_moving's (all 0 without a tracker); seqs the K sequences.  Either of the last two may
 *     be NULL.  bl_mppi_debug_rollout: the T * n_sub poses of `seq` ([T][2], NULL: zeros; taken as given, no clamp chain; an entry
 *     with magnitude >= 2^21 is refused).
 * How it is computed (bl_mppi.hip): no sequence is stored; a sample's sequence is regenerated from Philox and the two prev registers
 * wherever it is needed.  k_mppi_rollout<STAGED, MOVING>: a thread per sample, a workgroup per (state, 256 samples); the window of the
 * rollouts' reach staged in LDS by the local planner's window rule with n_steps = T * n_sub (bl_mppi_debug_path: 0 staged, 1 grids);
 * the used slots compacted into LDS in slot order; cost[k] and the least key per workgroup.  k_mppi_average: the weights and the
 * 2 T + 2 integer sums per workgroup by wave shuffles, then LDS.  k_mppi_finish, a workgroup per state: the sums, the divisions, the
 * clamp chain, the candidate's rollout and the fall-back.  No atomics.  One synchronisation, at the return. */
#define BL_MPPI_MAX_SAMPLES 16384
#define BL_MPPI_MAX_HORIZON 64
#define BL_MPPI_MAX_SUB 16
#define BL_MPPI_MAX_STEPS 255
#define BL_MPPI_MAX_LAMBDA (1 << 30)
#define BL_MPPI_MAX_Q (1 << 21)
#define BL_MPPI_FELL_BACK 8
typedef struct bl_mppi_params_t {
    float v_min, v_max, w_max;         /* m/s, m/s, rad/s */
    float acc_v, acc_w;                /* m/s^2, rad/s^2, >= 0 */
    float dt_sim;                      /* s, > 0: the integration step; a control period is n_sub of them */
    float noise_v, noise_w;            /* m/s, rad/s, >= 0: the perturbation's scale */
    int32_t n_samples, horizon, n_sub; /* K 1 .. 16384, T 1 .. 64, 1 .. 16 with T * n_sub <= 255 */
    int32_t lambda;                    /* 1 .. 2^30: the softmin's temperature in cost units */
    int32_t w_field, w_heading, w_clear;   /* 0 .. 65535 each */
    int32_t pad;
    uint64_t seed;
} bl_mppi_params_t;                    /* 72 bytes: offsets 0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44, 48, 52, 56, 60, 64 */
typedef struct bl_mppi_state_t {
    bl_localplan_state_t s;
    uint32_t tick, stream;             /* Philox counter words: the control tick, and which robot or hypothesis draws */
} bl_mppi_state_t;                     /* 40 bytes: offsets 0, 32, 36 */
typedef struct bl_mppi_result_t {
    float trans_v, angular_v;          /* seq_out[0] * 2^-16 */
    int32_t index_best, n_admissible;
    int64_t cost_best, cost_out;
    uint64_t weight_sum, weight_sq_sum;    /* S and Q: S * S / Q is the effective sample size */
    int32_t flags, pad;                /* BL_LOCALPLAN_REACHED / OFF_FIELD / BLOCKED, BL_MPPI_FELL_BACK */
} bl_mppi_result_t;                    /* 56 bytes: offsets 0, 4, 8, 12, 16, 24, 32, 40, 48, 52 */
typedef struct bl_mppi bl_mppi;
int bl_mppi_create(bl_ctx* ctx, bl_mppi** out);                       /* buffers grow on demand */
void bl_mppi_destroy(bl_mppi* mp);
int bl_mppi_set_params(bl_mppi* mp, const bl_mppi_params_t* params);  /* refused: the handle keeps what it had */
/* BL_ERR_STATE before set_params and for a field handle without a field; n == 0 is fine; seq_in may be NULL */
int bl_mppi_plan(bl_mppi* mp, bl_navfield* nf, bl_obstracks* tr, const bl_localplan_moving_t* m, const bl_mppi_state_t* states, int n,
                 const int32_t* seq_in, int32_t* seq_out, bl_mppi_result_t* results);
int bl_mppi_debug_samples(bl_mppi* mp, bl_navfield* nf, bl_obstracks* tr, const bl_localplan_moving_t* m, const bl_mppi_state_t* state,
                          const int32_t* seq_in, int64_t* costs, int32_t* first_hit, int32_t* seqs);
int bl_mppi_debug_rollout(bl_mppi* mp, bl_navfield* nf, const bl_mppi_state_t* state, const int32_t* seq, bl_pose_xyt_t* out);
void bl_mppi_weight_table(uint32_t out[257]);                         /* host arithmetic only */
/* which path the last rollout launch took: 0 the window staged in LDS, 1 the grids read directly; -1 before the first */
int bl_mppi_debug_path(const bl_mppi* mp);
/* device time of the last bl_mppi_plan's kernels (HIP events around the launches); BL_ERR_STATE before the first */
int bl_mppi_last_device_ms(const bl_mppi* mp, float* ms);

/* ------------------------------------------------------------------ beam model (no reference counterpart)
 * A ray-cast sensor model for the particle filter.  The reference's endpoint rule and the likelihood field score a ray by the cell it
 * ends in; a pose whose rays pass through a mapped wall and end on the next one scores as well as the true pose.  The beam model
 * (Probabilistic Robotics 6.3) casts every ray against the map as far as the maximum range and scores the measured range against
 * the expected one.  Off by default; nothing of the filter's update changes.  EVERY PARAMETER IS AN UNTUNED KNOB.
 *   Rays.  For one pose (x, y, theta) and one scan, ray r is DROPPED when range <= 0.15f or not finite, a RETURN when
 *     0.15f < range < max_range, a MAX READING when range >= max_range.  Of the non-dropped rays in scan order every ray_stride-th is
 *     USED, starting with the first; more than 4096 used rays are refused.
 *   Geometry.  The obstacle layer's step a: float32 with one rounding per operation, one pose for the whole scan,
 *       (px, py) = ((float)(((double)x - origin_x) * cells_per_meter), likewise y);  a = wrap_to_pi(theta - theta_r)
 *       start cell s = (trunc(px), trunc(py));  for a return the end cell e = (trunc(fx), trunc(fy)), fx = (range * cosf(a)) *
 *       cells_per_meter + px, fy likewise with sinf;  for every used ray the far cell m, the same expression with max_range in place of
 *       range.  has(f) = |fx| < 2^30 and |fy| < 2^30; a ray whose has is false for e (a return) or for m is dropped for this pose.
 *     A pose takes part when its three members are finite, |px| < 2^30, |py| < 2^30 and s lies inside the grid.
 *   Expected range.  The obstacle layer's walk (step b) from s to m, start included, end excluded, K = Chebyshev(s, m) cells.
 *     first = the least k whose cell is inside the grid and has log-odds >= occ_min, else K.  When first < K the ray has an
 *     EXPECTED HIT at walk cell c*.
 *   Lengths, in quarter cells: q(a, b) = isqrt(16 * ((ax - bx)^2 + (ay - by)^2)), exact.  z = q(e, s) for a return, z* = q(c*, s) for
 *     an expected hit.  reach = ceil((double)max_range * cells_per_meter) <= 4096 (else BL_ERR_ARG), so every value fits 32 bits.
 *   Per-ray probability p, a uint32.  For a return: Hit[min(|z - z*|, hit_cut)] when there is an expected hit, plus
 *     Short[min(z >> 2, 1023)] when there is no expected hit or z < z*, plus Rand.  For a max reading: MaxFree when there is no
 *     expected hit, else MaxBlocked.  The tables, made on the host in double (lround: ties away from zero) from the float32 members:
 *       Hit[d]   = lround(2^30 * z_hit * exp(-((d / 4) * (d / 4)) / (2 * sigma_cells * sigma_cells))),  d = 0 .. 1023
 *       Short[c] = lround(2^30 * z_short * lambda * exp(-lambda * c)),                                  c = 0 .. 1023
 *       Rand = max(1, lround(2^30 * z_rand / reach));  MaxFree = max(1, lround(2^30 * z_max));
 *       MaxBlocked = max(1, lround(2^30 * z_max * blocked_factor)).
 *     Rand depends on the map's cells_per_meter through reach; the others on the parameters alone (bl_beam_tables takes the
 *     cells_per_meter for this reason).  bl_beam_set_params refuses a set for which some p could be 0 or exceed 2^31 - 1.  Because the
 *     max(1, .) above would hide the first case, it is asked of the values before it: lround(2^30 * z_rand / 4096) (the largest legal
 *     reach), lround(2^30 * z_max) and lround(2^30 * z_max * blocked_factor) must each be >= 1; and Hit[0] + Short[0] +
 *     lround(2^30 * z_rand) (a reach of one cell), MaxFree and MaxBlocked must each be <= 2^31 - 1.
 *   Integer logarithm.  e = 31 - clz(p);  mant = ((p << (31 - e)) >> 23) & 255 (uint32 arithmetic);  lg(p) = (e - 30) * LN2 + LT[mant],
 *     LT[i] = lround(65536 * ln(1 + i / 256)), LN2 = lround(65536 * ln 2).
 *   Score.  S(pose) = the sum over the used, not dropped rays of lg(p), an int64 in Q16 nats.  A pose that takes no part scores
 *     BL_BEAM_OFF_GRID and is ignored by the maximum.  A scan without a used ray gives S = 0 for every pose that takes part.
 *   Weights, over the poses that take part: Smax the largest S;  j = min(256, ((Smax - S) * 256) / span) in int64;  units = U[j],
 *     U[j] = max(1, lround(2^20 * 2^(-20 j / 256))), so U[0] = 2^20 and U[256] = 1.  span is the score gap at which a particle reaches
 *     the floor: the tempering knob (beam models are overconfident).  A pose that takes no part gets 1 unit.
 *   bl_beam_reweigh_pf(beam, pf, map, scan, out_pose) scores the filter's posterior poses where they lie on the device (the active
 *     particles of the current record), replaces their weight units in place -- poses and parents untouched -- rescans the weights and
 *     ends with what bl_pf_estimate_posterior_pose does: poseEstimate() is then the beam-weighted mean.  The units count as an UPLOAD
 *     of unequal units (bl_pf_set_particles): neither the equal-weight rule nor the all-floor rule of a sensor update applies to
 *     them, whatever their values.  The recovery tracker (bl_pf_set_recovery) never folds them either: with recovery on, the weight
 *     total of the sensor update that produced the record is kept aside before its units are replaced, and that total is what the
 *     tracker folds at the start of the next moved update, as it would have without the call.  With recovery off the record counts as
 *     an upload for the tracker too (nothing of it is folded, also when recovery is turned on before the next update).
 *   Refused with BL_ERR_ARG: by bl_beam_set_params a member that is not finite, max_range <= 0.15, sigma_cells <= 0, a negative z_*,
 *     lambda or blocked_factor, any of them with 2^30 * value > 2^31, occ_min outside 1 .. 127, hit_cut outside 1 .. 1023, span
 *     outside 1 .. 2^40, ray_stride outside 1 .. 64, and the two conditions on p (the handle keeps what it had); by the calls that
 *     take a map a map of another ctx, reach outside 1 .. 4096, more than 4096 used rays (nothing is enqueued).  BL_ERR_STATE: the
 *     calls that take a map, and bl_beam_tables, before bl_beam_set_params; bl_beam_units and bl_beam_last_device_ms
 *     before the first scores / reweigh_pf; bl_beam_reweigh_pf for a filter that is not initialised, has a pending
 *     bl_pf_update_begin, or is sharded.
 *   How it is computed (bl_beam.hip): k_beam_cast, a workgroup per 32 poses, a wave per 4 of them in turn, a lane per ray that walks
 *     the reference's Bresenham loop and stops at its first occupied cell; the cells from the grid through L2 (bl_beam_debug_path 1, the
 *     default: measured faster) or, under bl_beam_debug_set, from an LDS window when the bounding box of the workgroup's start cells
 *     widened by reach + 2 fits 40 KB (0; 2: both in one launch);
 *     k_beam_final, one workgroup, Smax from the workgroups' records; k_beam_units.  No atomics.  Calls are stream-ordered on the ctx
 *     stream; bl_beam_scores makes one read-back, bl_beam_reweigh_pf only the pose's. */
#define BL_BEAM_MAX_RAYS 4096
#define BL_BEAM_MAX_REACH 4096         /* cells: ceil(max_range * cells_per_meter) */
#define BL_BEAM_OFF_GRID INT64_MIN
typedef struct bl_beam_params_t {
    float max_range;                   /* metres, finite, > 0.15 */
    float sigma_cells;                 /* cells, > 0: the hit term's standard deviation */
    float z_hit, z_short, z_max, z_rand;   /* >= 0: the mixture's weights (they need not sum to 1) */
    float lambda;                      /* per cell, >= 0: the short term's decay */
    float blocked_factor;              /* >= 0: a max reading through a mapped wall is this much less likely than a free one */
    int32_t occ_min;                   /* 1 .. 127: a static cell is occupied when its log-odds is >= occ_min */
    int32_t hit_cut;                   /* 1 .. 1023 quarter cells: beyond it the hit term is Hit[hit_cut] */
    int32_t ray_stride;                /* 1 .. 64 */
    int32_t pad;
    int64_t span;                      /* 1 .. 2^40, Q16 nats: the score gap at which a particle reaches the floor */
} bl_beam_params_t;                    /* 56 bytes: offsets 0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44, 48 */
typedef struct bl_beam bl_beam;
int bl_beam_create(bl_ctx* ctx, bl_beam** out);                        /* buffers grow on demand */
void bl_beam_destroy(bl_beam* beam);
int bl_beam_set_params(bl_beam* beam, const bl_beam_params_t* params); /* refused: the handle keeps what it had */
/* the tables of the parameters in force for a map of cells_per_meter: hit[1024], short_[1024], lt[256] and scalars = Rand, MaxFree,
 * MaxBlocked, LN2, reach; any pointer may be NULL */
int bl_beam_tables(const bl_beam* beam, float cells_per_meter, uint32_t* hit, uint32_t* short_, uint32_t* lt, uint32_t scalars[5]);
void bl_beam_unit_table(uint32_t out[257]);                            /* host arithmetic only */
/* n host poses in, n scores out; any n >= 0 */
int bl_beam_scores(bl_beam* beam, const bl_grid* map, const bl_lidar_t* scan, const bl_pose_xyt_t* poses, int n, int64_t* out_scores);
/* The intermediate values of one pose's used rays, by the same kernel: bl_beam_last_rays() entries each (room for the scan's
 * num_ranges is always enough); any pointer may be NULL.  A ray dropped by `has`: first = K = z = z* = -1, p = 0; z = -1 for a max
 * reading; z* = -1 without an expected hit.  A pose that takes no part: zeros.  The units and the count that bl_beam_units reads are
 * left as they were; bl_beam_debug_path and bl_beam_last_device_ms speak of this launch afterwards. */
int bl_beam_debug_cast(bl_beam* beam, const bl_grid* map, const bl_lidar_t* scan, const bl_pose_xyt_t* pose, int32_t* out_first,
                       int32_t* out_K, int32_t* out_z, int32_t* out_zstar, uint32_t* out_p);
int bl_beam_reweigh_pf(bl_beam* beam, bl_pf* pf, const bl_grid* map, const bl_lidar_t* scan, bl_pose_xyt_t* out_pose);
/* the units of the last bl_beam_scores or bl_beam_reweigh_pf; n must be that call's count (the filter's active particles) */
int bl_beam_units(bl_beam* beam, uint32_t* out_units, int n);
int bl_beam_last_rays(const bl_beam* beam);                            /* used rays of the last scan taken; -1 before the first */
/* tests and probes: stage_windows 1 stages a workgroup's window in LDS when it fits (0, the default: the grid is read everywhere);
 * window_bytes 16 .. 40960 (0: the default, 40960) is what a staged window may take */
int bl_beam_debug_set(bl_beam* beam, int stage_windows, int window_bytes);
/* which path the workgroups of the last launch took: 0 staged, 1 direct, 2 some of each; -1 before the first (synchronises) */
int bl_beam_debug_path(bl_beam* beam);
/* device time of the last call's kernels (HIP events around the launches); BL_ERR_STATE before the first */
int bl_beam_last_device_ms(const bl_beam* beam, float* ms);

/* ------------------------------------------------------------------ range table (no reference counterpart)
 * On a map that does not change, the expected range of a ray depends only on its start cell and its direction.  The table holds it
 * for every cell and Hn headings, so that the beam model can look it up instead of walking the map (range_libc's LUT).  Off unless
 * called: bl_beam_scores, bl_beam_reweigh_pf and the filter's update are untouched.
 *   Handle.  bl_rangetable_create(ctx, headings, &rt): headings = Hn, a power of two in 64 .. 1024, else BL_ERR_ARG.
 *   Directions.  reach = ceil((double)max_range * cells_per_meter), as in bl_beam_tables.  For h = 0 .. Hn - 1
 *       D[h] = (lround(reach * cos(2 pi h / Hn)), lround(reach * sin(2 pi h / Hn))), made on the host in double, int32 pairs.
 *   Entries.  uint16, T[(y * W + x) * Hn + h].  The ray starts at cell s = (x, y) and ends at the far cell m = s + D[h]; the walk is
 *     the beam model's (start cell k = 0 included, far cell k = K excluded, K = Chebyshev(s, m)).  first = the least k whose cell lies
 *     inside the grid and has log-odds >= occ_min; the entry is q(c*, s) of that cell, the beam model's exact integer length in quarter
 *     cells, and BL_RANGETABLE_NONE when there is no such k.  An occupied start cell holds 0 in all Hn entries.  The largest real
 *     entry is 23 170 (reach <= 4096), so the sentinel cannot collide with a value.
 *   bl_rangetable_build(rt, beam, map) takes reach and occ_min from the beam model's parameters and the size, origin and
 *     cells_per_meter from the map, stores them in the handle and fills the whole table.  More than 2^31 entries (W * H * Hn) are
 *     refused with BL_ERR_ARG before anything is allocated, and the handle keeps the table it had.  A handle may be built again with
 *     other parameters or another map.
 *   bl_rangetable_update(rt, map, x0, y0, x1, y1) is called after the cells of the box x0 .. x1, y0 .. y1 (inclusive) changed: the
 *     entries of every cell of the box widened by reach on each side and clipped to the grid are computed again (a cell's entries
 *     depend on no cell farther away), by the same kernel.  The table then equals byte for byte what build gives on the new map.  A box
 *     with x1 < x0 or y1 < y0, or one that lies wholly outside the grid, changes nothing.  A map of another shape than the built one:
 *     BL_ERR_ARG, the table stays as it was.  Before the first build: BL_ERR_STATE.
 *   bl_rangetable_read(rt, x0, y0, w, h, out) downloads the entries of the cells x0 .. x0 + w - 1, y0 .. y0 + h - 1 (inside the
 *     grid, else BL_ERR_ARG) as out[((y - y0) * w + (x - x0)) * Hn + hd].  bl_rangetable_directions(rt, out): 2 * Hn int32 (x, y per
 *     heading) of the built table.  Both BL_ERR_STATE before the first build.  bl_rangetable_info works at any time.
 *   Scoring by table, bl_rangetable_scores(beam, rt, scan, poses, n, out_scores).  The used rays, the start cell s of a pose and the
 *     poses that take no part are exactly the beam model's, with the frame the table was built on.  Per used ray
 *       a = wrap_to_pi(theta - theta_r) in float32 (the angle of the beam model's geometry); a ray whose a is not finite is dropped;
 *       hd = (int)floorf(a * kf + 0.5f) & (Hn - 1), kf = (float)(Hn / (2 pi)): one multiply and one add, each rounded to float;
 *       z* = T[s, hd]: an expected hit unless it is BL_RANGETABLE_NONE;
 *       for a return z = (int)(range * q), q = 4.0f * cells_per_meter: no sine, no cosine, no end cell.
 *     The rest is the beam model's with the handle's own tables: Hit[min(|z - z*|, hit_cut)] with an expected hit, plus
 *     Short[min(z >> 2, 1023)] without one or when z < z*, plus Rand; MaxBlocked / MaxFree for a max reading; lg, the int64 sum, Smax,
 *     the units.  BL_ERR_STATE: the table is not built; the beam model's occ_min differs from the one the table was built with; the
 *     beam model's reach at the table's cells_per_meter differs from the built one.  THE TABLE IS NOT CHECKED AGAINST THE LIVE MAP:
 *     keeping it current is the caller's job (bl_rangetable_update).
 *   bl_rangetable_reweigh_pf(beam, pf, rt, scan, out_pose) is bl_beam_reweigh_pf with the table behind it: the same install of the
 *     units, the same state rules, the same behaviour under recovery; sharded filters are refused.  bl_rangetable_debug_lookup returns one
 *     pose's hd, z, z*, p per used ray (z = -1 for a max reading, z* = -1 without an expected hit, hd = z = z* = -1 and p = 0 for a
 *     dropped ray, zeros for a pose that takes no part), as bl_beam_debug_cast does for the cast.  bl_beam_units and
 *     bl_beam_last_device_ms work after either form; bl_beam_debug_path answers 1 after a scoring by table.
 *   How it is computed.  k_rt_build (bl_rangetable.hip): a wave per cell, a lane per heading in rounds of 64; the lane walks the
 *     Bresenham loop from s and stops at its first occupied cell or when it leaves the grid; an occupied start cell is settled without
 *     a walk; D[] in LDS; a cell's entries are stored as one row, 128 bytes per 64 lanes; the map bytes come from the grid through
 *     L2.  k_beam_lookup (bl_beam.hip): k_beam_cast's launch shape, the three score tables in LDS, a pose's rays read one row of
 *     2 * Hn bytes; k_beam_final and k_beam_units as they stand.  No atomics; no workgroup waits for another. */
#define BL_RANGETABLE_NONE 0xFFFF
typedef struct bl_rangetable bl_rangetable;
typedef struct bl_rangetable_info_t {
    int32_t width, height;             /* of the map built on; 0 before the first build */
    int32_t headings;
    int32_t reach, occ_min;            /* 0 before the first build */
    int32_t built;                     /* 0 or 1 */
    int64_t bytes;                     /* of the table on the device: 2 * width * height * headings */
} bl_rangetable_info_t;                /* 32 bytes: offsets 0, 4, 8, 12, 16, 20, 24 */
int bl_rangetable_create(bl_ctx* ctx, int headings, bl_rangetable** out);
void bl_rangetable_destroy(bl_rangetable* rt);
int bl_rangetable_build(bl_rangetable* rt, const bl_beam* beam, const bl_grid* map);
int bl_rangetable_update(bl_rangetable* rt, const bl_grid* map, int x0, int y0, int x1, int y1);
int bl_rangetable_read(bl_rangetable* rt, int x0, int y0, int w, int h, uint16_t* out);
int bl_rangetable_directions(const bl_rangetable* rt, int32_t* out);
int bl_rangetable_info(const bl_rangetable* rt, bl_rangetable_info_t* out);
/* device time of the last build's or update's kernel (HIP events around the launch); BL_ERR_STATE before the first */
int bl_rangetable_last_device_ms(const bl_rangetable* rt, float* ms);
/* The beam model scored through the table.  (Named after the handle they need beside the beam model: the bl_beam_ names are the
 * cast's.)  n host poses in, n scores out; any n >= 0 */
int bl_rangetable_scores(bl_beam* beam, const bl_rangetable* rt, const bl_lidar_t* scan, const bl_pose_xyt_t* poses, int n, int64_t* out_scores);
int bl_rangetable_reweigh_pf(bl_beam* beam, bl_pf* pf, const bl_rangetable* rt, const bl_lidar_t* scan, bl_pose_xyt_t* out_pose);
/* bl_beam_last_rays() entries each (room for the scan's num_ranges is always enough); any pointer may be NULL.  The units and the
 * count that bl_beam_units reads are left as they were. */
int bl_rangetable_debug_lookup(bl_beam* beam, const bl_rangetable* rt, const bl_lidar_t* scan, const bl_pose_xyt_t* pose, int32_t* out_h,
                               int32_t* out_z, int32_t* out_zstar, uint32_t* out_p);

/* ------------------------------------------------------------------ clearance grid (no reference counterpart)
 * The beam model's cast reads every cell of a ray's walk, and nearly all of them are empty.  The clearance grid holds, per cell, how
 * far the nearest occupied cell is, so that the walk can leap over the empty stretch: one byte per cell, redone in a box after a map
 * update, for maps that change (the range table is for maps that do not).  Off unless called: bl_beam_*, bl_rangetable_* and the
 * filter's update are untouched.
 *   Handle.  bl_clearance_create(ctx, cap, &cl): cap = C in 1 .. 255, else BL_ERR_ARG.  C IS AN UNTUNED KNOB.
 *   Entries.  uint8, D[y * W + x] = min(C, the least max(|x - ox|, |y - oy|) over the cells (ox, oy) inside the grid whose log-odds is
 *     >= occ_min): the Chebyshev distance to the nearest occupied cell, capped.  An occupied cell holds 0; a map without an occupied
 *     cell holds C everywhere; cells outside the grid are never occupied.
 *   bl_clearance_build(cl, map, occ_min) (occ_min in 1 .. 127, else BL_ERR_ARG) stores the map's size, origin and cells_per_meter and
 *     occ_min in the handle and fills the whole grid.  A handle may be built again on another shape or occ_min.  More than 2^30 cells
 *     are refused with BL_ERR_ARG before anything is allocated.
 *   bl_clearance_update(cl, map, x0, y0, x1, y1) is called after the cells of the box x0 .. x1, y0 .. y1 (inclusive) changed: every
 *     entry of the box widened by C on each side and clipped to the grid is computed again (an entry depends on no cell farther
 *     away), by the same kernels.  The grid then equals byte for byte what build gives on the new map.  A box with x1 < x0 or
 *     y1 < y0, or one that lies wholly outside the grid, changes nothing.  A map of another shape than the built one: BL_ERR_ARG,
 *     the grid stays as it was.  Before the first build: BL_ERR_STATE.
 *   bl_clearance_read(cl, x0, y0, w, h, out) downloads the entries of the cells x0 .. x0 + w - 1, y0 .. y0 + h - 1 (inside the
 *     grid, else BL_ERR_ARG) as out[(y - y0) * w + (x - x0)]; BL_ERR_STATE before the first build.  bl_clearance_info works at any
 *     time.  A NULL handle and a map of another ctx are BL_ERR_ARG.
 *   The leap walk.  Consecutive cells of the beam model's walk are Chebyshev neighbours, so from walk cell k with D = d > 0 the cells
 *     k + 1 .. k + d - 1 are not occupied and the walk may go on at cell k + d, whose place the walk's closed form gives (one 32-bit
 *     division).  From k = 0: a cell outside the grid ends the walk with first = K (a walk that has left never comes back); d = 0
 *     ends it with first = k; otherwise k += d; k >= K ends it with first = K.  first, K and the hit cell equal the cast's for
 *     every ray; `rounds` counts the entries read.
 *   Scoring by leaps, bl_clearance_scores(beam, cl, scan, poses, n, out_scores): bl_beam_scores in the frame the grid was built on,
 *     with the expected range found by the leap walk: the used rays, the geometry, the dropped rays, z, z*, p, lg, the int64 sum, Smax
 *     and the units equal the cast's value for value.  BL_ERR_STATE: the grid is not built; the beam model's occ_min differs from the
 *     one the grid was built with; before bl_beam_set_params.  THE GRID IS NOT CHECKED AGAINST THE LIVE MAP: keeping it current is
 *     the caller's job (bl_clearance_update).
 *   bl_clearance_reweigh_pf(beam, pf, cl, scan, out_pose) is bl_beam_reweigh_pf with the leaps behind it: the same install of the
 *     units, the same state rules, the same behaviour under recovery; sharded filters are refused.  bl_clearance_debug_cast returns
 *     bl_beam_debug_cast's five columns with its conventions and the rounds (-1 for a dropped ray, 0 for a pose that takes no
 *     part).  bl_beam_units, bl_beam_last_rays and bl_beam_last_device_ms work after this form too; bl_beam_debug_path answers 1.
 *   How it is computed (bl_clearance.hip), two passes.  k_clr_rows: a wave per 64 cells of a row; the occupancy of these and of as
 *     many neighbouring 64-cell words as C reaches, each as one ballot; a lane's distance along the row to the nearest set bit by
 *     count-trailing and count-leading zeros, capped, a uint8 of the intermediate.  k_clr_cols: a thread per cell, threads along x;
 *     D = min over dy of max(|dy|, row[y + dy]) taken outward from dy = 0 and stopped when |dy| reaches the best so far.
 *     k_beam_leap (bl_beam.hip): k_beam_cast's launch shape and frame, D read through L2.  No atomics; no workgroup waits for
 *     another; no result depends on the launch shape.  The intermediate takes as many bytes on the device as the grid. */
typedef struct bl_clearance bl_clearance;
typedef struct bl_clearance_info_t {
    int32_t width, height;             /* of the map built on; 0 before the first build */
    int32_t cap;
    int32_t occ_min;                   /* 0 before the first build */
    int32_t built;                     /* 0 or 1 */
    int32_t pad;
    int64_t bytes;                     /* of the grid on the device: width * height */
} bl_clearance_info_t;                 /* 32 bytes: offsets 0, 4, 8, 12, 16, 20, 24 */
int bl_clearance_create(bl_ctx* ctx, int cap, bl_clearance** out);
void bl_clearance_destroy(bl_clearance* cl);
int bl_clearance_build(bl_clearance* cl, const bl_grid* map, int occ_min);
int bl_clearance_update(bl_clearance* cl, const bl_grid* map, int x0, int y0, int x1, int y1);
int bl_clearance_read(bl_clearance* cl, int x0, int y0, int w, int h, uint8_t* out);
int bl_clearance_info(const bl_clearance* cl, bl_clearance_info_t* out);
/* device time of the last build's or update's kernels (HIP events around the launches); BL_ERR_STATE before the first */
int bl_clearance_last_device_ms(const bl_clearance* cl, float* ms);
/* The beam model scored by leaps.  (Named after the handle they need beside the beam model: the bl_beam_ names are the cast's.)
 * n host poses in, n scores out; any n >= 0 */
int bl_clearance_scores(bl_beam* beam, const bl_clearance* cl, const bl_lidar_t* scan, const bl_pose_xyt_t* poses, int n, int64_t* out_scores);
int bl_clearance_reweigh_pf(bl_beam* beam, bl_pf* pf, const bl_clearance* cl, const bl_lidar_t* scan, bl_pose_xyt_t* out_pose);
/* bl_beam_last_rays() entries each (room for the scan's num_ranges is always enough); any pointer may be NULL.  The units and the
 * count that bl_beam_units reads are left as they were. */
int bl_clearance_debug_cast(bl_beam* beam, const bl_clearance* cl, const bl_lidar_t* scan, const bl_pose_xyt_t* pose, int32_t* out_first,
                            int32_t* out_K, int32_t* out_z, int32_t* out_zstar, uint32_t* out_p, int32_t* out_rounds);

/* ------------------------------------------------------------------ scan history and map rebuild  
 * A map is otherwise written once, at the pose held at that moment, and the scan is thrown away.  The log keeps the last
 * `capacity_scans` scans on the device -- per scan the KEPT rays exactly as the mapper takes them (ranges, thetas, times; ranges
 * <= 0.15 already dropped), the kept count and the pose (utime, x, y, theta) -- so that a map can be made again from any window of
 * them, at any poses, in any grid.  Index 0 is the oldest retained scan.  All calls are stream-ordered on the ctx stream.
 *
 * bl_scanlog_rebuild(log, first, count, poses, prev_pose, max_laser, hit, miss, base, out).  The whole contract:
 *   - Start from `base`'s cells.  `base` must have the same shape and frame as `out`, and may be `out` itself.  NULL means all zero.
 *   - Take a fresh Mapping(max_laser, hit, miss).
 *   - If `prev_pose` is given, the mapper is primed with it: initialized_ true, previousPose_ = *prev_pose.
 *   - If `prev_pose` is NULL, scan `first` only latches its pose and changes no cell, as the first call of any Mapping does.
 *   - Then updateMap(scan_k, pose_k, out) runs for k = first ... first + count - 1, in order.  pose_k is poses[k - first], or the
 *     recorded pose when `poses` is NULL.
 *   - `out` equals the result byte for byte.
 *   Every rule of the map update's geometry holds: the range <= max_laser cut; per-ray pose interpolation between pose k-1 and
 *   pose k by ray time; no interpolation when the two utimes are equal; float -> int truncation; the 2^24 coordinate limit; the end
 *   cell gets the hit and is excluded from the walk; the start cell is included in the walk; off-grid cells are skipped; hits come
 *   before misses within a scan.  The geometry uses `out`'s frame, so a rebuild into a grid of another resolution or origin is the
 *   same call.  `out` is treated afterwards as bl_grid_upload treats its target (its mirror is stale, its cells start a new
 *   lineage).  A live bl_mapping object is neither read nor changed.  The call makes one small read-back (it synchronises).
 * Appending to a full ring drops the oldest scan.  A scan with more kept rays than max_rays_per_scan is refused and the log stays
 * as it was.  The second append form reads x, y, theta from device memory, stream-ordered, with no host round trip; utime comes
 * from the argument, as in bl_mapping_update_dev_pose.  bl_scanlog_set_poses overwrites recorded poses (a caller that corrected a
 * trajectory keeps it); bl_scanlog_get_poses, bl_scanlog_get_scan synchronise.
 * BL_ERR_ARG: capacity_scans < 1, max_rays_per_scan outside 1 .. 8192, more than 1 GiB of log (16 bytes a ray); a window outside
 * 0 .. size or count < 1; negative odds; a grid of another ctx; a base of another shape or frame.  A refused call enqueues nothing
 * and leaves `out` and the log untouched.  bl_scanlog_last_stats before the first rebuild: BL_ERR_STATE. */
typedef struct bl_scanlog bl_scanlog;
typedef struct bl_scanlog_stats_t {
    int64_t tiles;                     /* tiles of `out` (tile_cells x tile_cells cells each) */
    int64_t chunks;                    /* chunks of chunk_scans consecutive scans */
    int64_t pairs;                     /* (tile, chunk) pairs whose boxes meet: workgroups of the fold */
    int64_t scratch_bytes;             /* composed functions held between fold and apply: pairs * tile_cells^2 * 4 */
    int32_t chunk_scans, tile_cells;
    int32_t scans;                     /* scans that change cells: count, less the latching one without a prev_pose */
    int32_t pad;
    float ms_total, ms_geometry, ms_fold, ms_apply;   /* device time between events; geometry includes the read-back */
} bl_scanlog_stats_t;                  /* 64 bytes */
int bl_scanlog_create(bl_ctx* ctx, int capacity_scans, int max_rays_per_scan, bl_scanlog** out);
void bl_scanlog_destroy(bl_scanlog* log);
int bl_scanlog_append(bl_scanlog* log, const bl_lidar_t* scan, const bl_pose_xyt_t* pose);
int bl_scanlog_append_dev_pose(bl_scanlog* log, const bl_lidar_t* scan, const void* d_pose /* bl_pose_xyt_t* */, int64_t pose_utime);
int bl_scanlog_size(const bl_scanlog* log);                             /* scans held; 0 for NULL */
int bl_scanlog_get_poses(bl_scanlog* log, int first, int count, bl_pose_xyt_t* out);
int bl_scanlog_set_poses(bl_scanlog* log, int first, int count, const bl_pose_xyt_t* poses);
/* the kept rays of entry i (room for max_rays_per_scan each; any pointer may be NULL) */
int bl_scanlog_get_scan(bl_scanlog* log, int i, float* ranges, float* thetas, int64_t* times, int* kept);
int bl_scanlog_rebuild(bl_scanlog* log, int first, int count, const bl_pose_xyt_t* poses /* NULL: recorded */,
                       const bl_pose_xyt_t* prev_pose /* may be NULL */, float max_laser, int8_t hit, int8_t miss,
                       const bl_grid* base /* may be NULL */, bl_grid* out);
int bl_scanlog_last_stats(bl_scanlog* log, bl_scanlog_stats_t* stats);  /* of the last rebuild; waits for it */

/* ------------------------------------------------------------------ pose graph  
 * The solver that turns "scan 900 saw the place scan 40 saw" into moved poses: what computes the corrected poses that the scan
 * history rebuilds a map at.
 *
 * Problem.  Nodes x_k = (x, y, theta), 2 <= N <= 4096, theta within [-pi, pi].  An edge (i, j, z, info) says that pose j seen from
 *   pose i is z; info holds xx, xy, yy, xt, yt, tt of a symmetric positive semi-definite 3 x 3 matrix Omega, in the order of the scan
 *   matcher's covariance.  The cost is F = sum over the edges of e' Omega e,
 *     e = ( R(theta_i)' (t_j - t_i) - z_xy , wrap(theta_j - theta_i - z_theta) ).
 *   The first N - 1 edges are the chain (k, k + 1), in order: the odometry, which keeps the system connected.  Up to 1024 loop edges
 *   follow, between any i != j; repeated pairs are allowed; a loop edge whose six information values are all zero behaves as an absent
 *   one.  One node, params.fixed, is held.
 * Method.  Gauss-Newton with Levenberg-Marquardt step control: H = sum J' Omega J + lambda I, H dx = -sum J' Omega e.  A try is accepted
 *   only if F falls (then lambda *= lambda_down); otherwise lambda *= lambda_up and the try is repeated.  The solve stops at an
 *   accepted step with max |dx| <= step_tol (status CONVERGED_STEP; a zero gradient counts as such a step and is not "accepted"), at
 *   an accepted step with F_old - F_new <= rel_tol F_old (CONVERGED_DECREASE), or after max_tries tries (OUT_OF_TRIES).  The linear
 *   step is conjugate gradients preconditioned by the block-tridiagonal part of H, which block cyclic reduction factors once per try;
 *   it stops when r' T^-1 r <= cg_tol^2 times its first value, or after max_cg iterations (or when p' H p is not positive), and then
 *   the status carries the flag CG_CAP and the step so far is tried.
 * Arithmetic.  All state is double; every operation is one of + - * / rounded by itself; every sum has one order.
 *   Sine and cosine of a heading are those of the heading narrowed to float, widened to double.  wrap is one comparison and one
 *   +- 2 pi.  Results do not depend on the number of subsets, on their order or on any launch parameter.
 * Subsets.  solve takes n_subsets bit masks over the loop edges, (L + 31) / 32 uint32 words each, bit l of a mask: loop edge l is in
 *   force.  NULL means one subset with every edge on (n_subsets must be 1).  One workgroup solves one subset from start to finish,
 *   all of them side by side in one launch.  A loop edge alone with the chain has as its optimal cost its Mahalanobis distance under
 *   the accumulated odometry, so L + 1 subsets test every candidate at once.
 * Calls.  set_nodes and set_nodes_from_log (device to device, entries first .. first + count - 1 of a log of the same ctx) replace the
 *   nodes, and drop the chain and the loop edges.  set_chain takes N - 1 edges with i = k, j = k + 1; set_chain_from_nodes makes them
 *   on the device, z_k the relative pose of the nodes k, k + 1 by the residual's own statements, so that with no loop edge the start
 *   cost is exactly 0.  set_loops replaces the loop edges (n = 0: none).  solve is enqueued on the ctx stream and does not wait.
 *   results, poses (x, y, theta in double, 3 a node, and/or narrowed once to float with the node's utime), edge_chi2 (N - 1 + L values
 *   of e' Omega e at the start and at the end, edges out of force included) and last_device_ms wait for it.  poses_to_log writes a
 *   subset's narrowed poses over the recorded poses of entries first .. first + N - 1, device to device, stream-ordered.
 * BL_ERR_ARG: max_nodes outside 2 .. 4096, max_loop_edges outside 0 .. 1024, max_subsets < 1, more than 1 GiB in all; n outside
 *   2 .. max_nodes; a chain edge that is not (k, k + 1); a loop edge with i = j or a node outside 0 .. N - 1; a z or info that is not
 *   finite; n_subsets outside 1 .. max_subsets; fixed outside 0 .. N - 1; max_tries < 1; max_cg < 1; lambda0 < 0; lambda_up <= 1;
 *   lambda_down outside (0, 1]; a negative or non-finite tolerance; a subset outside the last solve's; a log of another ctx or a
 *   window outside it.  BL_ERR_STATE: chain or loops before nodes, solve before nodes and chain, a reader before the first solve.
 *   A refused call enqueues nothing and changes nothing. */
typedef struct bl_posegraph bl_posegraph;
typedef struct bl_posegraph_edge_t {
    int32_t i, j;
    double z[3];                       /* x, y, theta of pose j in the frame of pose i */
    double info[6];                    /* xx, xy, yy, xt, yt, tt */
} bl_posegraph_edge_t;                 /* 80 bytes */
typedef struct bl_posegraph_params_t {
    int32_t fixed, max_tries, max_cg, pad;
    double lambda0, lambda_up, lambda_down;
    double step_tol, rel_tol, cg_tol;
} bl_posegraph_params_t;               /* 64 bytes */
#define BL_POSEGRAPH_CONVERGED_STEP 1
#define BL_POSEGRAPH_CONVERGED_DECREASE 2
#define BL_POSEGRAPH_OUT_OF_TRIES 3
#define BL_POSEGRAPH_CG_CAP 16         /* flag, or-ed in: some try's conjugate gradients ended before their tolerance */
typedef struct bl_posegraph_result_t {
    double cost_before, cost_after;    /* F over the edges in force, at the nodes and at the result */
    double final_lambda;
    int32_t tries, accepted;
    int32_t cg_iterations;             /* over all tries */
    int32_t status;
} bl_posegraph_result_t;               /* 40 bytes */
int bl_posegraph_create(bl_ctx* ctx, int max_nodes, int max_loop_edges, int max_subsets, bl_posegraph** out);
void bl_posegraph_destroy(bl_posegraph* pg);
int bl_posegraph_set_nodes(bl_posegraph* pg, int n, const bl_pose_xyt_t* poses);
int bl_posegraph_set_nodes_from_log(bl_posegraph* pg, bl_scanlog* log, int first, int count);
int bl_posegraph_set_chain(bl_posegraph* pg, const bl_posegraph_edge_t* edges /* N - 1 */);
int bl_posegraph_set_chain_from_nodes(bl_posegraph* pg, const double* info6);
int bl_posegraph_set_loops(bl_posegraph* pg, int n, const bl_posegraph_edge_t* edges);
int bl_posegraph_solve(bl_posegraph* pg, const bl_posegraph_params_t* params, int n_subsets, const uint32_t* masks /* may be NULL */);
int bl_posegraph_results(bl_posegraph* pg, bl_posegraph_result_t* results /* n_subsets of the last solve */);
int bl_posegraph_poses(bl_posegraph* pg, int subset, bl_pose_xyt_t* out_xyt /* may be NULL */, double* out_double /* may be NULL */);
int bl_posegraph_edge_chi2(bl_posegraph* pg, int subset, double* before /* may be NULL */, double* after /* may be NULL */);
int bl_posegraph_poses_to_log(bl_posegraph* pg, int subset, bl_scanlog* log, int first);
int bl_posegraph_last_device_ms(bl_posegraph* pg, float* ms);

/* ------------------------------------------------------------------ loop closure  
 * The front end of the pose graph: from a scan log, the loop edges.  Every candidate pair is chosen, every submap rebuilt, every scan
 * matched against its submap straight from the log and every edge formed in one sequence of launches whose length does not depend on
 * the number of candidates.  The numpy restatement is tests/loop_closure_model.py.
 *
 * Inputs: a bl_scanlog with n entries; a grid `like`, of which only the two resolution floats mpc and cpm are read; the parameters
 *   stride >= 1, min_gap >= 0, radius (float, > 0), w, 0 .. 31, submap_cells S, 16 .. 512, max_laser, hit, miss, a
 *   bl_scan_match_params_t (its keep_volume must be 0) and a bl_scan_match_prior_t (its want_moments is taken as set; half_life is
 *   checked as bl_scanmatch_match_prior checks it).
 * Pairs.  For q = 0, stride, 2 stride, ... < n, let last = q - min_gap - 1.  If last < 0 there is no candidate.
 *   d2(j) = (x_j - x_q)^2 + (y_j - y_q)^2 over j = 0 .. last.  The recorded float poses are widened to double and every operation is
 *   rounded by itself.  j is the lowest index of the minimum.  There is no candidate if d2(j) > (double)radius * (double)radius.
 *   Candidates are numbered in ascending q; m = 0 .. M - 1.
 * Submap m.  Its window is first = max(j - w, 0) to end = min(j + w, n - 1).  The grid is S x S with like's mpc and cpm.  Its origin
 *   is ((float)x_j - half, (float)y_j - half) with half = (float)((double)S * (double)mpc / 2.0).  Both subtractions are in float.
 *   Its cells are, byte for byte, what bl_scanlog_rebuild(log, first, end - first + 1, NULL, NULL, max_laser, hit, miss, NULL, sub)
 *   leaves.  So the window's first scan only latches its pose.  Every later one is traced from its predecessor's pose with the
 *   per-ray time interpolation of the map update.
 * Match m.  bl_scanmatch_match_prior's definition word for word.  The scan is the kept rays of entry q as they lie in the log,
 *   filtered by the matcher's rule (range > 0.15f and range < max_range).  The centre is entry q's recorded pose; utime is that
 *   pose's.  The map is submap m.  The caller's params and prior apply.  The result is a bl_scan_match_result_t and a
 *   bl_scan_match_moments_t.  These equal, byte for byte, what the existing call returns for the same inputs.  A scan with more than
 *   4096 valid rays is not matched: it carries the flag BL_LC_TOO_MANY_RAYS, and its result and moments are all zero.
 * Gate.  A candidate is kept when all of these hold: accepted, ties == 1, |di| < nx, |dj| < ny, |dk| < ntheta.  Otherwise the flag
 *   word says which failed: BL_LC_NOT_ACCEPTED, BL_LC_TIED, BL_LC_ON_EDGE.
 * Edge of a kept candidate (i = j, j = q).  All arithmetic is plain double: each + - * / is rounded by itself and no operation is
 *   fused.
 *     p = bl_scanmatch_refined_pose(result, moments, centre, mpc, dtheta).
 *     Sigma = bl_scanmatch_covariance(moments, mpc, dtheta).  Both are the helpers above, called as they are.
 *     c and s are the cosine and sine of theta_j, formed as the pose graph forms them for a node: those of the float heading, widened.
 *     dx = p.x - x_j, dy = p.y - y_j.
 *     z = (c dx + s dy, c dy - s dx, wrap(p.theta - theta_j)), with the pose graph's wrap (one comparison, one +- 2 pi).
 *     S = R' Sigma R + diag(mpc^2 / 12, mpc^2 / 12, dtheta^2 / 12), R' = ((c, s, 0), (-s, c, 0), (0, 0, 1)).  The two products are
 *       taken left to right.  Every entry is (a0 b0 + a1 b1) + a2 b2.
 *     info is the inverse of S by cofactors, each divided by the determinant (S00 C00 + S01 C01) + S02 C02, and symmetrised as
 *       0.5 (I_ab + I_ba).  Its order is xx, xy, yy, xt, yt, tt.
 *   A candidate that is not kept has an all-zero edge.
 * Calls.  find is enqueued on the ctx stream and synchronises once to hand back M.  candidates returns the M records of the last
 *   find, edges the kept candidates' edges in ascending q, ready for bl_posegraph_set_loops.  submap is diagnostic: submap m's S * S
 *   bytes and its origin (either pointer may be NULL).  A log with fewer than two entries gives M = 0 and BL_OK.
 * BL_ERR_ARG: a null pointer; max_candidates outside 1 .. 1024; a parameter outside the limits above; negative odds or odds above 127;
 *   keep_volume != 0; a half life outside 1 .. 2^20; a window or a prior the matcher would refuse; a log of another ctx; radius not
 *   positive or NaN; scratch (submaps, objective volumes, ray cells, endpoints) above 1 GiB; more queries with a partner than
 *   max_candidates; m outside 0 .. M - 1.  Every refusal leaves the last results readable and unchanged; all but the count of partners
 *   are found before any launch. */
#define BL_LC_NOT_ACCEPTED 1
#define BL_LC_TIED 2
#define BL_LC_ON_EDGE 4
#define BL_LC_TOO_MANY_RAYS 8
#define BL_LC_MAX_CANDIDATES 1024
#define BL_LC_MAX_W 31
#define BL_LC_MIN_SUBMAP 16
#define BL_LC_MAX_SUBMAP 512
typedef struct bl_loopclose_params_t {
    int32_t stride, min_gap;
    float radius;
    int32_t w, submap_cells;
    float max_laser;
    int32_t hit, miss;
    bl_scan_match_params_t match;
    bl_scan_match_prior_t prior;
} bl_loopclose_params_t;               /* 84 bytes: offsets 0, 4, 8, 12, 16, 20, 24, 28, 32, 60 */
typedef struct bl_loopclose_candidate_t {
    int32_t q, j;                      /* the query scan and its partner */
    int32_t first, count;              /* the submap's window of the log */
    uint32_t flags;                    /* BL_LC_*; 0: kept */
    int32_t pad;
    bl_scan_match_result_t result;
    bl_scan_match_moments_t moments;
    bl_posegraph_edge_t edge;          /* i = j, j = q; all zero unless kept */
} bl_loopclose_candidate_t;            /* 272 bytes: offsets 0, 4, 8, 12, 16, 20, 24, 80, 192 */
typedef struct bl_loopclose bl_loopclose;
int bl_loopclose_create(bl_ctx* ctx, int max_candidates, bl_loopclose** out);
void bl_loopclose_destroy(bl_loopclose* lc);
int bl_loopclose_find(bl_loopclose* lc, bl_scanlog* log, const bl_grid* like, const bl_loopclose_params_t* params, int* n_candidates);
int bl_loopclose_candidates(bl_loopclose* lc, bl_loopclose_candidate_t* out /* M of the last find */);
int bl_loopclose_edges(bl_loopclose* lc, int* n, bl_posegraph_edge_t* out /* may be NULL: only the count; room for M */);
int bl_loopclose_submap(bl_loopclose* lc, int m, int8_t* cells /* S * S */, float* origin_xy /* 2 */);
/* device time of the last find between events: total, and pairs / rays + fold / match / records (ms4 may be NULL); BL_ERR_STATE
 * before the first find that launched */
int bl_loopclose_last_device_ms(bl_loopclose* lc, float* ms, float* ms4);

/* ------------------------------------------------------------------ loop closure by place recognition  
 * The pair rule above finds a partner only while the drift of the recorded poses is smaller than `radius`.  find_places chooses the
 * partner by what the scans look like instead: every logged scan gets a descriptor, a query's partner is the older scan whose
 * descriptor it resembles most at the best circular shift, and the match is centred on the partner's pose turned by that shift.
 * Everything is integer work on the bits of the logged floats; the numpy restatement is tests/place_model.py.
 *
 * Constants.  BL_PLACE_SECTORS = 64, BL_PLACE_BINS = 32, K = 10.185916f (the float nearest 32 / pi), STEP = 0.09817477f (the float
 *   nearest 2 pi / 64).
 * Parameters (bl_place_params_t).  bins_per_meter in (0, 1000]; max_range in (0.15, 1000]; dilate 0 or 1; min_key 0 .. 65536;
 *   min_bits 0 .. 2048.  bins_per_meter, dilate, min_key and min_bits are untuned knobs.
 * Descriptor of entry e: 64 words of 32 bits, all zero at first.  Ray r counts for every r < min(kept, max_rays) when the matcher's
 *   own rule holds (range > 0.15f and range < max_range, with this struct's max_range) and fabsf(theta) <= 1024.0f (false for NaN).
 *   Sector a = (int)floorf(theta * K) & 63, one float multiply.  Bin b = min((int)(range * bins_per_meter), 31), one float multiply,
 *   truncated.  Bit b of word a is set.  bits[e] is the number of set bits.  The rays' times and the robot's motion during the scan
 *   are ignored: the descriptor is that of the scan as it lies in the log.
 * Query side.  D'q[a] = Dq[a] when dilate == 0, else Dq[a] | Dq[a] << 1 | Dq[a] >> 1 in uint32 (bits fall off both ends);
 *   bits'q is the number of set bits of D'q.
 * Score of (q, j, s), s = 0 .. 63.  ov = sum over a of popcount(D'q[(a + s) & 63] & Dj[a]); den = bits'q + bits[j] - ov;
 *   key = den == 0 ? 0 : (ov * 65536) / den in unsigned integers (ov <= 2048).
 * Best.  Queries are q = 0, stride, 2 stride, ... < n with last = q - min_gap - 1, as the pair search counts them.  j is eligible when
 *   0 <= j <= last and bits[j] >= min_bits.  If bits[q] < min_bits or no j is eligible the query has no best: j = -1, partner = -1,
 *   every other field but q and bits_q is 0.  Otherwise the best is the greatest key over the eligible j and all s; among equal keys
 *   the lowest j wins, then the lowest s.  partner = j when key >= min_key, else -1; the best is recorded either way.
 * Candidates.  The queries with a partner, numbered in ascending q.  first, count, origin and submap are those of the section above.
 *   The centre of the match is (x_j, y_j, theta_c, utime_q) with theta_c = theta_j + (float)ss * STEP, ss = s < 32 ? s : s - 64; the
 *   product and the sum are each rounded to float by itself, there is no fused operation and no wrap.  Match, gate, flags, record and
 *   edge are the section above's word for word with this centre where the recorded pose of q stood.  params.radius is not read.
 * Sign.  Ray i of a scan is cast at pose.theta - scan.theta, so two scans from one spot with headings theta_q and theta_j line up at
 *   s near (theta_q - theta_j) * 64 / (2 pi), modulo 64.
 * Calls.  find_places runs as find does and refuses what find refuses, the radius test left out and the limits above added; every
 *   refusal leaves the last results readable and unchanged.  places returns the per-query records, descriptors the n x 64 words and
 *   the n counts (either pointer may be NULL; n itself is handed back), both of the last find_places that launched; BL_ERR_STATE before one.  A plain find
 *   leaves them as they were.  The first slot of last_device_ms's split then holds descriptors + best pairs. */
#define BL_PLACE_SECTORS 64
#define BL_PLACE_BINS 32
typedef struct bl_place_params_t {
    float bins_per_meter, max_range;
    int32_t dilate, min_key, min_bits;
} bl_place_params_t;                   /* 20 bytes: offsets 0, 4, 8, 12, 16 */
typedef struct bl_place_t {
    int32_t q, j, shift, key, overlap, bits_q, bits_j, partner;
} bl_place_t;                          /* 32 bytes: offsets 0, 4, 8, 12, 16, 20, 24, 28 */
int bl_loopclose_find_places(bl_loopclose* lc, bl_scanlog* log, const bl_grid* like, const bl_loopclose_params_t* params,
                             const bl_place_params_t* place, int* n_candidates);
int bl_loopclose_places(bl_loopclose* lc, int* n_queries, bl_place_t* out /* may be NULL: only the count */);
int bl_loopclose_descriptors(bl_loopclose* lc, int* n, uint32_t* words /* n * 64, may be NULL */, int32_t* bits /* n, may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* BOTLAB_HIP_H */
