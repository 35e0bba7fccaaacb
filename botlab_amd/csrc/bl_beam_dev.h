// bl_beam_dev.h -- the rules of the beam model (include/botlab_hip.h, "beam model" and "range table"), each stated once: a pose's
// start cell, the first-hit walk, the tables' places, the length in quarter cells, a return's probability, the integer logarithm,
// the look-up's heading index and the reach in cells.  k_beam_cast and k_beam_lookup (bl_beam.hip) score with them and k_rt_build
// (bl_rangetable.hip) fills its entries with the same walk and length, so a table entry equals the cast's z* by construction.
// k_beam_leap (bl_beam.hip) takes the same walk in leaps over a clearance grid (beam_first_hit_leap).
//   host and device  everything but beam_reach
//   host             beam_reach, with the library's error text
// What differs stays with its kernel: where a cell is read from (the grid through L2 or a staged window), what leaving the grid
// means to the walk, and the launch shapes.  tests/cpp/beam_dev_ref.cpp compiles the first part for the host
// (tests/test_beam_dev_header_cpu.py).
#ifndef BL_BEAM_DEV_H
#define BL_BEAM_DEV_H

#if defined(__HIPCC__)
#include <math.h>

#include "bl_internal.h"
#else
#include <stdlib.h>

#include "../../include/botlab_hip.h"
#include "bl_math.h"
struct float4 { float x, y, z, w; };
inline int min(int a, int b) { return a < b ? a : b; }
inline int max(int a, int b) { return a > b ? a : b; }
#endif
#include "bl_mapray_dev.h"

#define BEAM_HIT 0                        // the tables' places in the block of BEAM_TABLE_WORDS words
#define BEAM_SHORT 1024
#define BEAM_LT 2048
#define BEAM_TABLE_WORDS 2304

// the start cell of a pose; false for a pose that takes no part
BL_HD bool beam_start(const float4& p, const bl_frame& f, float* px, float* py, int* sx, int* sy)
{
    if (!(__builtin_fabsf(p.x) < __builtin_inff() && __builtin_fabsf(p.y) < __builtin_inff() && __builtin_fabsf(p.z) < __builtin_inff())) return false;
    bl_global_to_grid(p.x, p.y, f, px, py);
    if (!(__builtin_fabsf(*px) < 0x1p30f && __builtin_fabsf(*py) < 0x1p30f)) return false;
    *sx = (int)*px; *sy = (int)*py;
    return *sx >= 0 && *sx < f.width && *sy >= 0 && *sy < f.height;
}

// The first-hit walk: the reference's Bresenham loop (mapping.cpp:101-127) from (sx, sy) towards (tx, ty), start cell included, end
// cell excluded, K = max(|tx - sx|, |ty - sy|) cells, as far as the first cell for which occupied(x, y) holds: cell `first` of the
// walk, at (x, y).  first = K when there is none, and x, y then say nothing.  occupied carries the kernel's read (the grid through
// L2 or a staged window); no cell outside the grid is occupied.  x and y each move one way only, so a walk that has left the grid
// never comes back: for a start cell inside it, ending the walk at the first cell for which left(x, y) holds (k_rt_build: the cell
// lies outside the grid, and occupied is not asked about it) and walking on to the end cell (beam_ray: no `left`, occupied answers
// false outside) give the same first, K and hit cell.
struct beam_hit { int first, K, x, y; };
struct beam_walk_on { BL_HD bool operator()(int, int) const { return false; } };
template <class Occupied, class Left = beam_walk_on>
BL_HD beam_hit beam_first_hit(int sx, int sy, int tx, int ty, Occupied occupied, Left left = Left())
{
    const int dx = abs(tx - sx), dy = abs(ty - sy);
    const int stepx = sx < tx ? 1 : -1, stepy = sy < ty ? 1 : -1;
    const int K = max(dx, dy);
    int err = dx - dy, x = sx, y = sy, k = 0;
    for (; k < K; ++k) {
        if (left(x, y)) { k = K; break; }
        if (occupied(x, y)) break;
        const int e2 = 2 * err;
        if (e2 >= -dy) { err -= dy; x += stepx; }
        if (e2 <= dx) { err += dx; y += stepy; }
    }
    const beam_hit h = {k, K, x, y};
    return h;
}

// The same walk in leaps ("clearance grid" in the header): clearance(x, y) of a cell inside the grid is a lower bound, 0 only for an
// occupied cell, on the Chebyshev distance to the nearest occupied cell.  Consecutive cells of the walk are Chebyshev neighbours, so
// from cell k with clearance d > 0 the cells k + 1 .. k + d - 1 are free and the walk goes on at cell k + d, placed by the closed form
// of bl_mapray_dev.h: one division (K <= BL_BEAM_MAX_REACH + 1, so bl_walk_begin takes its 32-bit branch).  left(x, y): the cell lies
// outside the grid, which ends the walk as it ends k_rt_build's; clearance is not asked about it.  first, K and the hit cell are
// beam_first_hit's; rounds counts the calls of clearance.
struct beam_leap_hit { int first, K, x, y, rounds; };
template <class Clearance, class Left>
BL_HD beam_leap_hit beam_first_hit_leap(int sx, int sy, int tx, int ty, Clearance clearance, Left left)
{
    const int4 ray = make_int4(sx, sy, tx, ty);
    const int K = bl_ray_steps(ray);
    int k = 0, rounds = 0, x = sx, y = sy;
    while (k < K) {
        bl_walk_cell(ray, k, &x, &y);
        if (left(x, y)) { k = K; break; }
        ++rounds;
        const int d = clearance(x, y);
        if (d == 0) break;
        k += d;
    }
    const beam_leap_hit h = {k < K ? k : K, K, x, y, rounds};
    return h;
}

BL_HD int beam_quarter(int ax, int ay, int bx, int by)
{
    const int dx = ax - bx, dy = ay - by;
    const uint32_t v = 16u * (uint32_t)(dx * dx + dy * dy);            // below 2^31: the cells lie within reach + 2 <= 4098 of each other
    uint32_t r = (uint32_t)__builtin_sqrtf((float)v);
    while (r * r > v) --r;
    while ((r + 1u) * (r + 1u) <= v) ++r;
    return (int)r;
}

// p of a return of z quarter cells; zstar: the expected hit's, read only with `expect`
BL_HD uint32_t beam_return_p(const uint32_t* s_tab, uint32_t rnd, int hit_cut, bool expect, int z, int zstar)
{
    uint32_t p = rnd;
    if (expect) p += s_tab[BEAM_HIT + min(abs(z - zstar), hit_cut)];
    if (!expect || z < zstar) p += s_tab[BEAM_SHORT + min(z >> 2, 1023)];
    return p;
}

BL_HD int beam_lg(const uint32_t* s_tab, uint32_t p, int ln2)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const int e = 31 - __clz((int)p);                                   // p >= 1: bl_beam_set_params
#else
    const int e = 31 - __builtin_clz(p);
#endif
    const uint32_t mant = ((p << (31 - e)) >> 23) & 255u;
    return (e - 30) * ln2 + (int)s_tab[BEAM_LT + mant];
}

// the heading a look-up reads for a ray at the finite angle ang: Hn a power of two, kf = (float)(Hn / (2 pi))
BL_HD int beam_heading_index(float ang, float kf, int Hn) { return (int)__builtin_floorf(ang * kf + 0.5f) & (Hn - 1); }

#if defined(__HIPCC__)
// the reach in cells of a maximum range on a map of cpm cells per metre: ceil(max_range * cpm), 1 .. BL_BEAM_MAX_REACH
static inline int beam_reach(float max_range, float cpm, int* reach)
{
    const double r = ceil((double)max_range * (double)cpm);
    BL_CHECK_ARG(r >= 1.0 && r <= (double)BL_BEAM_MAX_REACH);           // (false for NaN too)
    *reach = (int)r;
    return BL_OK;
}
#endif

#endif
