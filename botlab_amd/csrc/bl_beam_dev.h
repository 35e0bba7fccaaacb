// bl_beam_dev.h -- the rules of the beam model (include/botlab_hip.h, "beam model") that more than one kernel needs, stated once: the
// tables' places, the length in quarter cells, a return's probability and the integer logarithm.  k_beam_lookup (bl_beam.hip) scores
// with them and k_rt_build (bl_rangetable.hip) measures its entries with beam_quarter.  k_beam_cast takes the places and beam_quarter
// from here but carries the probability and the logarithm written out in beam_ray, as it did before this header: calling the two
// functions instead gives it another register allocation, and its instruction stream is held to what DESIGN.md 4.28 measured.
#ifndef BL_BEAM_DEV_H
#define BL_BEAM_DEV_H

#include "bl_internal.h"

#define BEAM_HIT 0                        // the tables' places in the block of BEAM_TABLE_WORDS words
#define BEAM_SHORT 1024
#define BEAM_LT 2048
#define BEAM_TABLE_WORDS 2304

__device__ __forceinline__ int beam_quarter(int ax, int ay, int bx, int by)
{
    const int dx = ax - bx, dy = ay - by;
    const uint32_t v = 16u * (uint32_t)(dx * dx + dy * dy);            // below 2^31: the cells lie within reach + 2 <= 4098 of each other
    uint32_t r = (uint32_t)__builtin_sqrtf((float)v);
    while (r * r > v) --r;
    while ((r + 1u) * (r + 1u) <= v) ++r;
    return (int)r;
}

// p of a return of z quarter cells; zstar: the expected hit's, read only with `expect`
__device__ __forceinline__ uint32_t beam_return_p(const uint32_t* s_tab, uint32_t rnd, int hit_cut, bool expect, int z, int zstar)
{
    uint32_t p = rnd;
    if (expect) p += s_tab[BEAM_HIT + min(abs(z - zstar), hit_cut)];
    if (!expect || z < zstar) p += s_tab[BEAM_SHORT + min(z >> 2, 1023)];
    return p;
}

__device__ __forceinline__ int beam_lg(const uint32_t* s_tab, uint32_t p, int ln2)
{
    const int e = 31 - __clz((int)p);                                   // p >= 1: bl_beam_set_params
    const uint32_t mant = ((p << (31 - e)) >> 23) & 255u;
    return (e - 30) * ln2 + (int)s_tab[BEAM_LT + mant];
}

#endif
