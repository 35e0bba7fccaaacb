// bl_beam_dev.h's two first-hit walks compiled for the host, walk by walk over arrays, for tests/test_clearance_model_cpu.py (built
// as a shared object by the test with -ffp-contract=off, as the library is): beam_first_hit, ended where it leaves the grid, and
// beam_first_hit_leap over a clearance grid of the same cells.
#include "../../botlab_amd/csrc/bl_beam_dev.h"

extern "C" {

// n walks (sx, sy, tx, ty) with the start cell inside the W x H grid; cells occupied at >= occ_min, D their clearance grid.
// loop: first, K, x, y, reads per walk; leap: first, K, x, y, rounds per walk
void cd_walks(const int8_t* cells, const uint8_t* D, int W, int H, int occ_min, int n, const int* walks, int* loop, int* leap)
{
    const auto outside = [&](int x, int y) { return !((unsigned int)x < (unsigned int)W && (unsigned int)y < (unsigned int)H); };
    for (int i = 0; i < n; ++i) {
        const int sx = walks[4 * i], sy = walks[4 * i + 1], tx = walks[4 * i + 2], ty = walks[4 * i + 3];
        int reads = 0;
        const beam_hit a = beam_first_hit(sx, sy, tx, ty, [&](int x, int y) { ++reads; return cells[(size_t)y * W + x] >= occ_min; }, outside);
        const beam_leap_hit b = beam_first_hit_leap(sx, sy, tx, ty, [&](int x, int y) { return (int)D[(size_t)y * W + x]; }, outside);
        int* o = loop + 5 * i;
        o[0] = a.first; o[1] = a.K; o[2] = a.x; o[3] = a.y; o[4] = reads;
        o = leap + 5 * i;
        o[0] = b.first; o[1] = b.K; o[2] = b.x; o[3] = b.y; o[4] = b.rounds;
    }
}

}
