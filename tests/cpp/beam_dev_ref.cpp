// bl_beam_dev.h's host-and-device part, array by array, for tests/test_beam_dev_header_cpu.py (built as a shared object by the test
// with -ffp-contract=off, as the library is): the start cell, the first-hit walk in both of its grid-leaving forms, the length in
// quarter cells, a return's probability, the integer logarithm and the look-up's heading index.
#include "../../botlab_amd/csrc/bl_beam_dev.h"

extern "C" {

// beam_start of n poses (x, y, theta); frame = (ox, oy, mpc, cpm).  out: ok, sx, sy per pose; pos: px, py per pose
void bd_start(int n, const float* poses, int width, int height, const float* frame, int* out, float* pos)
{
    bl_frame f;
    f.width = width; f.height = height; f.ox = frame[0]; f.oy = frame[1]; f.mpc = frame[2]; f.cpm = frame[3];
    for (int i = 0; i < n; ++i) {
        const float4 p = {poses[3 * i], poses[3 * i + 1], poses[3 * i + 2], 0.0f};
        float px = 0.0f, py = 0.0f;
        int sx = 0, sy = 0;
        out[3 * i] = beam_start(p, f, &px, &py, &sx, &sy) ? 1 : 0;
        out[3 * i + 1] = sx; out[3 * i + 2] = sy;
        pos[2 * i] = px; pos[2 * i + 1] = py;
    }
}

// beam_first_hit over a W x H grid of cells, occupied at >= occ_min.  stop = 0: the walk goes on outside the grid, where no cell
// is occupied (beam_ray's form); stop = 1: it ends at the first cell outside (k_rt_build's form).  out: first, K, x, y
void bd_first_hit(const int8_t* cells, int W, int H, int occ_min, int sx, int sy, int tx, int ty, int stop, int* out)
{
    const auto inside = [&](int x, int y) { return (unsigned int)x < (unsigned int)W && (unsigned int)y < (unsigned int)H; };
    beam_hit h;
    if (stop)
        h = beam_first_hit(sx, sy, tx, ty, [&](int x, int y) { return cells[(size_t)y * W + x] >= occ_min; },
                           [&](int x, int y) { return !inside(x, y); });
    else
        h = beam_first_hit(sx, sy, tx, ty, [&](int x, int y) { return inside(x, y) && cells[(size_t)y * W + x] >= occ_min; });
    out[0] = h.first; out[1] = h.K; out[2] = h.x; out[3] = h.y;
}

void bd_quarter(int n, const int* a, int* out)
{
    for (int i = 0; i < n; ++i) out[i] = beam_quarter(a[4 * i], a[4 * i + 1], a[4 * i + 2], a[4 * i + 3]);
}

// tab: BEAM_TABLE_WORDS words, Hit | Short | Lt
uint32_t bd_return_p(const uint32_t* tab, uint32_t rnd, int hit_cut, int expect, int z, int zstar)
{
    return beam_return_p(tab, rnd, hit_cut, expect != 0, z, zstar);
}

int bd_lg(const uint32_t* tab, uint32_t p, int ln2) { return beam_lg(tab, p, ln2); }

void bd_heading_index(int n, const float* ang, float kf, int Hn, int* out)
{
    for (int i = 0; i < n; ++i) out[i] = beam_heading_index(ang[i], kf, Hn);
}

int bd_table_words(void) { return BEAM_TABLE_WORDS; }
int bd_table_place(int which) { return which == 0 ? BEAM_HIT : which == 1 ? BEAM_SHORT : BEAM_LT; }

}
