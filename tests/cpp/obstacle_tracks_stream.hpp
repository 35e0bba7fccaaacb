// obstacle_tracks_stream.hpp -- the step stream that tests/obstacle_tracks_stream.py writes and both C++ programs of the obstacle
// tracks read (obstacle_tracks_test.cpp on the device, obstacle_tracks_ref_main.cpp on the host alone).
// Input:  width, height (int32), meters_per_cell, origin x, y (float), the cells (int8), the layer's parameters (float, 4 x int32),
//         the tracker's (8 x int32), then steps until 'E':
//           'L' count (uint8 per cell), last (uint32 per cell), n      the layer's state replaced
//           'U'  update        'R'  reset        'T'  download, then upload of what came back
//           'S' 256 slots (56 bytes each), state (16 bytes)            upload
//           'P' parameters (32 bytes)
//           'C' horizon (int32), robot pose x, y (float), keep_clear (int32)
// Output: per step its letter and the status (int32, 0 = accepted); after 'U' also the tracks, the blobs and the labels, each as a
//         count (int32) and the records, and the stats (56 bytes); after an accepted 'C' the composed grid (int8 per cell).
#ifndef OBSTACLE_TRACKS_STREAM_HPP
#define OBSTACLE_TRACKS_STREAM_HPP

#include <cstdio>
#include <cstdlib>
#include <vector>

#include <botlab_hip.h>

namespace obt_stream {

inline void rd(FILE* f, void* p, size_t n) { if (n && fread(p, 1, n, f) != n) { std::fprintf(stderr, "short read\n"); std::exit(2); } }
inline void put_i32(FILE* out, char tag, int32_t rc) { std::fwrite(&tag, 1, 1, out); std::fwrite(&rc, 4, 1, out); }

struct Header {
    int32_t w, h;
    float mpc, ox, oy;
    std::vector<int8_t> cells;
    bl_obslayer_params_t lp;
    bl_obstracks_params_t tp;
};

inline Header read_header(FILE* in)
{
    Header hd;
    rd(in, &hd.w, 4); rd(in, &hd.h, 4); rd(in, &hd.mpc, 4); rd(in, &hd.ox, 4); rd(in, &hd.oy, 4);
    if (hd.w < 1 || hd.h < 1 || hd.w > 4096 || hd.h > 4096) { std::fprintf(stderr, "bad shape\n"); std::exit(2); }
    hd.cells.resize(static_cast<size_t>(hd.w) * hd.h);
    rd(in, hd.cells.data(), hd.cells.size());
    rd(in, &hd.lp, sizeof(hd.lp)); rd(in, &hd.tp, sizeof(hd.tp));
    return hd;
}

inline void put_update(FILE* out, int32_t rc, const std::vector<bl_obstrack_t>& t, const std::vector<bl_obsblob_t>& b, const std::vector<int32_t>& l,
                       const bl_obstracks_stats_t& st)
{
    put_i32(out, 'U', rc);
    const int32_t nt = static_cast<int32_t>(t.size()), nb = static_cast<int32_t>(b.size()), nl = static_cast<int32_t>(l.size());
    std::fwrite(&nt, 4, 1, out); if (nt) std::fwrite(t.data(), sizeof(bl_obstrack_t), t.size(), out);
    std::fwrite(&nb, 4, 1, out); if (nb) std::fwrite(b.data(), sizeof(bl_obsblob_t), b.size(), out);
    std::fwrite(&nl, 4, 1, out); if (nl) std::fwrite(l.data(), 4, l.size(), out);
    std::fwrite(&st, sizeof(st), 1, out);
}

}  // namespace obt_stream

#endif  // OBSTACLE_TRACKS_STREAM_HPP
