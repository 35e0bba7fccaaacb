// obstacle_tracks_ref_main.cpp -- the host reference of the obstacle tracks (obstacle_tracks_ref.hpp) over a step stream
// (obstacle_tracks_stream.hpp), with no GPU and no library: g++ -std=c++11 -I include.  Arguments: input, output.
// This is the program that is built with -fsanitize=address,undefined to check the association and transition logic's memory use.
#include <cmath>
#include "obstacle_tracks_ref.hpp"
#include "obstacle_tracks_stream.hpp"

using namespace obt_stream;

int main(int argc, char** argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: obstacle_tracks_ref_main input output\n"); return 2; }
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) { std::fprintf(stderr, "cannot open files\n"); return 2; }
    const Header hd = read_header(in);
    const size_t cells = hd.cells.size();
    obt_ref::Tracker tr(hd.w, hd.h, hd.tp);
    std::vector<uint8_t> count(cells, 0), live(cells, 0);
    std::vector<uint32_t> last(cells, 0);
    uint32_t n = 0;
    const float cpm = 1.0f / hd.mpc;
    int steps = 0;
    for (;; ++steps) {
        char op = 0;
        rd(in, &op, 1);
        if (op == 'E') break;
        if (op == 'L') {
            rd(in, count.data(), cells); rd(in, last.data(), 4 * cells); rd(in, &n, 4);
            put_i32(out, 'L', 0);
        } else if (op == 'U') {
            for (size_t c = 0; c < cells; ++c)
                live[c] = (count[c] >= static_cast<uint32_t>(hd.lp.min_hits) && last[c] != 0u && n - last[c] < static_cast<uint32_t>(hd.lp.ttl_scans)) ? 1 : 0;
            const int rc = tr.update(live, n);
            put_update(out, rc, tr.tracks(), tr.blobs, tr.labels, tr.stats());
        } else if (op == 'R') {
            tr.reset();
            put_i32(out, 'R', 0);
        } else if (op == 'T') {
            const std::vector<bl_obstrack_t> slots(tr.slots);
            bl_obstracks_state_t s;
            s.n = tr.n; s.next_id = tr.next_id; s.fresh = tr.fresh ? 1 : 0; s.reserved = 0;
            put_i32(out, 'T', tr.upload(slots, s) ? 0 : 1);
        } else if (op == 'S') {
            std::vector<bl_obstrack_t> slots(BL_OBSTRACKS_MAX_TRACKS);
            bl_obstracks_state_t s;
            rd(in, slots.data(), slots.size() * sizeof(bl_obstrack_t)); rd(in, &s, sizeof(s));
            put_i32(out, 'S', tr.upload(slots, s) ? 0 : 1);
        } else if (op == 'P') {
            bl_obstracks_params_t q;
            rd(in, &q, sizeof(q));
            put_i32(out, 'P', tr.set_params(q) ? 0 : 1);
        } else if (op == 'C') {
            int32_t horizon = 0, keep = 0;
            float x = 0, y = 0;
            rd(in, &horizon, 4); rd(in, &x, 4); rd(in, &y, 4); rd(in, &keep, 4);
            for (size_t c = 0; c < cells; ++c)
                live[c] = (count[c] >= static_cast<uint32_t>(hd.lp.min_hits) && last[c] != 0u && n - last[c] < static_cast<uint32_t>(hd.lp.ttl_scans)) ? 1 : 0;
            const int rx = static_cast<int>(std::floor((static_cast<double>(x) - hd.ox) * cpm)), ry = static_cast<int>(std::floor((static_cast<double>(y) - hd.oy) * cpm));
            std::vector<int8_t> composed;
            const int rc = tr.compose(live, n, hd.cells, horizon, rx, ry, keep, composed);
            put_i32(out, 'C', rc);
            if (rc == 0) std::fwrite(composed.data(), 1, composed.size(), out);
        } else {
            std::fprintf(stderr, "unknown step %d\n", static_cast<int>(op));
            return 2;
        }
    }
    std::fclose(out); std::fclose(in);
    std::printf("obstacle_tracks_ref_main ok: %d steps\n", steps);
    return 0;
}
