// obstacle_tracks_test.cpp -- ObstacleTrackerT (include/botlab/obstacle_tracks.hpp) and MotionPlannerT::setMapWithTracks
// (include/botlab/planning_dropin.hpp) over a step stream (obstacle_tracks_stream.hpp), driven by
// tests/test_gpu_obstacle_tracks_cpp.py.  Arguments: input, output.  After an accepted 'C' the output also holds 'D' and the planner's
// distances (float per cell).  The host reference (obstacle_tracks_ref.hpp) walks beside the device: a slot, a blob, a label or a
// figure of the stats that differs ends the program with status 1.
#include <cstring>
#include "dropin_test_types.hpp"
#include <botlab/obstacle_tracks.hpp>
#include <botlab/planning_dropin.hpp>
#include "obstacle_tracks_ref.hpp"
#include "obstacle_tracks_stream.hpp"

using namespace obt_stream;
typedef botlab_hip::ObstacleLayerT<pose_xyt_t, lidar_t> Layer;
typedef botlab_hip::ObstacleTrackerT<Layer> Tracker;
typedef botlab_hip::MotionPlannerT<pose_xyt_t, robot_path_t> Planner;

template <class T> static bool same(const std::vector<T>& a, const std::vector<T>& b)
{
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

int main(int argc, char** argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: obstacle_tracks_test input output\n"); return 2; }
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) { std::fprintf(stderr, "cannot open files\n"); return 2; }
    const Header hd = read_header(in);
    const size_t cells = hd.cells.size();
    occupancy_grid_t msg;
    msg.width = hd.w; msg.height = hd.h; msg.meters_per_cell = hd.mpc; msg.origin_x = hd.ox; msg.origin_y = hd.oy;
    msg.num_cells = hd.w * hd.h;
    msg.cells = hd.cells;
    botlab_hip::OccupancyGrid map;
    map.fromLCM(msg);
    Layer layer(hd.w, hd.h, hd.lp);
    Tracker tracker(layer, hd.tp);
    Planner planner;
    obt_ref::Tracker ref(hd.w, hd.h, hd.tp);
    std::vector<uint8_t> count(cells, 0), live(cells, 0);
    std::vector<uint32_t> last(cells, 0);
    uint32_t n = 0;
    int steps = 0;
    for (;; ++steps) {
        char op = 0;
        rd(in, &op, 1);
        if (op == 'E') break;
        if (op == 'L') {
            rd(in, count.data(), cells); rd(in, last.data(), 4 * cells); rd(in, &n, 4);
            layer.upload(count, last, n);
            put_i32(out, 'L', 0);
        } else if (op == 'U') {
            const int rc = tracker.tryUpdate();
            for (size_t c = 0; c < cells; ++c)
                live[c] = (count[c] >= static_cast<uint32_t>(hd.lp.min_hits) && last[c] != 0u && n - last[c] < static_cast<uint32_t>(hd.lp.ttl_scans)) ? 1 : 0;
            const int ref_rc = ref.update(live, n);
            const std::vector<bl_obstrack_t> t = tracker.tracks();
            const std::vector<bl_obsblob_t> b = tracker.blobs();
            const std::vector<int32_t> l = tracker.labels();
            bl_obstracks_stats_t st = tracker.stats(), rst = ref.stats();
            rst.rounds = st.rounds;                                     // the reference sorts: it has no rounds
            if (rc != ref_rc || !same(t, ref.tracks()) || !same(b, ref.blobs) || !same(l, ref.labels) || std::memcmp(&st, &rst, sizeof(st)) != 0) {
                std::fprintf(stderr, "step %d: the device and the host reference differ (status %d / %d, %zu / %zu tracks, %zu / %zu blobs)\n", steps, rc,
                             ref_rc, t.size(), ref.tracks().size(), b.size(), ref.blobs.size());
                return 1;
            }
            put_update(out, rc, t, b, l, st);
        } else if (op == 'R') {
            tracker.reset(); ref.reset();
            put_i32(out, 'R', 0);
        } else if (op == 'T') {
            std::vector<bl_obstrack_t> slots;
            bl_obstracks_state_t s;
            tracker.download(slots, s);
            const bool ok = tracker.upload(slots, s);
            (void)ref.upload(slots, s);
            put_i32(out, 'T', ok ? 0 : 1);
        } else if (op == 'S') {
            std::vector<bl_obstrack_t> slots(BL_OBSTRACKS_MAX_TRACKS);
            bl_obstracks_state_t s;
            rd(in, slots.data(), slots.size() * sizeof(bl_obstrack_t)); rd(in, &s, sizeof(s));
            const bool ok = tracker.upload(slots, s);
            if (ok != ref.upload(slots, s)) { std::fprintf(stderr, "step %d: upload accepted by one only\n", steps); return 1; }
            put_i32(out, 'S', ok ? 0 : 1);
        } else if (op == 'P') {
            bl_obstracks_params_t q;
            rd(in, &q, sizeof(q));
            const bool ok = tracker.setParams(q);
            if (ok != ref.set_params(q)) { std::fprintf(stderr, "step %d: parameters accepted by one only\n", steps); return 1; }
            put_i32(out, 'P', ok ? 0 : 1);
        } else if (op == 'C') {
            int32_t horizon = 0, keep = 0;
            pose_xyt_t pose;
            pose.utime = 0; pose.theta = 0;
            rd(in, &horizon, 4); rd(in, &pose.x, 4); rd(in, &pose.y, 4); rd(in, &keep, 4);
            planner.setMapWithTracks(map, layer, tracker, horizon, pose, keep);   // (a refusal ends the program: the driver sends none)
            put_i32(out, 'C', 0);
            {
                const botlab_hip::OccupancyGrid& g = planner.composedMap();
                for (int y = 0; y < g.heightInCells(); ++y)
                    for (int x = 0; x < g.widthInCells(); ++x) { const int8_t v = g.logOdds(x, y); std::fwrite(&v, 1, 1, out); }
                std::fwrite("D", 1, 1, out);
                const botlab_hip::ObstacleDistanceGrid& d = planner.distances();
                for (int y = 0; y < d.heightInCells(); ++y)
                    for (int x = 0; x < d.widthInCells(); ++x) { const float v = d(x, y); std::fwrite(&v, 4, 1, out); }
            }
        } else {
            std::fprintf(stderr, "unknown step %d\n", static_cast<int>(op));
            return 2;
        }
    }
    for (int y = 0; y < map.heightInCells(); ++y)                       // the map itself is untouched
        for (int x = 0; x < map.widthInCells(); ++x)
            if (map.logOdds(x, y) != hd.cells[static_cast<size_t>(y) * hd.w + x]) { std::fprintf(stderr, "the map changed\n"); return 1; }
    std::fclose(out); std::fclose(in);
    std::printf("obstacle_tracks_test ok: %d steps\n", steps);
    return 0;
}
