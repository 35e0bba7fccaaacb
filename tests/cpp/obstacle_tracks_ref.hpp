// obstacle_tracks_ref.hpp -- the obstacle tracks in plain C++ on the host, written from the definition in include/botlab_hip.h
// ("obstacle tracks") the way tests/obstacle_tracks_model.py is: blobs by flood fill, the association by sorting the candidate
// pairs.  No device code and nothing of the library but its struct types.  tests/cpp/obstacle_tracks_test.cpp walks it beside the
// device; tests/cpp/obstacle_tracks_ref_main.cpp runs it alone (the program that is built with the sanitizers).
#ifndef OBSTACLE_TRACKS_REF_HPP
#define OBSTACLE_TRACKS_REF_HPP

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include <botlab_hip.h>

namespace obt_ref {

inline long long floor_shift8(long long v) { return v >= 0 ? v / 256 : -((-v + 255) / 256); }       // floor(v / 256)
inline int stamp_offset(int s, int v) { const int a = s * v + 512; return a >= 0 ? a / 1024 : -((-a + 1023) / 1024); }

inline bool params_ok(const bl_obstracks_params_t& p)
{
    return p.min_cells >= 1 && p.min_cells <= 65536 && p.max_cells >= p.min_cells && p.max_cells <= 65536 && p.gate_cells >= 1 && p.gate_cells <= 64 &&
           p.alpha >= 0 && p.alpha <= 256 && p.beta >= 0 && p.beta <= 256 && p.confirm_hits >= 1 && p.confirm_hits <= 255 && p.max_missed >= 0 &&
           p.max_missed <= 255 && p.min_speed >= 0 && p.min_speed <= 1023;
}

struct Pair { long long d2; int i, j; };
inline bool operator<(const Pair& a, const Pair& b) { return a.d2 != b.d2 ? a.d2 < b.d2 : a.i != b.i ? a.i < b.i : a.j < b.j; }

struct Tracker {
    int W, H;
    bl_obstracks_params_t p;
    std::vector<bl_obstrack_t> slots;
    uint32_t next_id, n;
    bool fresh;
    std::vector<bl_obsblob_t> blobs;
    std::vector<int32_t> labels, live_xy;
    bl_obstracks_stats_t st;

    Tracker(int w, int h, const bl_obstracks_params_t& params) : W(w), H(h), p(params) { reset(); }

    void forget_blobs(int live_cells)
    {
        blobs.clear(); live_xy.clear();
        labels.assign(static_cast<std::size_t>(std::min(live_cells, BL_OBSTRACKS_MAX_CELLS)), -1);
        std::memset(&st, 0, sizeof(st));
        st.live_cells = live_cells;
    }
    void reset()
    {
        bl_obstrack_t z;
        std::memset(&z, 0, sizeof(z));
        slots.assign(BL_OBSTRACKS_MAX_TRACKS, z);
        for (int i = 0; i < BL_OBSTRACKS_MAX_TRACKS; ++i) slots[static_cast<std::size_t>(i)].slot = i;
        next_id = 1; n = 0; fresh = true;
        forget_blobs(0);
    }
    bool set_params(const bl_obstracks_params_t& q) { if (!params_ok(q)) return false; p = q; return true; }
    void count_tracks()
    {
        st.tracks = 0; st.confirmed = 0;
        for (const bl_obstrack_t& t : slots) if (t.id != 0u) { ++st.tracks; st.confirmed += (t.flags & BL_OBSTRACK_CONFIRMED) ? 1 : 0; }
    }
    bool upload(const std::vector<bl_obstrack_t>& in, const bl_obstracks_state_t& s)
    {
        if (in.size() != BL_OBSTRACKS_MAX_TRACKS || s.next_id < 1u) return false;
        std::vector<bl_obstrack_t> all(in);
        for (std::size_t i = 0; i < all.size(); ++i) {
            bl_obstrack_t& t = all[i];
            if (t.id == 0u) std::memset(&t, 0, sizeof(t));
            else {
                if (t.id >= s.next_id) return false;
                for (std::size_t k = 0; k < i; ++k) if (in[k].id == t.id) return false;
                if (t.vx < -1023 || t.vx > 1023 || t.vy < -1023 || t.vy > 1023) return false;
                if (t.px < -(1 << 30) || t.px > (1 << 30) || t.py < -(1 << 30) || t.py > (1 << 30)) return false;
                if (t.hits < 1 || t.hits > 65535 || t.missed < 0 || t.missed > 255) return false;
            }
            t.slot = static_cast<int32_t>(i);
        }
        slots = all; next_id = s.next_id; n = s.n; fresh = s.fresh != 0;
        forget_blobs(0);
        count_tracks();
        return true;
    }
    void refuse(int code, int live_cells) { forget_blobs(live_cells); st.refused = code; count_tracks(); }
    bl_obstracks_stats_t stats() const { bl_obstracks_stats_t s = st; s.n = n; s.next_id = next_id; return s; }
    std::vector<bl_obstrack_t> tracks() const
    {
        std::vector<bl_obstrack_t> out;
        for (const bl_obstrack_t& t : slots) if (t.id != 0u) out.push_back(t);
        return out;
    }

    // live: W * H bytes, nonzero where the layer's live(c) holds; the status the library would give
    int update(const std::vector<uint8_t>& live, uint32_t layer_n)
    {
        if (!fresh && layer_n != n + 1u) return BL_ERR_STATE;
        n = layer_n; fresh = false;
        int L = 0;
        for (uint8_t v : live) L += v ? 1 : 0;
        if (L > BL_OBSTRACKS_MAX_CELLS) { refuse(BL_OBSTRACKS_REFUSED_CELLS, L); return BL_OK; }
        // ---- blobs by flood fill, met in row-major order
        std::vector<int32_t> lab(live.size(), -1), xy, stack;
        std::vector<bl_obsblob_t> all;
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const std::size_t c = static_cast<std::size_t>(y) * W + x;
                if (!live[c]) continue;
                xy.push_back(x); xy.push_back(y);
                if (lab[c] >= 0) continue;
                bl_obsblob_t b;
                std::memset(&b, 0, sizeof(b));
                b.x0 = x; b.x1 = x; b.y0 = y; b.y1 = y; b.track = -1; b.rep = static_cast<int32_t>(c);
                const int32_t k = static_cast<int32_t>(all.size());
                lab[c] = k;
                stack.assign(1, static_cast<int32_t>(c));
                while (!stack.empty()) {
                    const int32_t cc = stack.back();
                    stack.pop_back();
                    const int cx = cc % W, cy = cc / W;
                    b.area += 1; b.sum_x += cx; b.sum_y += cy;
                    b.x0 = std::min(b.x0, cx); b.x1 = std::max(b.x1, cx); b.y0 = std::min(b.y0, cy); b.y1 = std::max(b.y1, cy);
                    for (int dy = -1; dy <= 1; ++dy)
                        for (int dx = -1; dx <= 1; ++dx) {
                            const int nx = cx + dx, ny = cy + dy;
                            if (nx < 0 || nx >= W || ny < 0 || ny >= H) continue;
                            const std::size_t nc = static_cast<std::size_t>(ny) * W + nx;
                            if (live[nc] && lab[nc] < 0) { lab[nc] = k; stack.push_back(static_cast<int32_t>(nc)); }
                        }
                }
                b.cx = static_cast<int32_t>((256 * b.sum_x) / b.area) + 128; b.cy = static_cast<int32_t>((256 * b.sum_y) / b.area) + 128;
                b.eligible = (b.area >= p.min_cells && b.area <= p.max_cells) ? 1 : 0;
                all.push_back(b);
            }
        const int nblobs = static_cast<int>(all.size()), kept = std::min(nblobs, BL_OBSTRACKS_MAX_BLOBS);
        std::vector<bl_obsblob_t> kb(all.begin(), all.begin() + kept);
        // ---- the candidate pairs, sorted
        std::vector<bl_obstrack_t> s(slots);
        std::vector<Pair> pairs;
        const long long g = 256ll * p.gate_cells;
        int eligible = 0;
        for (int j = 0; j < kept; ++j) eligible += kb[static_cast<std::size_t>(j)].eligible;
        for (int i = 0; i < BL_OBSTRACKS_MAX_TRACKS; ++i) {
            const bl_obstrack_t& t = s[static_cast<std::size_t>(i)];
            if (t.id == 0u) continue;
            for (int j = 0; j < kept; ++j) {
                const bl_obsblob_t& b = kb[static_cast<std::size_t>(j)];
                if (!b.eligible) continue;
                const long long dx = static_cast<long long>(b.cx) - (static_cast<long long>(t.px) + t.vx);
                const long long dy = static_cast<long long>(b.cy) - (static_cast<long long>(t.py) + t.vy);
                if (dx > g || dx < -g || dy > g || dy < -g) continue;
                const Pair q = {dx * dx + dy * dy, i, j};
                if (q.d2 <= g * g) pairs.push_back(q);
            }
        }
        std::sort(pairs.begin(), pairs.end());
        std::vector<int> tmatch(BL_OBSTRACKS_MAX_TRACKS, -1), bmatch(static_cast<std::size_t>(kept), -1);
        int matched = 0;
        for (const Pair& q : pairs)
            if (tmatch[static_cast<std::size_t>(q.i)] < 0 && bmatch[static_cast<std::size_t>(q.j)] < 0) {
                tmatch[static_cast<std::size_t>(q.i)] = q.j; bmatch[static_cast<std::size_t>(q.j)] = q.i; ++matched;
            }
        // ---- transition
        int deleted = 0;
        for (int i = 0; i < BL_OBSTRACKS_MAX_TRACKS; ++i) {
            bl_obstrack_t& t = s[static_cast<std::size_t>(i)];
            if (t.id == 0u) continue;
            const int px = t.px + t.vx, py = t.py + t.vy;
            const int j = tmatch[static_cast<std::size_t>(i)];
            if (j >= 0) {
                bl_obsblob_t& b = kb[static_cast<std::size_t>(j)];
                const int rx = b.cx - px, ry = b.cy - py;
                t.px = px + static_cast<int>(floor_shift8(static_cast<long long>(p.alpha) * rx));
                t.py = py + static_cast<int>(floor_shift8(static_cast<long long>(p.alpha) * ry));
                t.vx = std::max(-1023, std::min(1023, t.vx + static_cast<int>(floor_shift8(static_cast<long long>(p.beta) * rx))));
                t.vy = std::max(-1023, std::min(1023, t.vy + static_cast<int>(floor_shift8(static_cast<long long>(p.beta) * ry))));
                t.hits = std::min(t.hits + 1, 65535); t.missed = 0;
                t.area = b.area; t.x0 = b.x0; t.y0 = b.y0; t.x1 = b.x1; t.y1 = b.y1;
                t.flags = BL_OBSTRACK_MATCHED;
                b.track = i;
            } else {
                t.px = px; t.py = py;
                t.missed = std::min(t.missed + 1, 65535);
                t.flags = 0;
                if (t.missed > p.max_missed) { std::memset(&t, 0, sizeof(t)); ++deleted; }
            }
        }
        std::vector<int> wanted, free_slots;
        for (int j = 0; j < kept; ++j) if (kb[static_cast<std::size_t>(j)].eligible && bmatch[static_cast<std::size_t>(j)] < 0) wanted.push_back(j);
        for (int i = 0; i < BL_OBSTRACKS_MAX_TRACKS; ++i) if (s[static_cast<std::size_t>(i)].id == 0u) free_slots.push_back(i);
        const int nb = static_cast<int>(std::min(wanted.size(), free_slots.size()));
        if (nb > 0 && static_cast<unsigned long long>(next_id) + static_cast<unsigned long long>(nb) - 1ull >= 0xffffffffull) {
            refuse(BL_OBSTRACKS_REFUSED_IDS, L);
            return BL_OK;
        }
        for (int k = 0; k < nb; ++k) {
            bl_obsblob_t& b = kb[static_cast<std::size_t>(wanted[static_cast<std::size_t>(k)])];
            const int i = free_slots[static_cast<std::size_t>(k)];
            bl_obstrack_t& t = s[static_cast<std::size_t>(i)];
            t.id = next_id + static_cast<uint32_t>(k);
            t.px = b.cx; t.py = b.cy; t.vx = 0; t.vy = 0; t.hits = 1; t.missed = 0;
            t.area = b.area; t.x0 = b.x0; t.y0 = b.y0; t.x1 = b.x1; t.y1 = b.y1;
            t.flags = BL_OBSTRACK_BORN;
            b.track = i;
        }
        for (int i = 0; i < BL_OBSTRACKS_MAX_TRACKS; ++i) {
            bl_obstrack_t& t = s[static_cast<std::size_t>(i)];
            t.slot = i;
            if (t.id == 0u) continue;
            if (t.hits >= p.confirm_hits) t.flags |= BL_OBSTRACK_CONFIRMED;
            if (t.vx * t.vx + t.vy * t.vy >= p.min_speed * p.min_speed) t.flags |= BL_OBSTRACK_MOVING;
        }
        slots = s; blobs = kb; next_id += static_cast<uint32_t>(nb);
        live_xy = xy;
        labels.clear();
        for (std::size_t k = 0; k < xy.size(); k += 2) {
            const int32_t l = lab[static_cast<std::size_t>(xy[k + 1]) * W + xy[k]];
            labels.push_back(l < BL_OBSTRACKS_MAX_BLOBS ? l : -1);
        }
        std::memset(&st, 0, sizeof(st));
        st.live_cells = L; st.blobs = nblobs; st.eligible = eligible; st.dropped = nblobs - kept; st.matched = matched; st.born = nb;
        st.deleted = deleted; st.unborn = static_cast<int>(wanted.size()) - nb;
        count_tracks();
        return BL_OK;
    }

    // the composed grid; live_now / layer_n: the layer as it stands.  The status the library would give.
    int compose(const std::vector<uint8_t>& live_now, uint32_t layer_n, const std::vector<int8_t>& map, int horizon, int rx, int ry, int keep,
                std::vector<int8_t>& out) const
    {
        if (horizon < 0 || horizon > BL_OBSTRACKS_MAX_HORIZON || keep < -1 || keep > BL_OBSTRACKS_MAX_KEEP_CLEAR) return BL_ERR_ARG;
        if (horizon > 0 && !fresh && layer_n != n) return BL_ERR_STATE;
        out = map;
        for (std::size_t c = 0; c < out.size(); ++c) if (live_now[c]) out[c] = 127;
        const int want = BL_OBSTRACK_CONFIRMED | BL_OBSTRACK_MOVING;
        for (std::size_t k = 0; k < labels.size() && 2 * k + 1 < live_xy.size(); ++k) {
            const int32_t l = labels[k];
            if (horizon == 0 || l < 0 || blobs[static_cast<std::size_t>(l)].track < 0) continue;
            const bl_obstrack_t& t = slots[static_cast<std::size_t>(blobs[static_cast<std::size_t>(l)].track)];
            if ((t.flags & want) != want) continue;
            for (int s = 1; s <= 4 * horizon; ++s) {
                const int sx = live_xy[2 * k] + stamp_offset(s, t.vx), sy = live_xy[2 * k + 1] + stamp_offset(s, t.vy);
                if (sx < 0 || sx >= W || sy < 0 || sy >= H) continue;
                if (keep >= 0 && std::abs(static_cast<long long>(sx) - rx) <= keep && std::abs(static_cast<long long>(sy) - ry) <= keep) continue;
                out[static_cast<std::size_t>(sy) * W + sx] = 127;
            }
        }
        return BL_OK;
    }
};

}  // namespace obt_ref

#endif  // OBSTACLE_TRACKS_REF_HPP
