// localplan_cpu_ref.cpp -- the local planner's definition (include/botlab_hip.h, "local planner") as a plain single-thread C++
// loop, for the comparison in DESIGN.md 4.17: the same candidate set the device evaluates, on one host core, with libm's sinf / cosf
// once per (j, k) as the kernel shares them.  Reads the dump tests/tools/localplan_measure.py writes and prints the winner of every
// state and the time per full evaluation.
//   g++ -O2 -ffp-contract=off -o localplan_cpu_ref localplan_cpu_ref.cpp ; localplan_cpu_ref <dump> [repetitions]
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

struct Head { int32_t W, H, table_n, n_states, n_v, n_w, n_steps, w_field, w_heading, w_clear, w_speed; float mpc, cpm, ox, oy, dt_sim; };
struct State { int64_t utime; float x, y, theta, pad, v, w; };
static const int DX[8] = {1, -1, 0, 0, 1, -1, 1, -1}, DY[8] = {0, 0, 1, -1, 1, 1, -1, -1};
static const uint32_t UNREACHED = 0xFFFFFFFFu;

static float wrap_to_pi(float a)
{
    while ((double)a < -M_PI) a = (float)((double)a + 2.0 * M_PI);
    while ((double)a > M_PI) a = (float)((double)a - 2.0 * M_PI);
    return a;
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    const int reps = argc > 2 ? std::atoi(argv[2]) : 5;
    Head h;
    if (std::fread(&h, sizeof(h), 1, f) != 1) return 2;
    std::vector<uint32_t> field((size_t)h.W * h.H);
    std::vector<uint16_t> l1((size_t)h.W * h.H);
    std::vector<int32_t> table((size_t)h.table_n);
    std::vector<State> states((size_t)h.n_states);
    std::vector<float> vt((size_t)h.n_states * h.n_v), wt((size_t)h.n_states * h.n_w);
    if (std::fread(field.data(), 4, field.size(), f) != field.size() || std::fread(l1.data(), 2, l1.size(), f) != l1.size() ||
        std::fread(table.data(), 4, table.size(), f) != table.size() || std::fread(states.data(), sizeof(State), states.size(), f) != states.size() ||
        std::fread(vt.data(), 4, vt.size(), f) != vt.size() || std::fread(wt.data(), 4, wt.size(), f) != wt.size()) return 2;
    std::fclose(f);
    auto cost_of = [&](int x, int y) -> int {
        if (x < 0 || y < 0 || x >= h.W || y >= h.H) return -1;
        const int n = l1[(size_t)y * h.W + x];
        return (n == 0xFFFF || n >= h.table_n) ? -1 : table[(size_t)n];
    };
    const float ang[8] = {0.0f, (float)M_PI, (float)(M_PI / 2), (float)(-M_PI / 2), (float)(M_PI / 4), (float)(3 * M_PI / 4), (float)(-M_PI / 4), (float)(-3 * M_PI / 4)};
    const float kh = (float)(1024.0 / M_PI);
    std::vector<float> cs((size_t)h.n_steps), sn((size_t)h.n_steps);
    std::vector<int> win((size_t)h.n_states);
    std::vector<long long> wcost((size_t)h.n_states);
    std::vector<double> times;
    for (int rep = 0; rep < reps; ++rep) {
        const auto t0 = std::chrono::steady_clock::now();
        for (int s = 0; s < h.n_states; ++s) {
            const State& st = states[(size_t)s];
            long long best = INT64_MAX; int bc = -1;
            for (int j = 0; j < h.n_w; ++j) {
                float th = wrap_to_pi(st.theta);
                const float dth = wt[(size_t)s * h.n_w + j] * h.dt_sim;
                for (int k = 0; k < h.n_steps; ++k) { cs[(size_t)k] = cosf(th); sn[(size_t)k] = sinf(th); th = wrap_to_pi(th + dth); }
                for (int i = 0; i < h.n_v; ++i) {
                    const float step = vt[(size_t)s * h.n_v + i] * h.dt_sim;
                    float x = st.x, y = st.y;
                    int ex = 0, ey = 0, pen = 0; bool ok = true;
                    for (int k = 0; k < h.n_steps && ok; ++k) {
                        x = x + step * cs[(size_t)k]; y = y + step * sn[(size_t)k];
                        const double vx = ((double)x - (double)h.ox) * (double)h.cpm, vy = ((double)y - (double)h.oy) * (double)h.cpm;
                        if (!(vx > -1.0 && vx < (double)h.W && vy > -1.0 && vy < (double)h.H)) { ok = false; break; }
                        ex = (int)vx; ey = (int)vy;
                        const int q = cost_of(ex, ey);
                        if (q < 0) ok = false; else pen += q;
                    }
                    if (!ok) continue;
                    const uint32_t fe = field[(size_t)ey * h.W + ex];
                    if (fe == UNREACHED) continue;
                    int hd = 0;
                    if (fe != 0) {
                        const bool px = cost_of(ex + 1, ey) >= 0, mx = cost_of(ex - 1, ey) >= 0, py = cost_of(ex, ey + 1) >= 0, my = cost_of(ex, ey - 1) >= 0;
                        uint32_t bw = UNREACHED; int bm = -1;
                        for (int m = 0; m < 8; ++m) {
                            bool okm = m < 4 ? (m == 0 ? px : m == 1 ? mx : m == 2 ? py : my)
                                             : ((DX[m] > 0 ? px : mx) && (DY[m] > 0 ? py : my) && cost_of(ex + DX[m], ey + DY[m]) >= 0);
                            if (!okm) continue;
                            const uint32_t v = field[(size_t)(ey + DY[m]) * h.W + ex + DX[m]];
                            if (v == UNREACHED) continue;
                            const uint32_t w = v + (m < 4 ? 10u : 14u);
                            if (w < bw) { bw = w; bm = m; }
                        }
                        if (bm < 0) hd = 1024;
                        else {
                            double d = (double)th - (double)ang[bm];
                            if (std::fabs(d) > M_PI) d -= d > 0 ? 2 * M_PI : -2 * M_PI;
                            hd = (int)floorf(fabsf((float)d) * kh);
                        }
                    }
                    const long long c = (long long)h.w_field * fe + (long long)h.w_heading * hd + (long long)h.w_clear * pen + (long long)h.w_speed * (h.n_v - 1 - i);
                    if (c < best) { best = c; bc = j * h.n_v + i; }
                }
            }
            win[(size_t)s] = bc; wcost[(size_t)s] = best;
        }
        times.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    for (int s = 0; s < h.n_states; ++s) std::printf("state %d winner %d cost %lld\n", s, win[(size_t)s], wcost[(size_t)s]);
    double lo = times[0], hi = times[0];
    for (double t : times) { if (t < lo) lo = t; if (t > hi) hi = t; }
    std::printf("cpu_ref: %d states x %d candidates x %d steps, %d repetitions, ms per call min %.3f max %.3f, per state min %.3f\n", h.n_states,
                h.n_v * h.n_w, h.n_steps, reps, lo, hi, lo / h.n_states);
    return 0;
}
