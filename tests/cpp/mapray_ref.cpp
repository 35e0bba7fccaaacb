// bl_mapray_dev.h's host-and-device part, array by array, for tests/test_mapray_header_cpu.py (built as a shared object by the
// test with -ffp-contract=off, as the library is): the walk from any step, the per-cell form, the start and end cells of a scan.
#include "../../botlab_amd/csrc/bl_mapray_dev.h"

extern "C" {

// cells k0 .. min(k0 + count, K) - 1 of the walk of ray = (x0, y0, x1, y1) into xy[2 i], xy[2 i + 1]; returns how many
int mr_walk(const int* ray, int k0, int count, int* xy)
{
    int n = 0;
    bl_walk_range(make_int4(ray[0], ray[1], ray[2], ray[3]), k0, k0 + count, [&](int x, int y) { xy[2 * n] = x; xy[2 * n + 1] = y; ++n; });
    return n;
}

// bl_walk_cell for every k of ks[0 .. n - 1]
void mr_walk_cells(const int* ray, const int* ks, int n, int* xy)
{
    for (int i = 0; i < n; ++i) bl_walk_cell(make_int4(ray[0], ray[1], ray[2], ray[3]), ks[i], &xy[2 * i], &xy[2 * i + 1]);
}

int mr_ray_steps(const int* ray) { return bl_ray_steps(make_int4(ray[0], ray[1], ray[2], ray[3])); }
int mr_no_ray(void) { return BL_NO_RAY; }

// bl_ray_cells of n kept rays of a scan traced from pose pb = (x, y, theta) at utime tb to pe at te; frame = (ox, oy, mpc, cpm)
void mr_ray_cells(int width, int height, const float* frame, float max_laser, const float* pb, int64_t tb, const float* pe, int64_t te, int n,
                  const float* ranges, const float* thetas, const int64_t* times, int* out)
{
    bl_frame f;
    f.width = width; f.height = height; f.ox = frame[0]; f.oy = frame[1]; f.mpc = frame[2]; f.cpm = frame[3];
    const bl_pose3 b = {pb[0], pb[1], pb[2]}, e = {pe[0], pe[1], pe[2]};
    const bool interp = tb != te;
    const double t_den = interp ? (double)(te - tb) : 1.0;
    for (int i = 0; i < n; ++i) {
        const int4 r = bl_ray_cells(f, max_laser, interp, tb, t_den, b, e, ranges[i], thetas[i], interp ? times[i] : 0);
        out[4 * i] = r.x; out[4 * i + 1] = r.y; out[4 * i + 2] = r.z; out[4 * i + 3] = r.w;
    }
}

}
