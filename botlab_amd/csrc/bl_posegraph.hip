// bl_posegraph.hip -- pose-graph back end (include/botlab_hip.h, "pose graph").
//
// Nodes x_k = (x, y, theta), a chain of N - 1 odometry edges (k, k + 1) and up to 1024 loop edges (i, j).  The cost is
// F = sum e' Omega e over the edges, e = (R(theta_i)' (t_j - t_i) - z_xy, wrap(theta_j - theta_i - z_theta)).  k_pg_solve minimises
// it by Gauss-Newton with Levenberg-Marquardt step control; ONE workgroup carries one graph from its first residual to its last
// pose, and workgroup s solves the graph whose loop edges are those of bit mask s.
//
// Every floating-point operation is a double + - * / rounded by itself (-ffp-contract=off, no fused operation anywhere in this
// file), every sum has one order, and tests/pose_graph_model.py restates them all: the two agree bit for bit.
//
//   edges    a thread per edge: e, chi2 = e' Omega e, and with the Jacobians A = de/dx_i, B = de/dx_j the blocks A'Omega A,
//            B'Omega B, A'Omega B and the vectors A'Omega e, B'Omega e.  The Jacobian of the held node is zero.
//   gather   a thread per node: its diagonal block D_k and gradient g_k, summed from 0 in ascending edge index -- chain edge k - 1,
//            chain edge k, then the node's loop edges by a list built once per solve.  No atomics.
//   try      H = D + lambda I (the held node: I) with the chain's A'Omega B beside the diagonal and one pair of blocks per loop edge.
//            H dx = -g by conjugate gradients preconditioned with the block-tridiagonal part T of H; T is factored once per try
//            by block cyclic reduction (floor(log2 N) + 1 levels) and the factors serve every iteration.
//   sums     thread t of PG_T adds its terms t, t + PG_T, ... in that order from 0, then the PG_T partial sums fold in halves:
//            p[t] += p[t + h], h = PG_T / 2 ... 1.
// All vectors live in the subset's workspace in global memory (L2-resident: 3 MB a graph at N = 4096), the loop edges' lists in LDS.
#include <string.h>

#include "bl_internal.h"

#define PG_T 512
#define PG_MAX_NODES 4096
#define PG_MAX_LOOPS 1024
#define PG_MAX_BYTES (1ull << 30)
#define PG_PI 3.141592653589793
#define PG_TWO_PI 6.283185307179586

// doubles of workspace per node and per edge (see pg_ws)
#define PG_NODE_DOUBLES 60
#define PG_EDGE_DOUBLES 33

struct bl_posegraph {
    bl_ctx* ctx;
    int max_nodes, max_loops, max_subsets;
    int n, n_loops;
    bool have_chain;
    int solved;                              // subsets of the last solve (0: none yet)
    int solved_n, solved_edges;
    bl_pose_xyt_t* d_nodes;                  // [max_nodes]
    bl_posegraph_edge_t* d_edges;            // chain at 0, loops at max_nodes - 1
    unsigned int* d_masks;                   // [max_subsets][32]
    double* d_ws; size_t ws_stride;          // per subset
    bl_pose_xyt_t* d_out;                    // [max_subsets][max_nodes]: the solved poses narrowed once
    bl_posegraph_result_t* d_results;        // [max_subsets]
    hipEvent_t ev[2];
};

struct pg_ws {
    double *x, *xn, *g, *dx, *r, *z, *p, *hp;        // 3 a node
    double *D, *Dl, *Dw;                             // 6 a node: the gathered blocks, with lambda, the reduction's (inverses in the end)
    double *Up, *Lo;                                 // 9 a node: block (k, k + s) of the reduction; block (k, k - s) frozen at elimination
    double *chi, *chi0, *chin;                       // 1 an edge: at x, at the start, at the trial
    double *AA, *BB, *AB, *ga, *gb;                  // 6, 6, 9, 3, 3 an edge
};

__host__ __device__ inline pg_ws pg_ws_of(double* base, int N, int E)
{
    pg_ws w; double* q = base;
    w.x = q; q += 3 * (size_t)N; w.xn = q; q += 3 * (size_t)N; w.g = q; q += 3 * (size_t)N; w.dx = q; q += 3 * (size_t)N;
    w.r = q; q += 3 * (size_t)N; w.z = q; q += 3 * (size_t)N; w.p = q; q += 3 * (size_t)N; w.hp = q; q += 3 * (size_t)N;
    w.D = q; q += 6 * (size_t)N; w.Dl = q; q += 6 * (size_t)N; w.Dw = q; q += 6 * (size_t)N;
    w.Up = q; q += 9 * (size_t)N; w.Lo = q; q += 9 * (size_t)N;
    w.chi = q; q += (size_t)E; w.chi0 = q; q += (size_t)E; w.chin = q; q += (size_t)E;
    w.AA = q; q += 6 * (size_t)E; w.BB = q; q += 6 * (size_t)E; w.AB = q; q += 9 * (size_t)E;
    w.ga = q; q += 3 * (size_t)E; w.gb = q; q += 3 * (size_t)E;
    return w;
}

// ---------------------------------------------------------------- 3 x 3 blocks: every entry (a0 b0 + a1 b1) + a2 b2
struct pg_m3 { double a[9]; };               // row-major
struct pg_s6 { double a[6]; };               // symmetric: xx, xy, yy, xt, yt, tt

__device__ __forceinline__ pg_m3 pg_full(const pg_s6 s)
{
    pg_m3 m;
    m.a[0] = s.a[0]; m.a[1] = s.a[1]; m.a[2] = s.a[3];
    m.a[3] = s.a[1]; m.a[4] = s.a[2]; m.a[5] = s.a[4];
    m.a[6] = s.a[3]; m.a[7] = s.a[4]; m.a[8] = s.a[5];
    return m;
}
__device__ __forceinline__ pg_m3 pg_tr(const pg_m3 m)
{
    pg_m3 t;
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) t.a[3 * r + c] = m.a[3 * c + r];
    return t;
}
__device__ __forceinline__ double pg_dot3(double a0, double b0, double a1, double b1, double a2, double b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }
__device__ __forceinline__ pg_m3 pg_mm(const pg_m3 A, const pg_m3 B)
{
    pg_m3 o;
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) o.a[3 * r + c] = pg_dot3(A.a[3 * r], B.a[c], A.a[3 * r + 1], B.a[3 + c], A.a[3 * r + 2], B.a[6 + c]);
    return o;
}
// the six upper entries of A B
__device__ __forceinline__ pg_s6 pg_mm_sym(const pg_m3 A, const pg_m3 B)
{
    const int R[6] = {0, 0, 1, 0, 1, 2}, Cc[6] = {0, 1, 1, 2, 2, 2};
    pg_s6 o;
    for (int q = 0; q < 6; ++q) o.a[q] = pg_dot3(A.a[3 * R[q]], B.a[Cc[q]], A.a[3 * R[q] + 1], B.a[3 + Cc[q]], A.a[3 * R[q] + 2], B.a[6 + Cc[q]]);
    return o;
}
__device__ __forceinline__ void pg_mv(const pg_m3 A, const double* v, double* o)
{
    for (int r = 0; r < 3; ++r) o[r] = pg_dot3(A.a[3 * r], v[0], A.a[3 * r + 1], v[1], A.a[3 * r + 2], v[2]);
}
// inverse of a symmetric block by cofactors, each entry divided by the determinant
__device__ __forceinline__ pg_s6 pg_inv(const pg_s6 s)
{
    const double a = s.a[0], b = s.a[1], c = s.a[2], d = s.a[3], e = s.a[4], f = s.a[5];
    const double c00 = c * f - e * e, c01 = d * e - b * f, c02 = b * e - c * d;
    const double c11 = a * f - d * d, c12 = b * d - a * e, c22 = a * c - b * b;
    const double det = (a * c00 + b * c01) + d * c02;
    pg_s6 o;
    o.a[0] = c00 / det; o.a[1] = c01 / det; o.a[2] = c11 / det; o.a[3] = c02 / det; o.a[4] = c12 / det; o.a[5] = c22 / det;
    return o;
}
__device__ __forceinline__ pg_m3 pg_ld9(const double* p) { pg_m3 m; for (int q = 0; q < 9; ++q) m.a[q] = p[q]; return m; }
__device__ __forceinline__ void pg_st9(double* p, const pg_m3 m) { for (int q = 0; q < 9; ++q) p[q] = m.a[q]; }
__device__ __forceinline__ pg_s6 pg_ld6(const double* p) { pg_s6 m; for (int q = 0; q < 6; ++q) m.a[q] = p[q]; return m; }
__device__ __forceinline__ void pg_st6(double* p, const pg_s6 m) { for (int q = 0; q < 6; ++q) p[q] = m.a[q]; }

__device__ __forceinline__ double pg_wrap(double d)
{
    if (d > PG_PI) d = d - PG_TWO_PI;
    else if (d < -PG_PI) d = d + PG_TWO_PI;
    return d;
}

// pose j seen from pose i, less z: the residual's three statements (z = 0: the relative pose itself)
__device__ __forceinline__ void pg_residual(const double* xi, const double* xj, const double* z, double* e, double* sn, double* cs, double* rx, double* ry)
{
    float sf, cf;
    bl_sincosf((float)xi[2], &sf, &cf);
    const double s = (double)sf, c = (double)cf;
    const double dx = xj[0] - xi[0], dy = xj[1] - xi[1];
    *rx = c * dx + s * dy;
    *ry = c * dy - s * dx;
    e[0] = *rx - z[0];
    e[1] = *ry - z[1];
    e[2] = pg_wrap((xj[2] - xi[2]) - z[2]);
    *sn = s; *cs = c;
}

// ---------------------------------------------------------------- sums over the workgroup (the same value to every thread)
__device__ __forceinline__ double pg_sum(double v, double* s_red)
{
    const int t = threadIdx.x;
    s_red[t] = v;
    __syncthreads();
    for (int h = PG_T / 2; h >= 64; h >>= 1) {
        if (t < h) s_red[t] = s_red[t] + s_red[t + h];
        __syncthreads();
    }
    if (t < 64) {
        double a = s_red[t];
        for (int h = 32; h >= 1; h >>= 1) a = a + __shfl_down(a, h, 64);
        if (t == 0) s_red[0] = a;
    }
    __syncthreads();
    const double r = s_red[0];
    __syncthreads();
    return r;
}
__device__ __forceinline__ double pg_max(double v, double* s_red)
{
    const int t = threadIdx.x;
    s_red[t] = v;
    __syncthreads();
    for (int h = PG_T / 2; h >= 1; h >>= 1) {
        if (t < h) s_red[t] = fmax(s_red[t], s_red[t + h]);
        __syncthreads();
    }
    const double r = s_red[0];
    __syncthreads();
    return r;
}
__device__ __forceinline__ double pg_dot(const double* a, const double* b, int N, double* s_red)
{
    double acc = 0.0;
    for (int k = threadIdx.x; k < N; k += PG_T) acc = acc + pg_dot3(a[3 * k], b[3 * k], a[3 * k + 1], b[3 * k + 1], a[3 * k + 2], b[3 * k + 2]);
    return pg_sum(acc, s_red);
}

struct pg_args {
    int N, L, words;
    bl_posegraph_params_t prm;
    const bl_pose_xyt_t* nodes;
    const bl_posegraph_edge_t* chain; const bl_posegraph_edge_t* loops;
    const unsigned int* masks;               // null: every loop edge on
    double* ws; size_t ws_stride;
    bl_pose_xyt_t* out; int out_stride;
    bl_posegraph_result_t* results;
};

struct pg_lds {
    double red[PG_T];
    int head[PG_MAX_NODES];                  // a node's first loop entry (2 e + side), -1: none
    short nxt[2 * PG_MAX_LOOPS];             // the next entry of the same node
    short li[PG_MAX_LOOPS], lj[PG_MAX_LOOPS];
    unsigned char act[PG_MAX_LOOPS];
    short on[PG_MAX_LOOPS];                  // the loop edges in force, ascending
    int n_on;
};

__device__ __forceinline__ const bl_posegraph_edge_t& pg_edge(const pg_args& a, int e) { return e < a.N - 1 ? a.chain[e] : a.loops[e - (a.N - 1)]; }

// residuals and chi2 of every edge at `x` into `chi`; full: the blocks and vectors too.  Returns the sum of chi2 over the edges in
// force: they are the terms of the sum, in ascending order with the others left out, so that an edge out of force is an absent one.
__device__ double pg_edges(const pg_args& a, const pg_ws& w, const pg_lds& s, const double* x, double* chi, bool full, double* s_red)
{
    const int E = a.N - 1 + a.L;
    for (int e = threadIdx.x; e < E; e += PG_T) {
        const bl_posegraph_edge_t& ed = pg_edge(a, e);
        const int i = ed.i, j = ed.j;
        double r[3], sn, cs, rx, ry;
        pg_residual(x + 3 * i, x + 3 * j, ed.z, r, &sn, &cs, &rx, &ry);
        pg_s6 om; for (int q = 0; q < 6; ++q) om.a[q] = ed.info[q];
        const pg_m3 Om = pg_full(om);
        double oe[3];
        pg_mv(Om, r, oe);
        const double c2 = pg_dot3(r[0], oe[0], r[1], oe[1], r[2], oe[2]);
        chi[e] = c2;
        if (!full) continue;
        pg_m3 A, B;
        for (int q = 0; q < 9; ++q) { A.a[q] = 0.0; B.a[q] = 0.0; }
        if (i != a.prm.fixed) { A.a[0] = -cs; A.a[1] = -sn; A.a[2] = ry; A.a[3] = sn; A.a[4] = -cs; A.a[5] = -rx; A.a[8] = -1.0; }
        if (j != a.prm.fixed) { B.a[0] = cs; B.a[1] = sn; B.a[3] = -sn; B.a[4] = cs; B.a[8] = 1.0; }
        const pg_m3 At = pg_tr(A), Bt = pg_tr(B);
        const pg_m3 OA = pg_mm(Om, A), OB = pg_mm(Om, B);
        pg_st6(w.AA + 6 * (size_t)e, pg_mm_sym(At, OA));
        pg_st6(w.BB + 6 * (size_t)e, pg_mm_sym(Bt, OB));
        pg_st9(w.AB + 9 * (size_t)e, pg_mm(At, OB));
        pg_mv(At, oe, w.ga + 3 * (size_t)e);
        pg_mv(Bt, oe, w.gb + 3 * (size_t)e);
    }
    __syncthreads();
    double acc = 0.0;
    for (int c = threadIdx.x; c < a.N - 1 + s.n_on; c += PG_T) acc = acc + chi[c < a.N - 1 ? c : a.N - 1 + s.on[c - (a.N - 1)]];
    return pg_sum(acc, s_red);
}

// D_k and g_k: from 0, chain edge k - 1, chain edge k, then the node's loop edges ascending
__device__ void pg_gather(const pg_args& a, const pg_ws& w, const pg_lds& s)
{
    const int N = a.N;
    for (int k = threadIdx.x; k < N; k += PG_T) {
        double d[6], g[3];
        for (int q = 0; q < 6; ++q) d[q] = 0.0;
        for (int q = 0; q < 3; ++q) g[q] = 0.0;
        if (k > 0) {
            for (int q = 0; q < 6; ++q) d[q] = d[q] + w.BB[6 * (size_t)(k - 1) + q];
            for (int q = 0; q < 3; ++q) g[q] = g[q] + w.gb[3 * (size_t)(k - 1) + q];
        }
        if (k < N - 1) {
            for (int q = 0; q < 6; ++q) d[q] = d[q] + w.AA[6 * (size_t)k + q];
            for (int q = 0; q < 3; ++q) g[q] = g[q] + w.ga[3 * (size_t)k + q];
        }
        for (int it = s.head[k]; it >= 0; it = s.nxt[it]) {
            const size_t e = (size_t)(N - 1 + (it >> 1));
            const double* blk = (it & 1) ? w.BB + 6 * e : w.AA + 6 * e;
            const double* vec = (it & 1) ? w.gb + 3 * e : w.ga + 3 * e;
            for (int q = 0; q < 6; ++q) d[q] = d[q] + blk[q];
            for (int q = 0; q < 3; ++q) g[q] = g[q] + vec[q];
        }
        for (int q = 0; q < 6; ++q) w.D[6 * (size_t)k + q] = d[q];
        for (int q = 0; q < 3; ++q) w.g[3 * (size_t)k + q] = g[q];
    }
    __syncthreads();
}

// Dl = D + lambda I (the held node: I), and the block cyclic reduction of the block-tridiagonal (Dl, chain A'Omega B).
// Level s = 1, 2, 4 ... <= N: the nodes e = s - 1 (mod 2 s) are eliminated -- Dw[e] becomes its inverse, Lo[e] the block (e, e - s),
// Up[e] stays the block (e, e + s) -- and the nodes k = 2 s - 1 (mod 2 s) take their Schur complements.
__device__ void pg_factor(const pg_args& a, const pg_ws& w, double lambda)
{
    const int N = a.N;
    for (int k = threadIdx.x; k < N; k += PG_T) {
        pg_s6 d = pg_ld6(w.D + 6 * (size_t)k);
        if (k == a.prm.fixed) { d.a[0] = 1.0; d.a[1] = 0.0; d.a[2] = 1.0; d.a[3] = 0.0; d.a[4] = 0.0; d.a[5] = 1.0; }
        else { d.a[0] = d.a[0] + lambda; d.a[2] = d.a[2] + lambda; d.a[5] = d.a[5] + lambda; }
        pg_st6(w.Dl + 6 * (size_t)k, d);
        pg_st6(w.Dw + 6 * (size_t)k, d);
        if (k < N - 1) pg_st9(w.Up + 9 * (size_t)k, pg_ld9(w.AB + 9 * (size_t)k));
    }
    __syncthreads();
    for (int s = 1; s <= N; s <<= 1) {
        for (int e = s - 1 + 2 * s * (int)threadIdx.x; e < N; e += 2 * s * PG_T) {
            pg_st6(w.Dw + 6 * (size_t)e, pg_inv(pg_ld6(w.Dw + 6 * (size_t)e)));
            if (e - s >= 0) pg_st9(w.Lo + 9 * (size_t)e, pg_tr(pg_ld9(w.Up + 9 * (size_t)(e - s))));
        }
        __syncthreads();
        for (int k = 2 * s - 1 + 2 * s * (int)threadIdx.x; k < N; k += 2 * s * PG_T) {
            const int lo = k - s, hi = k + s;
            pg_s6 d = pg_ld6(w.Dw + 6 * (size_t)k);
            {
                const pg_m3 U = pg_ld9(w.Up + 9 * (size_t)lo);
                const pg_m3 M = pg_mm(pg_tr(U), pg_full(pg_ld6(w.Dw + 6 * (size_t)lo)));
                const pg_s6 S = pg_mm_sym(M, U);
                for (int q = 0; q < 6; ++q) d.a[q] = d.a[q] - S.a[q];
            }
            if (hi < N) {
                const pg_m3 U = pg_ld9(w.Up + 9 * (size_t)k);
                const pg_m3 G = pg_mm(U, pg_full(pg_ld6(w.Dw + 6 * (size_t)hi)));
                const pg_s6 S = pg_mm_sym(G, pg_tr(U));
                for (int q = 0; q < 6; ++q) d.a[q] = d.a[q] - S.a[q];
                if (hi + s < N) {
                    pg_m3 P = pg_mm(G, pg_ld9(w.Up + 9 * (size_t)hi));
                    for (int q = 0; q < 9; ++q) P.a[q] = -P.a[q];
                    pg_st9(w.Up + 9 * (size_t)k, P);
                }
            }
            pg_st6(w.Dw + 6 * (size_t)k, d);
        }
        __syncthreads();
    }
}

// v <- T^-1 v with the factors of pg_factor
__device__ void pg_tsolve(const pg_args& a, const pg_ws& w, double* v)
{
    const int N = a.N;
    int top = 1;
    for (int s = 1; s <= N; s <<= 1) {
        top = s;
        for (int e = s - 1 + 2 * s * (int)threadIdx.x; e < N; e += 2 * s * PG_T) {
            double o[3];
            pg_mv(pg_full(pg_ld6(w.Dw + 6 * (size_t)e)), v + 3 * (size_t)e, o);
            for (int q = 0; q < 3; ++q) v[3 * (size_t)e + q] = o[q];
        }
        __syncthreads();
        for (int k = 2 * s - 1 + 2 * s * (int)threadIdx.x; k < N; k += 2 * s * PG_T) {
            const int lo = k - s, hi = k + s;
            double t[3], vk[3];
            pg_mv(pg_tr(pg_ld9(w.Up + 9 * (size_t)lo)), v + 3 * (size_t)lo, t);
            for (int q = 0; q < 3; ++q) vk[q] = v[3 * (size_t)k + q] - t[q];
            if (hi < N) {
                pg_mv(pg_tr(pg_ld9(w.Lo + 9 * (size_t)hi)), v + 3 * (size_t)hi, t);
                for (int q = 0; q < 3; ++q) vk[q] = vk[q] - t[q];
            }
            for (int q = 0; q < 3; ++q) v[3 * (size_t)k + q] = vk[q];
        }
        __syncthreads();
    }
    for (int s = top; s >= 1; s >>= 1) {
        for (int e = s - 1 + 2 * s * (int)threadIdx.x; e < N; e += 2 * s * PG_T) {
            const bool has_lo = e - s >= 0, has_hi = e + s < N;
            if (!has_lo && !has_hi) continue;
            double t[3], t2[3], o[3];
            if (has_lo) pg_mv(pg_ld9(w.Lo + 9 * (size_t)e), v + 3 * (size_t)(e - s), t);
            if (has_hi) pg_mv(pg_ld9(w.Up + 9 * (size_t)e), v + 3 * (size_t)(e + s), t2);
            if (has_lo && has_hi) { for (int q = 0; q < 3; ++q) t[q] = t[q] + t2[q]; }
            else if (has_hi) { for (int q = 0; q < 3; ++q) t[q] = t2[q]; }
            pg_mv(pg_full(pg_ld6(w.Dw + 6 * (size_t)e)), t, o);
            for (int q = 0; q < 3; ++q) v[3 * (size_t)e + q] = v[3 * (size_t)e + q] - o[q];
        }
        __syncthreads();
    }
}

// hp = H p: Dl_k p_k, + (chain k - 1)' p_{k-1}, + (chain k) p_{k+1}, then the node's loop edges ascending
__device__ void pg_hp(const pg_args& a, const pg_ws& w, const pg_lds& s)
{
    const int N = a.N;
    for (int k = threadIdx.x; k < N; k += PG_T) {
        double o[3], t[3];
        pg_mv(pg_full(pg_ld6(w.Dl + 6 * (size_t)k)), w.p + 3 * (size_t)k, o);
        if (k > 0) {
            pg_mv(pg_tr(pg_ld9(w.AB + 9 * (size_t)(k - 1))), w.p + 3 * (size_t)(k - 1), t);
            for (int q = 0; q < 3; ++q) o[q] = o[q] + t[q];
        }
        if (k < N - 1) {
            pg_mv(pg_ld9(w.AB + 9 * (size_t)k), w.p + 3 * (size_t)(k + 1), t);
            for (int q = 0; q < 3; ++q) o[q] = o[q] + t[q];
        }
        for (int it = s.head[k]; it >= 0; it = s.nxt[it]) {
            const int l = it >> 1;
            const pg_m3 M = pg_ld9(w.AB + 9 * (size_t)(N - 1 + l));
            if (it & 1) pg_mv(pg_tr(M), w.p + 3 * (size_t)s.li[l], t);
            else pg_mv(M, w.p + 3 * (size_t)s.lj[l], t);
            for (int q = 0; q < 3; ++q) o[q] = o[q] + t[q];
        }
        for (int q = 0; q < 3; ++q) w.hp[3 * (size_t)k + q] = o[q];
    }
    __syncthreads();
}

__global__ __launch_bounds__(PG_T) void k_pg_solve(pg_args a)
{
    __shared__ pg_lds s;
    const int tid = threadIdx.x, N = a.N, L = a.L, E = N - 1 + L, sub = blockIdx.x;
    const pg_ws w = pg_ws_of(a.ws + (size_t)sub * a.ws_stride, N, E);
    const unsigned int* mask = a.masks ? a.masks + (size_t)sub * a.words : nullptr;

    // the loop edges in force (mask bit set, information not all zero) and every node's list of them, ascending
    for (int l = tid; l < L; l += PG_T) {
        const bl_posegraph_edge_t& ed = a.loops[l];
        bool on = mask ? ((mask[l >> 5] >> (l & 31)) & 1u) != 0u : true;
        bool any = false;
        for (int q = 0; q < 6; ++q) any = any || ed.info[q] != 0.0;
        s.li[l] = (short)ed.i; s.lj[l] = (short)ed.j; s.act[l] = (on && any) ? 1 : 0;
    }
    for (int k = tid; k < N; k += PG_T) {
        const bl_pose_xyt_t p = a.nodes[k];
        w.x[3 * (size_t)k] = (double)p.x; w.x[3 * (size_t)k + 1] = (double)p.y; w.x[3 * (size_t)k + 2] = (double)p.theta;
    }
    __syncthreads();
    for (int k = tid; k < N; k += PG_T) {
        int prev = -1;
        for (int l = 0; l < L; ++l) {
            if (!s.act[l]) continue;
            int it;
            if (s.li[l] == k) it = 2 * l; else if (s.lj[l] == k) it = 2 * l + 1; else continue;
            if (prev < 0) s.head[k] = it; else s.nxt[prev] = (short)it;
            prev = it;
        }
        if (prev < 0) s.head[k] = -1; else s.nxt[prev] = -1;
    }
    if (tid == 0) {
        int n = 0;
        for (int l = 0; l < L; ++l) if (s.act[l]) s.on[n++] = (short)l;
        s.n_on = n;
    }
    __syncthreads();

    double F = pg_edges(a, w, s, w.x, w.chi, true, s.red);
    for (int e = tid; e < E; e += PG_T) w.chi0[e] = w.chi[e];
    const double F0 = F;
    pg_gather(a, w, s);

    double lambda = a.prm.lambda0;
    int tries = 0, accepted = 0, cg_total = 0, status = BL_POSEGRAPH_OUT_OF_TRIES, cap = 0;
    while (tries < a.prm.max_tries) {
        ++tries;
        pg_factor(a, w, lambda);
        // conjugate gradients on H dx = -g, preconditioned by T
        for (int q = tid; q < 3 * N; q += PG_T) { const double b = -w.g[q]; w.r[q] = b; w.z[q] = b; w.dx[q] = 0.0; }
        __syncthreads();
        pg_tsolve(a, w, w.z);
        for (int q = tid; q < 3 * N; q += PG_T) w.p[q] = w.z[q];
        __syncthreads();
        double rz = pg_dot(w.r, w.z, N, s.red);
        const double rz0 = rz, tol = (a.prm.cg_tol * a.prm.cg_tol) * rz0;
        int it = 0;
        bool done = !(rz0 > 0.0);
        while (!done && it < a.prm.max_cg) {
            pg_hp(a, w, s);
            const double php = pg_dot(w.p, w.hp, N, s.red);
            if (!(php > 0.0)) break;
            const double al = rz / php;
            for (int q = tid; q < 3 * N; q += PG_T) {
                w.dx[q] = w.dx[q] + al * w.p[q];
                const double rq = w.r[q] - al * w.hp[q];
                w.r[q] = rq; w.z[q] = rq;
            }
            __syncthreads();
            pg_tsolve(a, w, w.z);
            const double rz2 = pg_dot(w.r, w.z, N, s.red);
            ++it;
            if (rz2 <= tol) { done = true; break; }
            const double beta = rz2 / rz;
            for (int q = tid; q < 3 * N; q += PG_T) w.p[q] = w.z[q] + beta * w.p[q];
            __syncthreads();
            rz = rz2;
        }
        cg_total += it;
        if (!done) cap = 1;
        if (rz0 == 0.0) { status = BL_POSEGRAPH_CONVERGED_STEP; break; }          // no gradient: the step is zero

        // the trial poses and their cost
        double md = 0.0;
        for (int k = tid; k < N; k += PG_T) {
            const size_t q = 3 * (size_t)k;
            if (k == a.prm.fixed) { w.xn[q] = w.x[q]; w.xn[q + 1] = w.x[q + 1]; w.xn[q + 2] = w.x[q + 2]; continue; }
            w.xn[q] = w.x[q] + w.dx[q];
            w.xn[q + 1] = w.x[q + 1] + w.dx[q + 1];
            w.xn[q + 2] = pg_wrap(w.x[q + 2] + w.dx[q + 2]);
            md = fmax(md, fmax(fabs(w.dx[q]), fmax(fabs(w.dx[q + 1]), fabs(w.dx[q + 2]))));
        }
        __syncthreads();
        md = pg_max(md, s.red);
        const double F2 = pg_edges(a, w, s, w.xn, w.chin, false, s.red);
        if (F2 < F) {
            ++accepted;
            for (int q = tid; q < 3 * N; q += PG_T) w.x[q] = w.xn[q];
            __syncthreads();
            const double Fold = F;
            F = pg_edges(a, w, s, w.x, w.chi, true, s.red);
            pg_gather(a, w, s);
            if (md <= a.prm.step_tol) { status = BL_POSEGRAPH_CONVERGED_STEP; break; }
            if (Fold - F <= a.prm.rel_tol * Fold) { status = BL_POSEGRAPH_CONVERGED_DECREASE; break; }
            lambda = lambda * a.prm.lambda_down;
        } else {
            lambda = lambda * a.prm.lambda_up;
        }
    }

    // the poses narrowed once, utime carried through
    for (int k = tid; k < N; k += PG_T) {
        bl_pose_xyt_t p = a.nodes[k];
        p.x = (float)w.x[3 * (size_t)k]; p.y = (float)w.x[3 * (size_t)k + 1]; p.theta = (float)w.x[3 * (size_t)k + 2];
        a.out[(size_t)sub * a.out_stride + k] = p;
    }
    if (tid == 0) {
        bl_posegraph_result_t r;
        r.cost_before = F0; r.cost_after = F; r.final_lambda = lambda;
        r.tries = tries; r.accepted = accepted; r.cg_iterations = cg_total;
        r.status = status | (cap ? BL_POSEGRAPH_CG_CAP : 0);
        a.results[sub] = r;
    }
}

// z_k = pose k + 1 seen from pose k, by the residual's statements with z = 0
__global__ void k_pg_chain_from_nodes(const bl_pose_xyt_t* nodes, int N, bl_posegraph_edge_t* chain, bl_posegraph_edge_t info)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= N - 1) return;
    const bl_pose_xyt_t pi = nodes[k], pj = nodes[k + 1];
    const double xi[3] = {(double)pi.x, (double)pi.y, (double)pi.theta}, xj[3] = {(double)pj.x, (double)pj.y, (double)pj.theta};
    const double zero[3] = {0.0, 0.0, 0.0};
    double e[3], sn, cs, rx, ry;
    pg_residual(xi, xj, zero, e, &sn, &cs, &rx, &ry);
    bl_posegraph_edge_t ed = info;
    ed.i = k; ed.j = k + 1;
    ed.z[0] = e[0]; ed.z[1] = e[1]; ed.z[2] = e[2];
    chain[k] = ed;
}

// ---------------------------------------------------------------- host
static size_t pg_ws_doubles(int N, int E) { return (size_t)PG_NODE_DOUBLES * N + (size_t)PG_EDGE_DOUBLES * E; }

extern "C" int bl_posegraph_create(bl_ctx* ctx, int max_nodes, int max_loop_edges, int max_subsets, bl_posegraph** out)
{
    BL_CHECK_ARG(out != nullptr && ctx != nullptr);
    BL_CHECK_ARG(max_nodes >= 2 && max_nodes <= PG_MAX_NODES);
    BL_CHECK_ARG(max_loop_edges >= 0 && max_loop_edges <= PG_MAX_LOOPS);
    BL_CHECK_ARG(max_subsets >= 1 && max_subsets <= 65536);
    const int E = max_nodes - 1 + max_loop_edges;
    const size_t ws_stride = pg_ws_doubles(max_nodes, E);
    const unsigned long long bytes = (unsigned long long)max_subsets * (ws_stride * 8ull + (unsigned long long)max_nodes * sizeof(bl_pose_xyt_t) + 128ull + sizeof(bl_posegraph_result_t))
                                     + (unsigned long long)max_nodes * sizeof(bl_pose_xyt_t) + (unsigned long long)E * sizeof(bl_posegraph_edge_t);
    BL_CHECK_ARG(bytes <= PG_MAX_BYTES);
    BL_HIP(hipSetDevice(ctx->device));
    bl_posegraph* g = new bl_posegraph();
    memset(g, 0, sizeof(*g));
    g->ctx = ctx; g->max_nodes = max_nodes; g->max_loops = max_loop_edges; g->max_subsets = max_subsets; g->ws_stride = ws_stride;
    hipError_t e = hipMalloc((void**)&g->d_nodes, (size_t)max_nodes * sizeof(bl_pose_xyt_t));
    if (e == hipSuccess) e = hipMalloc((void**)&g->d_edges, (size_t)E * sizeof(bl_posegraph_edge_t));
    if (e == hipSuccess) e = hipMalloc((void**)&g->d_masks, (size_t)max_subsets * 32 * sizeof(unsigned int));
    if (e == hipSuccess) e = hipMalloc((void**)&g->d_ws, (size_t)max_subsets * ws_stride * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&g->d_out, (size_t)max_subsets * max_nodes * sizeof(bl_pose_xyt_t));
    if (e == hipSuccess) e = hipMalloc((void**)&g->d_results, (size_t)max_subsets * sizeof(bl_posegraph_result_t));
    for (int i = 0; i < 2 && e == hipSuccess; ++i) e = hipEventCreate(&g->ev[i]);
    if (e != hipSuccess) { bl_set_error("bl_posegraph_create: %s", hipGetErrorString(e)); bl_posegraph_destroy(g); return BL_ERR_HIP; }
    *out = g;
    return BL_OK;
}

extern "C" void bl_posegraph_destroy(bl_posegraph* g)
{
    if (!g) return;
    (void)hipStreamSynchronize(g->ctx->stream);
    void* bufs[] = {g->d_nodes, g->d_edges, g->d_masks, g->d_ws, g->d_out, g->d_results};
    for (void* b : bufs) if (b) (void)hipFree(b);
    for (int i = 0; i < 2; ++i) if (g->ev[i]) (void)hipEventDestroy(g->ev[i]);
    delete g;
}

static void pg_new_nodes(bl_posegraph* g, int n) { g->n = n; g->have_chain = false; g->n_loops = 0; }

extern "C" int bl_posegraph_set_nodes(bl_posegraph* g, int n, const bl_pose_xyt_t* poses)
{
    BL_CHECK_ARG(g != nullptr && poses != nullptr);
    BL_CHECK_ARG(n >= 2 && n <= g->max_nodes);
    BL_HIP(hipSetDevice(g->ctx->device));
    BL_HIP(hipMemcpyAsync(g->d_nodes, poses, (size_t)n * sizeof(bl_pose_xyt_t), hipMemcpyHostToDevice, g->ctx->stream));
    BL_HIP(hipStreamSynchronize(g->ctx->stream));              // the host array is the caller's and may be reused at once
    pg_new_nodes(g, n);
    return BL_OK;
}

// entries first .. first + count - 1 of a log lie in at most two runs of slots
template <class F>
static int pg_log_runs(const bl_scanlog_view& v, int first, int count, F f)
{
    const int s0 = (v.head + first) % v.capacity;
    const int n0 = count < v.capacity - s0 ? count : v.capacity - s0;
    int rc = f(s0, 0, n0);
    if (!rc && n0 < count) rc = f(0, n0, count - n0);
    return rc;
}

extern "C" int bl_posegraph_set_nodes_from_log(bl_posegraph* g, bl_scanlog* log, int first, int count)
{
    BL_CHECK_ARG(g != nullptr && log != nullptr);
    bl_scanlog_view v;
    bl_scanlog_view_host(log, &v);
    BL_CHECK_ARG(v.ctx == g->ctx);
    BL_CHECK_ARG(first >= 0 && count >= 2 && count <= g->max_nodes && first <= v.size && count <= v.size - first);
    BL_HIP(hipSetDevice(g->ctx->device));
    const int rc = pg_log_runs(v, first, count, [&](int slot, int at, int n) -> int {
        BL_HIP(hipMemcpyAsync(g->d_nodes + at, v.d_poses + slot, (size_t)n * sizeof(bl_pose_xyt_t), hipMemcpyDeviceToDevice, g->ctx->stream));
        return BL_OK;
    });
    if (rc) return rc;
    pg_new_nodes(g, count);
    return BL_OK;
}

static bool pg_edge_finite(const bl_posegraph_edge_t& e)
{
    for (int q = 0; q < 3; ++q) if (!(e.z[q] - e.z[q] == 0.0)) return false;
    for (int q = 0; q < 6; ++q) if (!(e.info[q] - e.info[q] == 0.0)) return false;
    return true;
}

extern "C" int bl_posegraph_set_chain(bl_posegraph* g, const bl_posegraph_edge_t* edges)
{
    BL_CHECK_ARG(g != nullptr && edges != nullptr);
    if (g->n < 2) { bl_set_error("bl_posegraph_set_chain: no nodes yet"); return BL_ERR_STATE; }
    for (int k = 0; k < g->n - 1; ++k) BL_CHECK_ARG(edges[k].i == k && edges[k].j == k + 1 && pg_edge_finite(edges[k]));
    BL_HIP(hipSetDevice(g->ctx->device));
    BL_HIP(hipMemcpyAsync(g->d_edges, edges, (size_t)(g->n - 1) * sizeof(bl_posegraph_edge_t), hipMemcpyHostToDevice, g->ctx->stream));
    BL_HIP(hipStreamSynchronize(g->ctx->stream));
    g->have_chain = true;
    return BL_OK;
}

extern "C" int bl_posegraph_set_chain_from_nodes(bl_posegraph* g, const double* info6)
{
    BL_CHECK_ARG(g != nullptr && info6 != nullptr);
    if (g->n < 2) { bl_set_error("bl_posegraph_set_chain_from_nodes: no nodes yet"); return BL_ERR_STATE; }
    bl_posegraph_edge_t info;
    memset(&info, 0, sizeof(info));
    for (int q = 0; q < 6; ++q) info.info[q] = info6[q];
    BL_CHECK_ARG(pg_edge_finite(info));
    BL_HIP(hipSetDevice(g->ctx->device));
    hipLaunchKernelGGL(k_pg_chain_from_nodes, dim3((g->n - 1 + 255) / 256), dim3(256), 0, g->ctx->stream, (const bl_pose_xyt_t*)g->d_nodes, g->n, g->d_edges, info);
    BL_HIP(hipGetLastError());
    g->have_chain = true;
    return BL_OK;
}

extern "C" int bl_posegraph_set_loops(bl_posegraph* g, int n, const bl_posegraph_edge_t* edges)
{
    BL_CHECK_ARG(g != nullptr && n >= 0 && n <= g->max_loops && (n == 0 || edges != nullptr));
    if (g->n < 2) { bl_set_error("bl_posegraph_set_loops: no nodes yet"); return BL_ERR_STATE; }
    for (int l = 0; l < n; ++l)
        BL_CHECK_ARG(edges[l].i >= 0 && edges[l].i < g->n && edges[l].j >= 0 && edges[l].j < g->n && edges[l].i != edges[l].j && pg_edge_finite(edges[l]));
    BL_HIP(hipSetDevice(g->ctx->device));
    if (n > 0) {
        BL_HIP(hipMemcpyAsync(g->d_edges + (g->max_nodes - 1), edges, (size_t)n * sizeof(bl_posegraph_edge_t), hipMemcpyHostToDevice, g->ctx->stream));
        BL_HIP(hipStreamSynchronize(g->ctx->stream));
    }
    g->n_loops = n;
    return BL_OK;
}

extern "C" int bl_posegraph_solve(bl_posegraph* g, const bl_posegraph_params_t* prm, int n_subsets, const uint32_t* masks)
{
    BL_CHECK_ARG(g != nullptr && prm != nullptr);
    BL_CHECK_ARG(n_subsets >= 1 && n_subsets <= g->max_subsets && (masks != nullptr || n_subsets == 1));
    if (g->n < 2 || !g->have_chain) { bl_set_error("bl_posegraph_solve: nodes and chain first"); return BL_ERR_STATE; }
    BL_CHECK_ARG(prm->fixed >= 0 && prm->fixed < g->n && prm->max_tries >= 1 && prm->max_cg >= 1);
    BL_CHECK_ARG(prm->lambda0 >= 0.0 && prm->lambda0 < 1e300 && prm->lambda_up > 1.0 && prm->lambda_up < 1e300 && prm->lambda_down > 0.0 && prm->lambda_down <= 1.0);
    BL_CHECK_ARG(prm->step_tol >= 0.0 && prm->rel_tol >= 0.0 && prm->cg_tol >= 0.0 && prm->step_tol < 1e300 && prm->rel_tol < 1e300 && prm->cg_tol < 1e150);
    bl_ctx* ctx = g->ctx;
    BL_HIP(hipSetDevice(ctx->device));
    pg_args a;
    memset(&a, 0, sizeof(a));
    a.N = g->n; a.L = g->n_loops; a.words = (g->n_loops + 31) / 32;
    a.prm = *prm;
    a.nodes = g->d_nodes; a.chain = g->d_edges; a.loops = g->d_edges + (g->max_nodes - 1);
    a.ws = g->d_ws; a.ws_stride = g->ws_stride;
    a.out = g->d_out; a.out_stride = g->max_nodes;
    a.results = g->d_results;
    if (masks && a.words > 0) {
        BL_HIP(hipMemcpyAsync(g->d_masks, masks, (size_t)n_subsets * a.words * sizeof(unsigned int), hipMemcpyHostToDevice, ctx->stream));
        BL_HIP(hipStreamSynchronize(ctx->stream));
        a.masks = g->d_masks;
    }
    BL_HIP(hipEventRecord(g->ev[0], ctx->stream));
    hipLaunchKernelGGL(k_pg_solve, dim3(n_subsets), dim3(PG_T), 0, ctx->stream, a);
    BL_HIP(hipGetLastError());
    BL_HIP(hipEventRecord(g->ev[1], ctx->stream));
    g->solved = n_subsets; g->solved_n = g->n; g->solved_edges = g->n - 1 + g->n_loops;
    return BL_OK;
}

static int pg_need_solve(const bl_posegraph* g, int subset, const char* who)
{
    if (g->solved < 1) { bl_set_error("%s: no solve yet", who); return BL_ERR_STATE; }
    BL_CHECK_ARG(subset >= 0 && subset < g->solved);
    return BL_OK;
}

extern "C" int bl_posegraph_results(bl_posegraph* g, bl_posegraph_result_t* results)
{
    BL_CHECK_ARG(g != nullptr && results != nullptr);
    const int rc = pg_need_solve(g, 0, "bl_posegraph_results");
    if (rc) return rc;
    BL_HIP(hipSetDevice(g->ctx->device));
    BL_HIP(hipMemcpyAsync(results, g->d_results, (size_t)g->solved * sizeof(bl_posegraph_result_t), hipMemcpyDeviceToHost, g->ctx->stream));
    BL_HIP(hipStreamSynchronize(g->ctx->stream));
    return BL_OK;
}

extern "C" int bl_posegraph_poses(bl_posegraph* g, int subset, bl_pose_xyt_t* out_xyt, double* out_double)
{
    BL_CHECK_ARG(g != nullptr && (out_xyt != nullptr || out_double != nullptr));
    const int rc = pg_need_solve(g, subset, "bl_posegraph_poses");
    if (rc) return rc;
    BL_HIP(hipSetDevice(g->ctx->device));
    if (out_xyt) BL_HIP(hipMemcpyAsync(out_xyt, g->d_out + (size_t)subset * g->max_nodes, (size_t)g->solved_n * sizeof(bl_pose_xyt_t), hipMemcpyDeviceToHost, g->ctx->stream));
    if (out_double) {
        const pg_ws w = pg_ws_of(g->d_ws + (size_t)subset * g->ws_stride, g->solved_n, g->solved_edges);
        BL_HIP(hipMemcpyAsync(out_double, w.x, (size_t)g->solved_n * 3 * sizeof(double), hipMemcpyDeviceToHost, g->ctx->stream));
    }
    BL_HIP(hipStreamSynchronize(g->ctx->stream));
    return BL_OK;
}

extern "C" int bl_posegraph_edge_chi2(bl_posegraph* g, int subset, double* before, double* after)
{
    BL_CHECK_ARG(g != nullptr && (before != nullptr || after != nullptr));
    const int rc = pg_need_solve(g, subset, "bl_posegraph_edge_chi2");
    if (rc) return rc;
    BL_HIP(hipSetDevice(g->ctx->device));
    const pg_ws w = pg_ws_of(g->d_ws + (size_t)subset * g->ws_stride, g->solved_n, g->solved_edges);
    if (before) BL_HIP(hipMemcpyAsync(before, w.chi0, (size_t)g->solved_edges * sizeof(double), hipMemcpyDeviceToHost, g->ctx->stream));
    if (after) BL_HIP(hipMemcpyAsync(after, w.chi, (size_t)g->solved_edges * sizeof(double), hipMemcpyDeviceToHost, g->ctx->stream));
    BL_HIP(hipStreamSynchronize(g->ctx->stream));
    return BL_OK;
}

extern "C" int bl_posegraph_poses_to_log(bl_posegraph* g, int subset, bl_scanlog* log, int first)
{
    BL_CHECK_ARG(g != nullptr && log != nullptr);
    const int rc0 = pg_need_solve(g, subset, "bl_posegraph_poses_to_log");
    if (rc0) return rc0;
    bl_scanlog_view v;
    bl_scanlog_view_host(log, &v);
    BL_CHECK_ARG(v.ctx == g->ctx);
    const int count = g->solved_n;
    BL_CHECK_ARG(first >= 0 && first <= v.size && count <= v.size - first);
    BL_HIP(hipSetDevice(g->ctx->device));
    const bl_pose_xyt_t* src = g->d_out + (size_t)subset * g->max_nodes;
    return pg_log_runs(v, first, count, [&](int slot, int at, int n) -> int {
        BL_HIP(hipMemcpyAsync(v.d_poses + slot, src + at, (size_t)n * sizeof(bl_pose_xyt_t), hipMemcpyDeviceToDevice, g->ctx->stream));
        return BL_OK;
    });
}

extern "C" int bl_posegraph_last_device_ms(bl_posegraph* g, float* ms)
{
    BL_CHECK_ARG(g != nullptr && ms != nullptr);
    if (g->solved < 1) { bl_set_error("bl_posegraph_last_device_ms: no solve yet"); return BL_ERR_STATE; }
    BL_HIP(hipSetDevice(g->ctx->device));
    BL_HIP(hipEventSynchronize(g->ev[1]));
    BL_HIP(hipEventElapsedTime(ms, g->ev[0], g->ev[1]));
    return BL_OK;
}
