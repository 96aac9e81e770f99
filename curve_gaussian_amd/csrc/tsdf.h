// THE RULE of the distance field and of its surface (include/curvegs.h, cgs_tsdf_integrate / cgs_tsdf_mesh_count /
// cgs_tsdf_mesh_emit), stated once for the kernels of tsdf.hip and the probe beside profiles/tsdf_mesh.md.  float64, one
// rounded operation at a time in the written order, nothing contracted, IEEE division, running sums in view order, 64-bit
// offsets.
//
// LATTICE.  The lattice points are the voxel centres of a SeedGrid, by seed_centre (seed_centre.h), the point the edge vote
// projects.  A cell is the cube between 8 neighbouring lattice points; cell (i, j, k), 0 <= i < nx - 1 and so on, has the
// linear index i + (nx - 1) (j + (ny - 1) k) and its corner c = dx + 2 dy + 4 dz is the lattice point (i + dx, j + dy,
// k + dz).  A corner's number grows with its linear lattice index.
//
// INTEGRATION (tsdf_observe): one view's word on one lattice point, the views in order.
//   the view keeps the point by nv_project_xyz_depth (c2 > 0, 0 <= u < W, 0 <= v < H); otherwise nothing
//   d = (double)plane[floor(v)][floor(u)], the pixel nv_hidden reads; nothing unless d > 0 && d < +inf
//   sdf = d - c2; nothing if sdf < -trunc; nothing if weight == 65535 already (the weight SATURATES: the pair stays a mean)
//   t = sdf / trunc; t = 1.0 if t > 1.0; sum += t; weight += 1
//
// EXTRACTION (tsdf_cell): marching tetrahedra.
//   A cell is live iff all 8 corners have weight >= min_weight (>= 1).  f = sum / (double)weight; a corner is INSIDE iff
//   f < 0 (0.0, -0.0 and a NaN are outside).
//   The cube is cut into the 6 Kuhn tetrahedra around the diagonal corner 0 -- corner 7: tetrahedron t = 0..5 belongs to
//   the t-th order (a, b, c) of the axes 0, 1, 2 in lexicographic order and has the corners (q0, q1, q2, q3) =
//   (0, 1 << a, (1 << a) | (1 << b), 7), ascending.  Its parity is that of the order: t = 0, 3, 4 even, t = 1, 2, 5 odd.
//   The inside mask m has bit x set iff q_x is inside.  E(x, y) is the vertex on the lattice edge q_x -- q_y.
//     one inside corner x, the others p < q < r:        (E(x,p), E(x,q), E(x,r)), turned iff x is odd
//     one outside corner x, the others p < q < r:       the same triangle, turned iff x is even
//     inside i < j, outside k < l: the quad E(i,k) E(i,l) E(j,l) E(j,k) split along E(i,k) -- E(j,l):
//                                  (E(i,k), E(i,l), E(j,l)) then (E(i,k), E(j,l), E(j,k)), both turned iff (i, j, k, l)
//                                  is an odd permutation
//   "turned" swaps the second and third vertex; a tetrahedron of odd parity turns every triangle once more.  WINDING: with
//   that, (v1 - v0) x (v2 - v0) points from inside to outside -- in the even tetrahedron 0 with corner 0 alone inside the
//   triangle on the three axes has the normal (1, 1, 1), and every other case is that one under a relabelling of the
//   corners, which mirrors the tetrahedron iff the relabelling is odd.
//   tsdf_case derives the 16 cases from these sentences at compile time; no table is written out.
//   VERTEX E(x, y): the ends in ascending linear lattice index (a, b) -- ascending corner number -- whatever their signs:
//   p = Pa + (fa / (fa - fb)) * (Pb - Pa) per component in float64, rounded to float32.  Two cells that share the edge
//   compute the same bits.
//   ORDER: by cell, then tetrahedron, then triangle.  Every triangle is emitted, those with equal vertices too.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "point_projection.h"
#include "seed_centre.h"

namespace cgs {

constexpr unsigned int TSDF_MAX_WEIGHT = 65535u;
constexpr int TSDF_CELL_MAX_TRIS = 12;

__device__ inline void tsdf_observe(const NvCam& c, double X, double Y, double Z, double wd, double hd,
                                    const float* __restrict__ plane, int width, double trunc, double& sum,
                                    unsigned int& weight) {
#pragma clang fp contract(off)
    double u, v, c2;
    if (!nv_project_xyz_depth(c, X, Y, Z, wd, hd, u, v, c2)) return;
    // 0 <= u < W and 0 <= v < H: the pixel is inside the plane
    const double d = (double)plane[(size_t)floor(v) * (size_t)width + (size_t)floor(u)];
    if (!(d > 0.0 && d < (double)INFINITY)) return;   // a NaN fails both
    const double sdf = d - c2;
    if (sdf < -trunc) return;
    if (weight >= TSDF_MAX_WEIGHT) return;
    double t = sdf / trunc;
    if (t > 1.0) t = 1.0;
    sum += t;
    weight += 1u;
}

// ---- the 16 cases of a tetrahedron of even parity, derived.  A vertex is 4 bits, lo | hi << 2 with lo < hi the ends'
// places among (q0, q1, q2, q3); a triangle is 12 bits, v0 | v1 << 4 | v2 << 8; a case is triangle 0 | triangle 1 << 12 |
// the number of triangles << 24.
constexpr unsigned int tsdf_edge(int x, int y) { return x < y ? (unsigned)(x | (y << 2)) : (unsigned)(y | (x << 2)); }
constexpr unsigned int tsdf_tri(unsigned int a, unsigned int b, unsigned int c, bool turned) {
    return turned ? (a | (c << 4) | (b << 8)) : (a | (b << 4) | (c << 8));
}
constexpr unsigned int tsdf_case(int m) {
    int in[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0};
    int ni = 0, no = 0;
    for (int x = 0; x < 4; x++) {
        if ((m >> x) & 1) in[ni++] = x;
        else out[no++] = x;
    }
    if (ni == 0 || ni == 4) return 0u;
    if (ni == 1) return tsdf_tri(tsdf_edge(in[0], out[0]), tsdf_edge(in[0], out[1]), tsdf_edge(in[0], out[2]), in[0] % 2 == 1) | (1u << 24);
    if (ni == 3) return tsdf_tri(tsdf_edge(out[0], in[0]), tsdf_edge(out[0], in[1]), tsdf_edge(out[0], in[2]), out[0] % 2 == 0) | (1u << 24);
    const int p[4] = {in[0], in[1], out[0], out[1]};
    int inversions = 0;
    for (int x = 0; x < 4; x++)
        for (int y = x + 1; y < 4; y++) inversions += p[x] > p[y] ? 1 : 0;
    const bool turned = inversions % 2 == 1;
    const unsigned int A = tsdf_edge(p[0], p[2]), B = tsdf_edge(p[0], p[3]), C = tsdf_edge(p[1], p[3]), D = tsdf_edge(p[1], p[2]);
    return tsdf_tri(A, B, C, turned) | (tsdf_tri(A, C, D, turned) << 12) | (2u << 24);
}
struct TsdfCases {
    unsigned int w[16];
};
constexpr TsdfCases tsdf_make_cases() {
    TsdfCases t = {};
    for (int m = 0; m < 16; m++) t.w[m] = tsdf_case(m);
    return t;
}
static __constant__ const TsdfCases c_tsdf_cases = tsdf_make_cases();

// tetrahedron t: its second and third corner (the first is 0, the last 7) and whether its parity is odd
constexpr int tsdf_tet_axis_a(int t) { return t / 2; }
constexpr int tsdf_tet_axis_b(int t) { return t % 2 == 0 ? (t / 2 == 0 ? 1 : 0) : (t / 2 == 2 ? 1 : 2); }
constexpr int tsdf_tet_q1(int t) { return 1 << tsdf_tet_axis_a(t); }
constexpr int tsdf_tet_q2(int t) { return (1 << tsdf_tet_axis_a(t)) | (1 << tsdf_tet_axis_b(t)); }
constexpr bool tsdf_tet_odd(int t) {
    const int a = tsdf_tet_axis_a(t), b = tsdf_tet_axis_b(t), c = 3 - a - b;
    return ((a > b ? 1 : 0) + (a > c ? 1 : 0) + (b > c ? 1 : 0)) % 2 == 1;
}

template <class T>
__device__ __forceinline__ T tsdf_sel4(T a0, T a1, T a2, T a3, unsigned int x) {
    return x == 0u ? a0 : x == 1u ? a1 : x == 2u ? a2 : a3;
}

// One tetrahedron of a live cell.  f: the 8 corner values; (xs, ys, zs): the lattice coordinates of the cell's two
// ends per axis.  Returns the number of its triangles; EMIT writes them to out (9 floats each).
template <int T, bool EMIT>
__device__ __forceinline__ int tsdf_tet(const double (&f)[8], const double (&xs)[2], const double (&ys)[2], const double (&zs)[2],
                                        float* __restrict__ out) {
#pragma clang fp contract(off)
    constexpr int Q1 = tsdf_tet_q1(T), Q2 = tsdf_tet_q2(T);
    constexpr bool ODD = tsdf_tet_odd(T);
    const double g0 = f[0], g1 = f[Q1], g2 = f[Q2], g3 = f[7];
    const unsigned int m = (g0 < 0.0 ? 1u : 0u) | (g1 < 0.0 ? 2u : 0u) | (g2 < 0.0 ? 4u : 0u) | (g3 < 0.0 ? 8u : 0u);
    const unsigned int word = c_tsdf_cases.w[m];
    const int n = (int)(word >> 24);
    if (EMIT) {
        for (int r = 0; r < n; r++) {
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const int slot = ODD ? (k == 0 ? 0 : 3 - k) : k;   // a tetrahedron of odd parity turns the triangle
                const unsigned int code = (word >> (12 * r + 4 * slot)) & 15u;
                const unsigned int a = code & 3u, b = code >> 2;   // a < b: ascending corner number
                const double fa = tsdf_sel4(g0, g1, g2, g3, a), fb = tsdf_sel4(g0, g1, g2, g3, b);
                const unsigned int ca = tsdf_sel4(0u, (unsigned)Q1, (unsigned)Q2, 7u, a);
                const unsigned int cb = tsdf_sel4(0u, (unsigned)Q1, (unsigned)Q2, 7u, b);
                const double w = fa / (fa - fb);
                const double ax = (ca & 1u) ? xs[1] : xs[0], bx = (cb & 1u) ? xs[1] : xs[0];
                const double ay = (ca & 2u) ? ys[1] : ys[0], by = (cb & 2u) ? ys[1] : ys[0];
                const double az = (ca & 4u) ? zs[1] : zs[0], bz = (cb & 4u) ? zs[1] : zs[0];
                out[9 * r + 3 * k + 0] = (float)(ax + w * (bx - ax));
                out[9 * r + 3 * k + 1] = (float)(ay + w * (by - ay));
                out[9 * r + 3 * k + 2] = (float)(az + w * (bz - az));
            }
        }
    }
    return n;
}

// Cell `cell` of the grid: the number of its triangles (0 when it is not live).  EMIT: written to `out` in the rule's order
// when the range offset .. offset + n lies inside [0, T]; nothing is written otherwise.
template <bool EMIT>
__device__ inline int tsdf_cell(const SeedGrid& g, const double* __restrict__ sum, const unsigned short* __restrict__ weight,
                                unsigned int min_weight, long long cell, long long offset, long long T,
                                float* __restrict__ tris) {
#pragma clang fp contract(off)
    const int cx = g.nx - 1, cy = g.ny - 1;
    const int i = (int)(cell % cx);
    const long long rest = cell / cx;
    const int j = (int)(rest % cy), k = (int)(rest / cy);
    const long long base = (long long)i + (long long)g.nx * ((long long)j + (long long)g.ny * (long long)k);
    double f[8];
    bool live = true;
#pragma unroll
    for (int c = 0; c < 8; c++) {
        const long long id = base + (c & 1) + (long long)g.nx * (((c >> 1) & 1) + (long long)g.ny * (c >> 2));
        const unsigned int w = weight[id];
        live = live && w >= min_weight;
        f[c] = sum[id] / (double)w;
    }
    if (!live) return 0;
    double xs[2] = {0.0, 0.0}, ys[2] = {0.0, 0.0}, zs[2] = {0.0, 0.0};
    if (EMIT) {
        seed_centre(g, base, xs[0], ys[0], zs[0]);
        seed_centre(g, base + 1 + (long long)g.nx * (1 + (long long)g.ny), xs[1], ys[1], zs[1]);
    }
    if (EMIT) {
        // the count first: the cell writes all of its triangles or none
        const int n = tsdf_tet<0, false>(f, xs, ys, zs, nullptr) + tsdf_tet<1, false>(f, xs, ys, zs, nullptr) +
                      tsdf_tet<2, false>(f, xs, ys, zs, nullptr) + tsdf_tet<3, false>(f, xs, ys, zs, nullptr) +
                      tsdf_tet<4, false>(f, xs, ys, zs, nullptr) + tsdf_tet<5, false>(f, xs, ys, zs, nullptr);
        if (n == 0 || offset < 0 || offset > T || (long long)n > T - offset) return n;
    }
    float* out = EMIT ? tris + 9 * offset : nullptr;
    int n = 0;
    n += tsdf_tet<0, EMIT>(f, xs, ys, zs, out);
    n += tsdf_tet<1, EMIT>(f, xs, ys, zs, EMIT ? out + 9 * n : nullptr);
    n += tsdf_tet<2, EMIT>(f, xs, ys, zs, EMIT ? out + 9 * n : nullptr);
    n += tsdf_tet<3, EMIT>(f, xs, ys, zs, EMIT ? out + 9 * n : nullptr);
    n += tsdf_tet<4, EMIT>(f, xs, ys, zs, EMIT ? out + 9 * n : nullptr);
    n += tsdf_tet<5, EMIT>(f, xs, ys, zs, EMIT ? out + 9 * n : nullptr);
    return n;
}

}  // namespace cgs
