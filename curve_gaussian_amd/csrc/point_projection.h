// The pinhole projection of a world point into a camera, shared by every kernel that must agree on which points a view
// keeps (novel_view.hip: cgs_project_points / cgs_render_points; edge_score.hip: cgs_point_mask; edge_seed.hip:
// cgs_voxel_votes, cgs_ray_claims and cgs_ray_wins -- k_voxel_votes, k_ray_claims, k_ray_wins through seed_walk;
// edge_support.hip: cgs_edge_support; edge_trim.hip: cgs_sample_support; edge_orient.hip: cgs_sample_support_oriented;
// edge_snap.hip: cgs_sample_snap_terms).
//
// Exact, the reference's operation order (eval_ABC.py project_points_to_camera :66-81): X float32 widened to float64,
// c = R X + T with every row ((r0*X + r1*Y) + r2*Z) + t, dropped if c2 <= 0 (a NaN depth is dropped too: it fails the
// image test), then u = fx * (c0 / c2) + cx, v = fy * (c1 / c2) + cy, kept if 0 <= u < W and 0 <= v < H.  Contraction into
// FMAs is off and divisions are IEEE, as in visibility.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace cgs {

struct NvCam {
    double m[12];   // [R | T], row-major 3x4
    double f[4];    // fx, fy, cx, cy
};

__device__ inline void nv_load_cam(NvCam& c, const double* __restrict__ intr, const double* __restrict__ w2c, int v) {
#pragma unroll
    for (int k = 0; k < 12; k++) c.m[k] = w2c[12 * (size_t)v + k];
#pragma unroll
    for (int k = 0; k < 4; k++) c.f[k] = intr[4 * (size_t)v + k];
}

// True if the point is kept; (u, v) as the reference computes them.  (X, Y, Z): a float32 point widened to float64.
__device__ inline bool nv_project_xyz(const NvCam& c, double X, double Y, double Z, double wd, double hd, double& u,
                                      double& v) {
#pragma clang fp contract(off)
    const double c0 = ((c.m[0] * X + c.m[1] * Y) + c.m[2] * Z) + c.m[3];
    const double c1 = ((c.m[4] * X + c.m[5] * Y) + c.m[6] * Z) + c.m[7];
    const double c2 = ((c.m[8] * X + c.m[9] * Y) + c.m[10] * Z) + c.m[11];
    if (c2 <= 0.0) return false;
    const double x = c0 / c2;
    const double y = c1 / c2;
    u = c.f[0] * x + c.f[2];
    v = c.f[1] * y + c.f[3];
    return u >= 0.0 && u < wd && v >= 0.0 && v < hd;   // NaN fails every comparison
}

// Point i of a float32 [P,3] array.
__device__ inline bool nv_project(const NvCam& c, const float* __restrict__ pts, long long i, double wd, double hd,
                                  double& u, double& v) {
    return nv_project_xyz(c, (double)pts[3 * i + 0], (double)pts[3 * i + 1], (double)pts[3 * i + 2], wd, hd, u, v);
}

}  // namespace cgs
