// The pinhole projection of a world point into a camera, shared by every kernel that must agree on which points a view
// keeps (novel_view.hip: cgs_project_points / cgs_render_points; edge_score.hip: cgs_point_mask; edge_seed.hip:
// cgs_voxel_votes, cgs_ray_claims and cgs_ray_wins -- k_voxel_votes, k_ray_claims, k_ray_wins through seed_walk;
// edge_support.hip: cgs_edge_support; edge_trim.hip: cgs_sample_support; edge_orient.hip: cgs_sample_support_oriented;
// edge_snap.hip: cgs_sample_snap_terms -- those seven and their _depth siblings through nv_verdict at the end of this file;
// edge_occlusion.hip: cgs_point_mask_depth through nv_project_xyz_depth, and
// cgs_mesh_depth, which projects a triangle's vertices in the same operation order through nv_camera_xyz / nv_image_uv;
// mesh_contours.hip: cgs_mesh_contours, an edge row's four vertices through the same two and nv_hidden;
// tsdf.hip: cgs_tsdf_integrate through nv_project_xyz_depth, reading the pixel nv_hidden reads).
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

// ---- occlusion (edge_occlusion.hip; include/curvegs.h, cgs_point_mask_depth).  New functions: the ones above stay as they are.

// c = R X + T in the operation order of nv_project_xyz, with no test at all.
__device__ inline void nv_camera_xyz(const NvCam& c, double X, double Y, double Z, double& c0, double& c1, double& c2) {
#pragma clang fp contract(off)
    c0 = ((c.m[0] * X + c.m[1] * Y) + c.m[2] * Z) + c.m[3];
    c1 = ((c.m[4] * X + c.m[5] * Y) + c.m[6] * Z) + c.m[7];
    c2 = ((c.m[8] * X + c.m[9] * Y) + c.m[10] * Z) + c.m[11];
}

// (u, v) of a camera-space point as nv_project_xyz forms them, with no in-frame test.
__device__ inline void nv_image_uv(const NvCam& c, double c0, double c1, double c2, double& u, double& v) {
#pragma clang fp contract(off)
    const double x = c0 / c2;
    const double y = c1 / c2;
    u = c.f[0] * x + c.f[2];
    v = c.f[1] * y + c.f[3];
}

// nv_project_xyz that also returns the camera-space depth c2: the same operations in the same order, the same verdict.
__device__ inline bool nv_project_xyz_depth(const NvCam& c, double X, double Y, double Z, double wd, double hd, double& u,
                                            double& v, double& c2) {
    double c0, c1;
    nv_camera_xyz(c, X, Y, Z, c0, c1, c2);
    if (c2 <= 0.0) return false;
    nv_image_uv(c, c0, c1, c2, u, v);
    return u >= 0.0 && u < wd && v >= 0.0 && v < hd;   // NaN fails every comparison
}

// THE occlusion rule, the one definition every depth-gated operator shares: a sample that a view sees at (u, v) with the
// camera-space depth c2 is hidden iff the view's depth plane has a surface more than `slack` in front of it at the sample's
// pixel.  depth_plane: float32 [height, width], camera z, +inf where there is no surface.  (u, v) must be inside the image
// (nv_project_xyz_depth returned true).  One float64 addition, one comparison; a NaN depth hides nothing.
__device__ inline bool nv_hidden(const float* __restrict__ depth_plane, int width, double u, double v, double c2,
                                 double slack) {
#pragma clang fp contract(off)
    const double d = (double)depth_plane[(size_t)floor(v) * (size_t)width + (size_t)floor(u)];
    return c2 > d + slack;
}

// ---- the gate as a template parameter (edge_support.hip, edge_trim.hip, edge_orient.hip, edge_snap.hip, edge_seed.hip;
// include/curvegs.h, cgs_edge_support_depth and the three after it, cgs_voxel_votes_depth and the two after it).  What one view says of one sample: not kept, kept and visible, or kept and
// hidden.  GATED = false is nv_project_xyz and nothing else -- depth_plane and slack are not touched, no sample is hidden;
// GATED = true is nv_project_xyz_depth followed by nv_hidden.  The two projections are the same operations in the same
// order, so NV_VISIBLE + NV_HIDDEN of the gated form is NV_VISIBLE of the ungated one, with the same (u, v).
enum NvVerdict { NV_OUT = 0, NV_VISIBLE = 1, NV_HIDDEN = 2 };

template <bool GATED>
__device__ __forceinline__ NvVerdict nv_verdict(const NvCam& c, double X, double Y, double Z, double wd, double hd,
                                                const float* __restrict__ depth_plane, int width, double slack, double& u,
                                                double& v) {
    if constexpr (GATED) {
        double c2;
        if (!nv_project_xyz_depth(c, X, Y, Z, wd, hd, u, v, c2)) return NV_OUT;
        return nv_hidden(depth_plane, width, u, v, c2, slack) ? NV_HIDDEN : NV_VISIBLE;
    } else {
        return nv_project_xyz(c, X, Y, Z, wd, hd, u, v) ? NV_VISIBLE : NV_OUT;
    }
}

}  // namespace cgs
