// The frozen rule of cgs_mesh_depth (include/curvegs.h) as two device functions -- a (triangle, view)'s set-up and one pixel
// of it -- so that every launch geometry states it once: k_mesh_depth (edge_occlusion.hip, one wave per (triangle, view))
// and the rejected shape kept as a probe (profiles/probes/edge_occlusion_thread.hip, one thread per (triangle, view)).
#pragma once
#include "point_projection.h"

namespace cgs {

constexpr unsigned int DEPTH_INF_BITS = 0x7f800000u;   // +inf, the largest bit pattern of a non-negative float

struct MeshTri {
    double u[3], v[3], z[3], area;
    int jlo, jhi, ilo, ihi;   // the candidate pixels, inside the image; empty when jlo > jhi or ilo > ihi
};

// False for a triangle the view skips (a vertex with c2 <= 0 or NaN, a NaN image coordinate, area 0 or NaN, no candidate).
__device__ inline bool mesh_tri_setup(const NvCam& c, const float* __restrict__ p, int height, int width, MeshTri& t) {
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < 3; k++) {
        double c0, c1;
        nv_camera_xyz(c, (double)p[3 * k + 0], (double)p[3 * k + 1], (double)p[3 * k + 2], c0, c1, t.z[k]);
        if (!(t.z[k] > 0.0)) return false;   // behind the camera, or NaN: no clipping
        nv_image_uv(c, c0, c1, t.z[k], t.u[k], t.v[k]);
        if (t.u[k] != t.u[k] || t.v[k] != t.v[k]) return false;
    }
    t.area = (t.u[1] - t.u[0]) * (t.v[2] - t.v[0]) - (t.v[1] - t.v[0]) * (t.u[2] - t.u[0]);
    if (!(t.area != 0.0)) return false;      // zero or NaN
    // the centres (j + 0.5, i + 0.5) inside the bounding box, borders included, clamped to the image in float64 BEFORE the
    // conversion (a coordinate may be huge or infinite)
    const double wd = (double)width, hd = (double)height;
    t.jlo = (int)fmin(fmax(ceil(fmin(fmin(t.u[0], t.u[1]), t.u[2]) - 0.5), 0.0), wd);
    t.jhi = (int)fmax(fmin(floor(fmax(fmax(t.u[0], t.u[1]), t.u[2]) - 0.5), wd - 1.0), -1.0);
    t.ilo = (int)fmin(fmax(ceil(fmin(fmin(t.v[0], t.v[1]), t.v[2]) - 0.5), 0.0), hd);
    t.ihi = (int)fmax(fmin(floor(fmax(fmax(t.v[0], t.v[1]), t.v[2]) - 0.5), hd - 1.0), -1.0);
    return t.jlo <= t.jhi && t.ilo <= t.ihi;
}

// Candidate pixel (j, i) of the view's plane (uint32 words holding float bits): the coverage test, the perspective-correct
// depth and the integer atomic minimum.  The plane is read first and the atomic left out when the stored depth is already
// nearer: depths only ever fall, so a stale read can only cost an atomic that changes nothing, never drop one that would.
__device__ inline void mesh_tri_pixel(const MeshTri& t, int i, int j, unsigned int* __restrict__ plane, int width) {
#pragma clang fp contract(off)
    const double px = (double)j + 0.5, py = (double)i + 0.5;
    const double e0 = (t.u[2] - t.u[1]) * (py - t.v[1]) - (t.v[2] - t.v[1]) * (px - t.u[1]);
    const double e1 = (t.u[0] - t.u[2]) * (py - t.v[2]) - (t.v[0] - t.v[2]) * (px - t.u[2]);
    const double e2 = (t.u[1] - t.u[0]) * (py - t.v[0]) - (t.v[1] - t.v[0]) * (px - t.u[0]);
    if (!((e0 >= 0.0 && e1 >= 0.0 && e2 >= 0.0) || (e0 <= 0.0 && e1 <= 0.0 && e2 <= 0.0))) return;
    const double invz = ((e0 / t.area) / t.z[0] + (e1 / t.area) / t.z[1]) + (e2 / t.area) / t.z[2];
    const float zf = (float)(1.0 / invz);
    const unsigned int bits = __float_as_uint(zf);
    if (!(zf > 0.0f) || bits >= DEPTH_INF_BITS) return;   // not a positive finite float: stores nothing
    unsigned int* at = plane + (size_t)i * (size_t)width + (size_t)j;   // ilo <= i <= ihi <= height - 1, likewise j
    if (bits < *at) atomicMin(at, bits);
}

}  // namespace cgs
