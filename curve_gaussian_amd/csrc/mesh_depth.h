// The frozen rule of cgs_mesh_depth (include/curvegs.h) as two device functions -- a (triangle, view)'s set-up and one pixel
// of it -- so that every launch geometry states it once: k_mesh_depth (edge_occlusion.hip, one wave per (triangle, view))
// and the rejected shape kept as a probe (profiles/probes/edge_occlusion_thread.hip, one thread per (triangle, view)).
// Below them the near-plane clip of cgs_mesh_depth_clipped / cgs_mesh_contours_clipped: the one cut (near_cut), a
// triangle's pieces (mesh_tri_clip) and the set-up of a piece from its camera-space vertices (mesh_tri_setup_cam).
#pragma once
#include "point_projection.h"

namespace cgs {

constexpr unsigned int DEPTH_INF_BITS = 0x7f800000u;   // +inf, the largest bit pattern of a non-negative float

struct MeshTri {
    double u[3], v[3], z[3], area;
    int jlo, jhi, ilo, ihi;   // the candidate pixels, inside the image; empty when jlo > jhi or ilo > ihi
};

// The second half of the set-up, from the image points: the area test and the candidate box.
__device__ inline bool mesh_tri_box(int height, int width, MeshTri& t) {
#pragma clang fp contract(off)
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
    return mesh_tri_box(height, width, t);
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

// ---- near-plane clipping (include/curvegs.h, cgs_mesh_depth_clipped / cgs_mesh_contours_clipped).  New functions: the ones
// above stay as they are.  A camera-space point is IN iff its c2 >= near (a NaN is OUT).

struct CamPt {
    double x, y, z;
};

// THE cut, the one definition the z-buffer and the contours share: where the edge from its IN end a toward its OUT end b
// meets the plane c2 == near.  Always taken in this direction, so two triangles that share a straddling edge get the same
// point to the bit.  p.z is assigned, not computed.
__device__ inline CamPt near_cut(const CamPt& a, const CamPt& b, double near) {
#pragma clang fp contract(off)
    const double t = (a.z - near) / (a.z - b.z);
    CamPt p;
    p.x = a.x + t * (b.x - a.x);
    p.y = a.y + t * (b.y - a.y);
    p.z = near;
    return p;
}

// mesh_tri_setup of a triangle given by its camera-space vertices: the same operations in the same order from c on.
__device__ inline bool mesh_tri_setup_cam(const NvCam& c, const CamPt& p0, const CamPt& p1, const CamPt& p2, int height,
                                          int width, MeshTri& t) {
#pragma clang fp contract(off)
    const CamPt* p[3] = {&p0, &p1, &p2};
#pragma unroll
    for (int k = 0; k < 3; k++) {
        t.z[k] = p[k]->z;
        if (!(t.z[k] > 0.0)) return false;
        nv_image_uv(c, p[k]->x, p[k]->y, t.z[k], t.u[k], t.v[k]);
        if (t.u[k] != t.u[k] || t.v[k] != t.v[k]) return false;
    }
    return mesh_tri_box(height, width, t);
}

// The pieces of a triangle in front of the plane c2 == near: their number (0, 1 or 2), the first in q[0..2], the second in
// (q[0], q[2], q[3]).  Three vertices IN: the triangle itself.  One IN, at index i: (a, cut(a,b), cut(a,c)) with a = i,
// b = i + 1, c = i + 2 (mod 3).  Two IN, the OUT one at index i: c = i, a = i + 1, b = i + 2 and the pieces (a, b, cut(b,c)),
// (a, cut(b,c), cut(a,c)).  A NaN in any coordinate: none.  The rotation is written with selects, not with an indexed array
// (which would live in scratch memory); every lane of a wave holds the same triangle, so the branches are uniform.
__device__ inline int mesh_tri_clip(const CamPt& v0, const CamPt& v1, const CamPt& v2, double near, CamPt (&q)[4]) {
    if (v0.x != v0.x || v0.y != v0.y || v0.z != v0.z || v1.x != v1.x || v1.y != v1.y || v1.z != v1.z || v2.x != v2.x ||
        v2.y != v2.y || v2.z != v2.z)
        return 0;
    const bool in0 = v0.z >= near, in1 = v1.z >= near, in2 = v2.z >= near;
    const int nin = (int)in0 + (int)in1 + (int)in2;
    if (nin == 0) return 0;
    if (nin == 3) {
        q[0] = v0, q[1] = v1, q[2] = v2;
        return 1;
    }
    // i: the one IN (nin == 1) or the one OUT (nin == 2); (r0, r1, r2) = (v_i, v_i+1, v_i+2)
    const int i = nin == 1 ? (in0 ? 0 : in1 ? 1 : 2) : (!in0 ? 0 : !in1 ? 1 : 2);
    const CamPt r0 = i == 0 ? v0 : i == 1 ? v1 : v2;
    const CamPt r1 = i == 0 ? v1 : i == 1 ? v2 : v0;
    const CamPt r2 = i == 0 ? v2 : i == 1 ? v0 : v1;
    if (nin == 1) {
        q[0] = r0, q[1] = near_cut(r0, r1, near), q[2] = near_cut(r0, r2, near);
        return 1;
    }
    q[0] = r1, q[1] = r2, q[2] = near_cut(r2, r0, near), q[3] = near_cut(r1, r0, near);
    return 2;
}

}  // namespace cgs
