// The frozen rule of cgs_surfel_depth (include/curvegs.h) as two device functions -- a (surfel, view)'s set-up and one pixel
// of it -- so that every launch geometry states it once: k_surfel_depth (surfel_depth.hip, one wave per (surfel, view)) and
// the two other shapes kept as probes (profiles/probes/surfel_depth_geometries.hip: one lane per (surfel, view), alone or with
// the large disks handed to the whole wave).  Below them the wave's walk over a set-up surfel's candidate box.
#pragma once
#include "mesh_depth.h"

namespace cgs {

// A surfel in one view: the camera-space centre c, the camera-space normal n, num = n . c, r2 = r * r, the candidate box.
struct Surfel {
    double c0, c1, c2, n0, n1, n2, num, r2;
    int jlo, jhi, ilo, ihi;   // the candidate pixels, inside the image; empty when jlo > jhi or ilo > ihi
};

// False for a surfel the view skips: a radius that is not > 0 (NaN included), a disk that could reach the camera plane
// (c2 - r <= 0 or NaN; r = +inf ends here), a NaN bound of the candidate box (such a surfel covers no pixel: the bound is NaN
// only with a NaN or infinite c0 / c1 or a NaN camera, and then no d2 is <= r2), no candidate.  nrm == nullptr: n = (0, 0, 1).
__device__ inline bool surfel_setup(const NvCam& c, const float* __restrict__ p, const float* __restrict__ nrm, float radius,
                                    int height, int width, Surfel& s) {
#pragma clang fp contract(off)
    nv_camera_xyz(c, (double)p[0], (double)p[1], (double)p[2], s.c0, s.c1, s.c2);
    s.n0 = 0.0, s.n1 = 0.0, s.n2 = 1.0;
    if (nrm) {   // (uniform over the launch)
        const double X = (double)nrm[0], Y = (double)nrm[1], Z = (double)nrm[2];
        s.n0 = (c.m[0] * X + c.m[1] * Y) + c.m[2] * Z;
        s.n1 = (c.m[4] * X + c.m[5] * Y) + c.m[6] * Z;
        s.n2 = (c.m[8] * X + c.m[9] * Y) + c.m[10] * Z;
    }
    const double r = (double)radius;
    const double zlo = s.c2 - r, zhi = s.c2 + r;
    if (!(r > 0.0) || !(zlo > 0.0)) return false;   // no clipping: dropped whole
    const double a0 = s.c0 - r, b0 = s.c0 + r, a1 = s.c1 - r, b1 = s.c1 + r;
    const double ulo = c.f[0] * fmin(a0 / zlo, a0 / zhi) + c.f[2];
    const double uhi = c.f[0] * fmax(b0 / zlo, b0 / zhi) + c.f[2];
    const double vlo = c.f[1] * fmin(a1 / zlo, a1 / zhi) + c.f[3];
    const double vhi = c.f[1] * fmax(b1 / zlo, b1 / zhi) + c.f[3];
    if (ulo != ulo || uhi != uhi || vlo != vlo || vhi != vhi) return false;
    // the centres (j + 0.5, i + 0.5) inside the box, borders included, clamped to the image in float64 BEFORE the conversion
    const double wd = (double)width, hd = (double)height;
    s.jlo = (int)fmin(fmax(ceil(ulo - 0.5), 0.0), wd);
    s.jhi = (int)fmax(fmin(floor(uhi - 0.5), wd - 1.0), -1.0);
    s.ilo = (int)fmin(fmax(ceil(vlo - 0.5), 0.0), hd);
    s.ihi = (int)fmax(fmin(floor(vhi - 0.5), hd - 1.0), -1.0);
    s.num = (s.n0 * s.c0 + s.n1 * s.c1) + s.n2 * s.c2;
    s.r2 = r * r;
    return s.jlo <= s.jhi && s.ilo <= s.ihi;
}

// Candidate pixel (j, i) of the view's plane (uint32 words holding float bits): the ray through the pixel centre meets the
// disk's plane at camera depth s; covered iff that point lies within r of the centre.  The store is mesh_tri_pixel's: the
// plain read, then the integer atomic minimum on the float's bits.  A NaN anywhere fails the coverage test or the float test.
__device__ inline void surfel_pixel(const NvCam& c, const Surfel& f, int i, int j, unsigned int* __restrict__ plane, int width) {
#pragma clang fp contract(off)
    const double px = (double)j + 0.5, py = (double)i + 0.5;
    const double dx = (px - c.f[2]) / c.f[0], dy = (py - c.f[3]) / c.f[1];
    const double den = (f.n0 * dx + f.n1 * dy) + f.n2;
    const double s = f.num / den;
    const double qx = s * dx - f.c0, qy = s * dy - f.c1, qz = s - f.c2;
    const double d2 = (qx * qx + qy * qy) + qz * qz;
    if (!(d2 <= f.r2)) return;
    const float zf = (float)s;
    const unsigned int bits = __float_as_uint(zf);
    if (!(zf > 0.0f) || bits >= DEPTH_INF_BITS) return;   // not a positive finite float: stores nothing
    unsigned int* at = plane + (size_t)i * (size_t)width + (size_t)j;   // ilo <= i <= ihi <= height - 1, likewise j
    if (bits < *at) atomicMin(at, bits);
}

// The number of candidate pixels of a set-up surfel: at most 2^28.
__device__ inline unsigned int surfel_box_pixels(const Surfel& f) {
    return (unsigned int)(f.jhi - f.jlo + 1) * (unsigned int)(f.ihi - f.ilo + 1);
}

// The wave's 64 lanes over the box of ONE surfel (every lane holds the same f), row-major, 64 pixels at a time.
__device__ inline void surfel_draw_wave(const NvCam& c, const Surfel& f, int lane, unsigned int* __restrict__ plane, int width) {
    const unsigned int bw = (unsigned int)(f.jhi - f.jlo + 1);
    const unsigned int n = surfel_box_pixels(f);
    for (unsigned int idx = (unsigned int)lane; idx < n; idx += 64) {
        const unsigned int r = idx / bw;
        surfel_pixel(c, f, f.ilo + (int)r, f.jlo + (int)(idx - r * bw), plane, width);
    }
}

}  // namespace cgs
