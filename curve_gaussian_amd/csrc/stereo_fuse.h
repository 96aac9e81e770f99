// The frozen rule of cgs_stereo_warp and cgs_stereo_fuse (include/curvegs.h) as device functions, so that every launch
// geometry states it once: k_stereo_warp / k_stereo_fuse (stereo_fuse.hip) and the warp geometry kept as a probe
// (profiles/probes/stereo_fuse_geometries.hip).  What a geometry may choose is WHICH lane takes which (target, slot, source
// pixel) or which target pixel; what a lane then does is here.  Float64, nothing contracted, IEEE division, no square root,
// running sums from 0.0 in the stated order.
#pragma once
#include <cstdint>

#include "mesh_depth.h"   // DEPTH_INF_BITS and, by inclusion, point_projection.h

namespace cgs {

constexpr int STEREO_MAX_FUSE = 16;   // CGS_STEREO_MAX_FUSE

// A positive finite float: what a depth map's pixel must hold to be a depth, and what the warp stores.
__device__ inline bool stereo_is_depth(float z) { return z > 0.0f && __float_as_uint(z) < DEPTH_INF_BITS; }   // a NaN fails

// Source pixel (i, j) of view w into one slot's plane of the target (uint32 words holding float bits, +inf where nothing
// has landed).  z: depth[w][i][j]; fw: the SOURCE's intrinsics; c: m = into[v][s], f = the TARGET's intrinsics.  The store
// is mesh_tri_pixel's (mesh_depth.h): the plain read, then the integer atomic minimum on the float's bits -- depths only
// ever fall, so a stale read can only cost an atomic that changes nothing.
__device__ inline void stereo_warp_pixel(float zsrc, const double* __restrict__ fw, const NvCam& c, int height, int width,
                                         int i, int j, unsigned int* __restrict__ plane) {
#pragma clang fp contract(off)
    if (!stereo_is_depth(zsrc)) return;
    const double z = (double)zsrc;
    const double px = (double)j + 0.5, py = (double)i + 0.5;
    const double X = ((px - fw[2]) / fw[0]) * z, Y = ((py - fw[3]) / fw[1]) * z;
    double u, v, c2;
    if (!nv_project_xyz_depth(c, X, Y, z, (double)width, (double)height, u, v, c2)) return;   // c2 > 0, 0 <= u < width, 0 <= v < height
    const float zf = (float)c2;
    if (!stereo_is_depth(zf)) return;
    unsigned int* at = plane + (size_t)floor(v) * (size_t)width + (size_t)floor(u);
    const unsigned int bits = __float_as_uint(zf);
    if (bits < *at) atomicMin(at, bits);
}

// One target pixel.  own: depth[v][i][j]; slot s's value is wp[s * stride], s < F <= STEREO_MAX_FUSE.  The candidates'
// inverse depths live in registers: every loop below has a constant trip count and is unrolled, the guards on F are
// uniform, so q[] is never indexed at run time (an indexed private array would live in scratch memory).  An absent
// candidate holds a NaN: a present one is 1 / (a positive finite float), never a NaN, and a NaN fails every comparison
// below, so it supports nothing and is no member.
__device__ inline void stereo_fuse_pixel(float own, const float* __restrict__ wp, size_t stride, int F, double tol,
                                         int min_support, float& out, uint8_t& support) {
#pragma clang fp contract(off)
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    double q[STEREO_MAX_FUSE + 1];
    q[0] = stereo_is_depth(own) ? 1.0 / (double)own : nan;
#pragma unroll
    for (int s = 0; s < STEREO_MAX_FUSE; s++) {
        q[s + 1] = nan;
        if (s < F) {
            const float w = wp[(size_t)s * stride];
            if (stereo_is_depth(w)) q[s + 1] = 1.0 / (double)w;
        }
    }
    int sb = -1;        // no best yet: the first present candidate replaces it
    double qb = nan;
#pragma unroll
    for (int k = 0; k <= STEREO_MAX_FUSE; k++) {
        if (k > F) continue;
        int cnt = 0;
#pragma unroll
        for (int m = 0; m <= STEREO_MAX_FUSE; m++)
            if (m <= F && fabs(q[m] - q[k]) <= tol) cnt++;
        if (q[k] == q[k] && (cnt > sb || (cnt == sb && q[k] < qb))) sb = cnt, qb = q[k];
    }
    out = 0.0f, support = 0;
    if (sb < min_support) return;   // min_support >= 1: also the pixel without a candidate
    double sum = 0.0;
    int count = 0;
#pragma unroll
    for (int m = 0; m <= STEREO_MAX_FUSE; m++)
        if (m <= F && fabs(q[m] - qb) <= tol) sum += q[m], count++;
    const double mean = sum / (double)count;
    out = (float)(1.0 / mean);
    support = (uint8_t)count;
}

}  // namespace cgs
