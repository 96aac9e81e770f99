// The frozen rule of cgs_stereo_sweep and cgs_stereo_consistency (include/curvegs.h) as device functions, so that every
// launch geometry states it once: k_stereo_sweep (stereo_depth.hip) and the geometry kept as a probe
// (profiles/probes/stereo_depth_geometries.hip).  What a geometry may choose is WHERE a reference pixel's own numbers come
// from -- its patch bytes and the per-column / per-row ray slopes ((px - cx) / fx, (py - cy) / fy) -- through the Ref
// parameter below: each of them is one fixed sequence of rounded operations whoever evaluates it, so reading it from LDS
// or forming it again gives the same bits.  Everything else -- the order of the taps, of the sources and of the hypotheses,
// every running sum -- is here.  Float64, nothing contracted, IEEE division, no square root.
#pragma once
#include <cstdint>

#include "point_projection.h"

namespace cgs {

struct StereoArgs {
    const uint8_t* gray;   // [V,height,width]
    const double* intr;    // [V,4]
    const double* inv;     // [V,D]
    const int* src;        // [V,S]
    const double* rel;     // [V,S,12]
    int V, height, width, D, S, radius, min_sources;
    double thr;            // (min_var * n) * n
    double max_cost;
};

__device__ inline double stereo_inf() { return __longlong_as_double(0x7ff0000000000000LL); }

// The reference pixel's numbers straight from global memory: Ref of the plain geometry.
struct StereoRefGlobal {
    const uint8_t* plane;   // the reference view's bytes
    int width, i, j;
    double fx, fy, cx, cy;
    __device__ double tap(int di, int dj) const { return (double)plane[(size_t)(i + di) * (size_t)width + (size_t)(j + dj)]; }
    __device__ double dx(int dj) const {
#pragma clang fp contract(off)
        const double px = (double)(j + dj) + 0.5;
        return (px - cx) / fx;
    }
    __device__ double dy(int di) const {
#pragma clang fp contract(off)
        const double py = (double)(i + di) + 0.5;
        return (py - cy) / fy;
    }
};

// sr, srr of a reference patch that lies inside the image; taps in row-major order.
template <class Ref>
__device__ inline void stereo_ref_sums(const Ref& ref, int R, double& sr, double& srr) {
#pragma clang fp contract(off)
    sr = 0.0, srr = 0.0;
    for (int di = -R; di <= R; di++)
        for (int dj = -R; dj <= R; dj++) {
            const double r = ref.tap(di, dj);
            sr += r;
            srr += r * r;
        }
}

// One source at one hypothesis: false when the source does not count, else its cost.  c: m = rel[v][s], f = the SOURCE's
// intrinsics; sp: the source's bytes.  An invalid tap ends the walk: the source does not count whatever the others hold.
template <class Ref>
__device__ inline bool stereo_source_cost(const Ref& ref, int R, double n, double thr, double sr, double var_r, double z,
                                          const NvCam& c, const uint8_t* __restrict__ sp, int height, int width, double& cost) {
#pragma clang fp contract(off)
    const double xmax = (double)(width - 1), ymax = (double)(height - 1);
    double ss = 0.0, sss = 0.0, srs = 0.0;
    for (int di = -R; di <= R; di++) {
        const double Y = ref.dy(di) * z;
        for (int dj = -R; dj <= R; dj++) {
            const double X = ref.dx(dj) * z;
            double c0, c1, c2, u, v;
            nv_camera_xyz(c, X, Y, z, c0, c1, c2);
            if (!(c2 > 0.0)) return false;
            nv_image_uv(c, c0, c1, c2, u, v);
            const double x = u - 0.5, y = v - 0.5;
            const double x0 = floor(x), y0 = floor(y);
            // in float64 BEFORE any conversion: a NaN or an infinity fails, and the four bytes below lie inside the plane
            if (!(x0 >= 0.0 && x0 + 1.0 <= xmax && y0 >= 0.0 && y0 + 1.0 <= ymax)) return false;
            const double a = x - x0, b = y - y0;
            const uint8_t* g = sp + (size_t)y0 * (size_t)width + (size_t)x0;
            const double g00 = (double)g[0], g01 = (double)g[1], g10 = (double)g[width], g11 = (double)g[width + 1];
            const double top = g00 * (1.0 - a) + g01 * a;
            const double bot = g10 * (1.0 - a) + g11 * a;
            const double val = top * (1.0 - b) + bot * b;
            ss += val;
            sss += val * val;
            srs += ref.tap(di, dj) * val;
        }
    }
    const double var_s = n * sss - ss * ss;
    if (!(var_s > thr)) return false;
    const double cov = n * srs - sr * ss;
    const double score = (cov * fabs(cov)) / (var_r * var_s);
    cost = 1.0 - score;
    return true;
}

// What view v's pixel stores, given sr / srr of its patch (which lies inside the image).  The winner and its two
// neighbours ride along the hypothesis loop: no cost volume.
template <class Ref>
__device__ inline float stereo_sweep_pixel(const StereoArgs& A, int v, const Ref& ref, double sr, double srr) {
#pragma clang fp contract(off)
    const int R = A.radius;
    const double n = (double)((2 * R + 1) * (2 * R + 1));
    const double var_r = n * srr - sr * sr;
    if (!(var_r > A.thr)) return 0.0f;
    const double inf = stereo_inf();
    const double* __restrict__ inv = A.inv + (size_t)v * (size_t)A.D;
    const size_t plane = (size_t)A.height * (size_t)A.width;
    int best = 0;
    double cb = inf, cm = inf, cp = inf, prev = inf;
    for (int d = 0; d < A.D; d++) {
        const double z = 1.0 / inv[d];
        double sum = 0.0;
        int count = 0;
        for (int s = 0; s < A.S; s++) {
            const size_t vs = (size_t)v * (size_t)A.S + (size_t)s;
            const int w = A.src[vs];
            if (w < 0 || w >= A.V) continue;   // no source (uniform over the workgroup)
            NvCam c;
#pragma unroll
            for (int k = 0; k < 12; k++) c.m[k] = A.rel[12 * vs + k];
#pragma unroll
            for (int k = 0; k < 4; k++) c.f[k] = A.intr[4 * (size_t)w + k];
            double cs;
            if (stereo_source_cost(ref, R, n, A.thr, sr, var_r, z, c, A.gray + (size_t)w * plane, A.height, A.width, cs)) {
                sum += cs;
                count++;
            }
        }
        const double cost = count >= A.min_sources ? sum / (double)count : inf;   // min_sources >= 1
        if (d == best + 1) cp = cost;
        if (d == 0 || cost < cb) best = d, cb = cost, cm = prev, cp = inf;
        prev = cost;
    }
    if (!(cb < inf && cb <= A.max_cost)) return 0.0f;
    double o = 0.0;
    if (best > 0 && best < A.D - 1 && cm < inf && cp < inf) {
        const double den = (cm - 2.0 * cb) + cp;
        if (den > 0.0) o = fmin(fmax((0.5 * (cm - cp)) / den, -0.5), 0.5);
    }
    double q = inv[best];
    if (o != 0.0) {   // (o == 0 adds nothing; the ends have no neighbour to read)
        const double step = o >= 0.0 ? inv[best + 1] - inv[best] : inv[best] - inv[best - 1];
        q = inv[best] + o * step;
    }
    return (float)(1.0 / q);
}

// cgs_stereo_consistency's pixel: depth is the INPUT stack, read at (v, i, j) and at the sources' pixels.
__device__ inline float stereo_consistent_pixel(const float* __restrict__ depth, const double* __restrict__ intr,
                                                const int* __restrict__ src, const double* __restrict__ rel,
                                                const double* __restrict__ tol, int V, int height, int width, int S,
                                                int min_consistent, int v, int i, int j) {
#pragma clang fp contract(off)
    const size_t plane = (size_t)height * (size_t)width;
    const float zf = depth[(size_t)v * plane + (size_t)i * (size_t)width + (size_t)j];
    const double z = (double)zf;
    if (!(z > 0.0)) return 0.0f;
    const double* f = intr + 4 * (size_t)v;
    const double px = (double)j + 0.5, py = (double)i + 0.5;
    const double X = ((px - f[2]) / f[0]) * z, Y = ((py - f[3]) / f[1]) * z;
    const double t = tol[v], wd = (double)width, hd = (double)height;
    int agree = 0;
    for (int s = 0; s < S; s++) {
        const size_t vs = (size_t)v * (size_t)S + (size_t)s;
        const int w = src[vs];
        if (w < 0 || w >= V) continue;
        NvCam c;
#pragma unroll
        for (int k = 0; k < 12; k++) c.m[k] = rel[12 * vs + k];
#pragma unroll
        for (int k = 0; k < 4; k++) c.f[k] = intr[4 * (size_t)w + k];
        double u, vv, c2;
        if (!nv_project_xyz_depth(c, X, Y, z, wd, hd, u, vv, c2)) continue;   // 0 <= u < width, 0 <= v < height
        const double ds = (double)depth[(size_t)w * plane + (size_t)floor(vv) * (size_t)width + (size_t)floor(u)];
        if (!(ds > 0.0)) continue;
        if (fabs(1.0 / ds - 1.0 / c2) <= t) agree++;
    }
    return agree >= min_consistent ? zf : 0.0f;
}

}  // namespace cgs
