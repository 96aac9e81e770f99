// Occluding contours of a triangle mesh, drawn into one uint8 mask per view (include/curvegs.h, cgs_mesh_contours).  The rule
// is frozen in the header and stated here once, as two device functions: what one view says of one edge row
// (contour_classify) and one step of a drawn contour (contour_step).  Float64, nothing contracted, IEEE division; the
// projection is point_projection.h's, the occlusion rule its nv_hidden.  The geometry is free:
//   k_mesh_contours   grid (edge rows / 256, views), 4 waves.  The view is blockIdx.y, so the camera's 16 doubles are uniform
//                     loads.  One LANE classifies one row of that view -- twelve floats, four camera-space points, two dot
//                     products, the clip and the step count.  Few rows are contours (two of a 64-gon cylinder's 250 smooth
//                     edges per view), so a wave per (row, view) would mostly exit: instead a ballot gives the contours among
//                     the wave's 64 rows and the WHOLE wave draws them one after another -- the segment is read from its
//                     lane's registers by lane index (v_readlane: the index comes from the ballot, so it is uniform) and the
//                     64 lanes stride over its steps.  No lane leaves before the loop, so every lane read holds live values.
//                     A kept step stores the byte 1: a constant, so neither the order nor a second writer matters, and the
//                     mask is the same for every launch geometry.  No atomics, no LDS, no scratch, 64-bit offsets.
//                     k_mesh_contours<., true> is cgs_mesh_contours_clipped: the lane that classifies a row also cuts its
//                     OUT end at the plane c2 == near (near_cut of mesh_depth.h, the z-buffer's); the drawing is the same.
#include <algorithm>

#include "kernels.h"
#include "mesh_depth.h"
#include "point_projection.h"

namespace cgs {

constexpr int CONTOUR_THREADS = 256;        // 4 waves
constexpr int CONTOUR_MAX_VIEWS = 65535;    // views per launch: grid.y

// A contour of one view, ready to be drawn: the image segment from (ua, va) along (du, dv), the part [t0, t0 + dt] of it that
// the clip keeps, the camera depths of its two ends, and the number of steps n (steps k = 0 .. n).
struct ContourSeg {
    double ua, va, du, dv, t0, dt, za, zb;
    int n;
};

// One boundary of the Liang-Barsky clip: the part of the segment with p * t <= q.  False when nothing is left.
__device__ inline bool contour_clip_side(double p, double q, double& t0, double& t1) {
#pragma clang fp contract(off)
    if (p == 0.0) return !(q < 0.0);
    const double r = q / p;
    if (p < 0.0) {
        if (r > t1) return false;
        if (r > t0) t0 = r;
    } else {
        if (r < t0) return false;
        if (r < t1) t1 = r;
    }
    return true;
}

// True iff the row (a, b, c, d) -- twelve floats -- is a contour of the view AND has something to draw; then s is filled.
// CLIP = false is cgs_mesh_contours and reads no `near`.  CLIP = true is cgs_mesh_contours_clipped: an end is IN iff its
// c2 >= near, a row with no end IN is skipped, the contour test is the same (on the unclipped points), and an OUT end is
// then replaced by near_cut (mesh_depth.h) from the IN end toward it, before the image points and the depths are taken.
template <bool CLIP>
__device__ inline bool contour_classify(const NvCam& c, const float* __restrict__ row, int height, int width, double near,
                                        ContourSeg& s) {
#pragma clang fp contract(off)
    double p[4][3];
#pragma unroll
    for (int k = 0; k < 4; k++)
        nv_camera_xyz(c, (double)row[3 * k + 0], (double)row[3 * k + 1], (double)row[3 * k + 2], p[k][0], p[k][1], p[k][2]);
    bool in_a = true, in_b = true;
    if constexpr (CLIP) {
        in_a = p[0][2] >= near, in_b = p[1][2] >= near;   // (a NaN is OUT)
        if (!in_a && !in_b) return false;
    } else {
        if (!(p[0][2] > 0.0) || !(p[1][2] > 0.0)) return false;   // an end at or behind the camera plane, or NaN: no clipping
    }
    const double m0 = p[0][1] * p[1][2] - p[0][2] * p[1][1];   // m = a x b: the normal of the plane through the eye and the edge
    const double m1 = p[0][2] * p[1][0] - p[0][0] * p[1][2];
    const double m2 = p[0][0] * p[1][1] - p[0][1] * p[1][0];
    const double sc = (m0 * p[2][0] + m1 * p[2][1]) + m2 * p[2][2];
    const double sd = (m0 * p[3][0] + m1 * p[3][1]) + m2 * p[3][2];
    if (!(sc * sd > 0.0)) return false;   // opposite sides, edge-on (a zero) or NaN
    if constexpr (CLIP) {
        if (!in_a || !in_b) {
            const CamPt A = {p[0][0], p[0][1], p[0][2]}, B = {p[1][0], p[1][1], p[1][2]};
            const CamPt cut = in_a ? near_cut(A, B, near) : near_cut(B, A, near);
            // the OUT end becomes the cut (selects, not an indexed store: the array stays in registers)
            p[0][0] = in_a ? p[0][0] : cut.x, p[0][1] = in_a ? p[0][1] : cut.y, p[0][2] = in_a ? p[0][2] : cut.z;
            p[1][0] = in_a ? cut.x : p[1][0], p[1][1] = in_a ? cut.y : p[1][1], p[1][2] = in_a ? cut.z : p[1][2];
        }
    }
    double ub, vb;
    nv_image_uv(c, p[0][0], p[0][1], p[0][2], s.ua, s.va);
    nv_image_uv(c, p[1][0], p[1][1], p[1][2], ub, vb);
    s.du = ub - s.ua;
    s.dv = vb - s.va;
    const double wd = (double)width, hd = (double)height;
    double t0 = 0.0, t1 = 1.0;
    if (!contour_clip_side(-s.du, s.ua, t0, t1)) return false;        // u >= 0
    if (!contour_clip_side(s.du, wd - s.ua, t0, t1)) return false;    // u <= width
    if (!contour_clip_side(-s.dv, s.va, t0, t1)) return false;        // v >= 0
    if (!contour_clip_side(s.dv, hd - s.va, t0, t1)) return false;    // v <= height
    s.t0 = t0;
    s.dt = t1 - t0;
    const double len = fmax(fabs(s.dt * s.du), fabs(s.dt * s.dv));   // the clipped segment's longer extent, in pixels
    if (!(len <= wd + hd)) return false;   // NaN (an infinite coordinate): draws nothing.  Bounds n by 2 (width + height)
    s.n = (int)ceil(2.0 * len);            // at most half a pixel per step on either axis
    s.za = p[0][2];
    s.zb = p[1][2];
    return true;
}

// Step k of a contour (0 <= k <= s.n): the image point, the in-frame test of the projection, the perspective-correct depth,
// the gate, and the byte.  plane: the view's uint8 [height, width]; depth_plane: its float32 plane (GATED only).  The in-frame
// test, not the clip, is what keeps the store inside the plane: the clip only bounds the number of steps.
template <bool GATED>
__device__ inline void contour_step(const ContourSeg& s, int k, int height, int width, const float* __restrict__ depth_plane,
                                    double slack, uint8_t* __restrict__ plane) {
#pragma clang fp contract(off)
    const double f = s.n > 0 ? (double)k / (double)s.n : 0.0;
    const double t = s.t0 + s.dt * f;
    const double u = s.ua + t * s.du;
    const double v = s.va + t * s.dv;
    if (!(u >= 0.0 && u < (double)width && v >= 0.0 && v < (double)height)) return;   // NaN fails every comparison
    if constexpr (GATED) {
        const double z = 1.0 / ((1.0 - t) / s.za + t / s.zb);   // 1/z is linear along the image segment
        if (nv_hidden(depth_plane, width, u, v, z, slack)) return;
    }
    // 0 <= u < width, so 0 <= floor(u) <= width - 1 (likewise v): the pixel is inside the view's plane
    plane[(size_t)floor(v) * (size_t)width + (size_t)floor(u)] = 1;
}

// Lane `src`'s value in every lane; src is uniform over the wave.
__device__ inline int wave_read(int x, int src) { return __builtin_amdgcn_readlane(x, src); }
__device__ inline double wave_read(double x, int src) {
    return __hiloint2double(wave_read(__double2hiint(x), src), wave_read(__double2loint(x), src));
}

template <bool GATED, bool CLIP>
__global__ void __launch_bounds__(CONTOUR_THREADS) k_mesh_contours(int E, const float* __restrict__ rows,
                                                                  const double* __restrict__ intr,
                                                                  const double* __restrict__ w2c, int height, int width,
                                                                  const float* __restrict__ depth, double slack,
                                                                  double near, uint8_t* __restrict__ mask) {
    NvCam c;
    nv_load_cam(c, intr, w2c, blockIdx.y);
    const long long e = (long long)blockIdx.x * CONTOUR_THREADS + threadIdx.x;
    ContourSeg mine = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 0};
    const bool is_contour = e < E && contour_classify<CLIP>(c, rows + 12 * (size_t)e, height, width, near, mine);
    unsigned long long todo = __ballot(is_contour);   // every lane of the wave is here: none has returned
    const size_t off = (size_t)blockIdx.y * (size_t)height * (size_t)width;
    uint8_t* __restrict__ plane = mask + off;
    const float* __restrict__ dplane = GATED ? depth + off : nullptr;
    const int lane = threadIdx.x & 63;
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        ContourSeg s;
        s.ua = wave_read(mine.ua, src);
        s.va = wave_read(mine.va, src);
        s.du = wave_read(mine.du, src);
        s.dv = wave_read(mine.dv, src);
        s.t0 = wave_read(mine.t0, src);
        s.dt = wave_read(mine.dt, src);
        s.za = wave_read(mine.za, src);
        s.zb = wave_read(mine.zb, src);
        s.n = wave_read(mine.n, src);
        for (int k = lane; k <= s.n; k += 64) contour_step<GATED>(s, k, height, width, dplane, slack, plane);
    }
}

template <bool CLIP>
static hipError_t mesh_contours_launches(hipStream_t s, int E, const float* rows, int V, const double* intr, const double* w2c,
                                         int height, int width, const DepthGate* gate, double near, uint8_t* mask) {
    const size_t plane = (size_t)height * (size_t)width;
    hipError_t err = hipMemsetAsync(mask, 0, (size_t)V * plane, s);
    if (err != hipSuccess || E == 0) return err;
    const unsigned blocks = (unsigned)(((long long)E + CONTOUR_THREADS - 1) / CONTOUR_THREADS);
    ProfScope p(CLIP ? "mesh_contours_clipped" : "mesh_contours", s);
    for (int v0 = 0; v0 < V; v0 += CONTOUR_MAX_VIEWS) {
        const int nv = std::min(CONTOUR_MAX_VIEWS, V - v0);
        const dim3 grid(blocks, nv);
        const double* K = intr + 4 * (size_t)v0;
        const double* M = w2c + 12 * (size_t)v0;
        uint8_t* out = mask + (size_t)v0 * plane;
        if (gate)
            hipLaunchKernelGGL((k_mesh_contours<true, CLIP>), grid, dim3(CONTOUR_THREADS), 0, s, E, rows, K, M, height, width,
                               gate->depth + (size_t)v0 * plane, gate->slack, near, out);
        else
            hipLaunchKernelGGL((k_mesh_contours<false, CLIP>), grid, dim3(CONTOUR_THREADS), 0, s, E, rows, K, M, height, width,
                               (const float*)nullptr, 0.0, near, out);
    }
    return hipSuccess;
}

hipError_t launch_mesh_contours(hipStream_t s, int E, const float* rows, int V, const double* intr, const double* w2c,
                                int height, int width, const DepthGate* gate, const double* near, uint8_t* mask) {
    return near ? mesh_contours_launches<true>(s, E, rows, V, intr, w2c, height, width, gate, *near, mask)
                : mesh_contours_launches<false>(s, E, rows, V, intr, w2c, height, width, gate, 0.0, mask);
}

}  // namespace cgs
