// Per-edge 2D support of extracted edges (include/curvegs.h, cgs_edge_support): how many of an edge's own samples every
// view sees, and how many of those land within a tolerance of a detected edge pixel.
//   k_edge_support     one wave per (edge, view), SUPPORT_WAVES edges per workgroup; blockIdx.y is the view, so the camera
//                      index is wave-uniform and the 16 doubles of a camera are scalar loads, as in visibility.hip and
//                      edge_seed.hip.  The lanes stride over the edge's points (12 consecutive bytes per lane: a wave reads
//                      768 consecutive bytes per step), project each with nv_project_xyz (point_projection.h, the device
//                      function of cgs_project_points / cgs_point_mask) and gather one int32 of the view's distance
//                      transform per seen point.  1 + T counts stay in registers; one __shfl_xor reduction per wave; lane 0
//                      stores the 1 + T integers.  No atomics, no LDS, no barrier: integers only, so the result does not
//                      depend on the launch geometry.  Every output word is written (an edge without points stores zeros).
//                      A template over GATED: false is cgs_edge_support as it always was (depth, slack and hidden are not
//                      read); true is cgs_edge_support_depth -- nv_verdict (point_projection.h) sends a sample that the view's
//                      depth plane hides to a sixth counter instead of `seen`, one float32 gather more per seen sample.
#include <algorithm>

#include "kernels.h"
#include "point_projection.h"

namespace cgs {

constexpr int SUPPORT_THREADS = 256;
constexpr int SUPPORT_WAVES = SUPPORT_THREADS / 64;   // edges per workgroup
constexpr int SUPPORT_MAX_VIEWS = 65535;              // views per launch: grid.y
static_assert(CGS_EDGE_SUPPORT_MAX_TOL == 4, "the kernel keeps 1 + 4 counts in registers");

template <bool GATED>
__global__ void __launch_bounds__(SUPPORT_THREADS) k_edge_support(int E, int P, const float* __restrict__ pts,
                                                                 const int* __restrict__ offsets, int V, int v0,
                                                                 const double* __restrict__ intr,
                                                                 const double* __restrict__ w2c, int height, int width,
                                                                 const int* __restrict__ d2, int T,
                                                                 const int* __restrict__ tol2, int* __restrict__ counts,
                                                                 const float* __restrict__ depth, double slack,
                                                                 int* __restrict__ hidden) {
    constexpr int MT = CGS_EDGE_SUPPORT_MAX_TOL;
    const int lane = threadIdx.x & 63;
    const long long e = (long long)blockIdx.x * SUPPORT_WAVES + (threadIdx.x >> 6);
    if (e >= E) return;   // wave-uniform; the kernel has no barrier
    const int view = blockIdx.y;   // of this launch: intr, w2c and d2 start at its first view, counts at view v0
    NvCam c;
    nv_load_cam(c, intr, w2c, view);
    int t2[MT];
#pragma unroll
    for (int t = 0; t < MT; t++) t2[t] = t < T ? tol2[t] : -1;   // a distance is >= 0: an unused slot counts nothing
    // the edge's range, clipped to the points that exist: offsets that break their contract read nothing out of bounds
    const long long begin = std::min<long long>(std::max<long long>(offsets[e], 0), P);
    const long long end = std::min<long long>(std::max<long long>(offsets[e + 1], 0), P);
    const double wd = (double)width, hd = (double)height;
    const int* __restrict__ plane = d2 + (size_t)view * (size_t)height * (size_t)width;
    const float* __restrict__ dplane = GATED ? depth + (size_t)view * (size_t)height * (size_t)width : nullptr;
    int seen = 0, hid = 0, near[MT];
#pragma unroll
    for (int t = 0; t < MT; t++) near[t] = 0;
    for (long long i = begin + lane; i < end; i += 64) {   // at most 2^31 / 64 points per lane: int counts
        double u, v;
        const NvVerdict verdict = nv_verdict<GATED>(c, (double)pts[3 * i + 0], (double)pts[3 * i + 1], (double)pts[3 * i + 2],
                                                    wd, hd, dplane, width, slack, u, v);
        if (verdict == NV_OUT) continue;
        if (GATED && verdict == NV_HIDDEN) {
            hid++;
            continue;
        }
        // 0 <= u < W, so 0 <= floor(u) <= W - 1 (likewise v): the pixel is inside the view's plane
        const int d = plane[(size_t)floor(v) * (size_t)width + (size_t)floor(u)];
        seen++;
#pragma unroll
        for (int t = 0; t < MT; t++) near[t] += d <= t2[t] ? 1 : 0;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        seen += __shfl_xor(seen, off, 64);
        if (GATED) hid += __shfl_xor(hid, off, 64);
#pragma unroll
        for (int t = 0; t < MT; t++) near[t] += __shfl_xor(near[t], off, 64);
    }
    if (lane != 0) return;
    int* __restrict__ out = counts + ((size_t)e * (size_t)V + (size_t)(v0 + view)) * (size_t)(1 + T);
    out[0] = seen;
#pragma unroll
    for (int t = 0; t < MT; t++)
        if (t < T) out[1 + t] = near[t];
    if (GATED && hidden) hidden[(size_t)e * (size_t)V + (size_t)(v0 + view)] = hid;   // written, like counts
}

template <bool GATED>
static void edge_support_launches(hipStream_t s, int E, int P, const float* points, const int* offsets, int V,
                                  const double* intr, const double* w2c, int height, int width, const int* d2, int T,
                                  const int* tol2, int* counts, DepthGate gate, int* hidden) {
    const size_t plane = (size_t)height * (size_t)width;
    const unsigned blocks = (unsigned)(((long long)E + SUPPORT_WAVES - 1) / SUPPORT_WAVES);
    ProfScope p(GATED ? "edge_support_depth" : "edge_support", s);
    for (int v0 = 0; v0 < V; v0 += SUPPORT_MAX_VIEWS) {
        const int nv = std::min(SUPPORT_MAX_VIEWS, V - v0);
        hipLaunchKernelGGL(k_edge_support<GATED>, dim3(blocks, nv), dim3(SUPPORT_THREADS), 0, s, E, P, points, offsets, V, v0,
                           intr + 4 * (size_t)v0, w2c + 12 * (size_t)v0, height, width, d2 + (size_t)v0 * plane, T, tol2,
                           counts, GATED ? gate.depth + (size_t)v0 * plane : nullptr, gate.slack, hidden);
    }
}

void launch_edge_support(hipStream_t s, int E, int P, const float* points, const int* offsets, int V, const double* intr,
                         const double* w2c, int height, int width, const int* d2, int T, const int* tol2,
                         const DepthGate* gate, int* counts, int* hidden) {
    if (gate)
        edge_support_launches<true>(s, E, P, points, offsets, V, intr, w2c, height, width, d2, T, tol2, counts, *gate, hidden);
    else
        edge_support_launches<false>(s, E, P, points, offsets, V, intr, w2c, height, width, d2, T, tol2, counts,
                                     DepthGate{nullptr, 0.0}, nullptr);
}

}  // namespace cgs
