// Per-sample 2D support of extracted edges (include/curvegs.h, cgs_sample_support): how many views see every sample of the
// edges, and in how many of those it lands within a tolerance of a detected edge pixel -- the reduction of edge_support.hip
// the other way round (per sample over the views, where k_edge_support reduces per (edge, view) over the samples).
//   k_sample_support   one thread per sample, the view loop inside the thread: the view index is wave-uniform, so the 16
//                      doubles of a camera are scalar loads, and a wave's 64 consecutive samples -- neighbours on their edge
//                      -- gather neighbouring pixels of one plane.  The point is read once (12 consecutive bytes per lane),
//                      projected with nv_project_xyz (point_projection.h, the device function of cgs_edge_support and
//                      cgs_point_mask).  1 + T sums stay in registers; at the end the thread adds them to its own row of
//                      the tally.  No atomics, no LDS, no barrier: integers only and one owner per row, so the result does
//                      not depend on the launch geometry.  The loop takes any number of views: one launch per call.
//                      A template over GATED: false is cgs_sample_support as it always was (depth, slack and hidden are not
//                      read); true is cgs_sample_support_depth -- nv_verdict (point_projection.h) counts a view whose depth
//                      plane hides the sample in a sixth sum instead of `seen`, one float32 gather more per seeing view.
#include "kernels.h"
#include "point_projection.h"

namespace cgs {

constexpr int TRIM_THREADS = 256;
static_assert(CGS_EDGE_SUPPORT_MAX_TOL == 4, "the kernel keeps 1 + 4 sums in registers");

template <bool GATED>
__global__ void __launch_bounds__(TRIM_THREADS) k_sample_support(int P, const float* __restrict__ pts, int V,
                                                                 const double* __restrict__ intr,
                                                                 const double* __restrict__ w2c, int height, int width,
                                                                 const int* __restrict__ d2, int T,
                                                                 const int* __restrict__ tol2, int* __restrict__ tally,
                                                                 const float* __restrict__ depth, double slack,
                                                                 int* __restrict__ hidden) {
    constexpr int MT = CGS_EDGE_SUPPORT_MAX_TOL;
    const long long i = (long long)blockIdx.x * TRIM_THREADS + threadIdx.x;
    if (i >= P) return;   // the kernel has no barrier
    int t2[MT];
#pragma unroll
    for (int t = 0; t < MT; t++) t2[t] = t < T ? tol2[t] : -1;   // a distance is >= 0: an unused slot counts nothing
    const double X = (double)pts[3 * i + 0], Y = (double)pts[3 * i + 1], Z = (double)pts[3 * i + 2];
    const double wd = (double)width, hd = (double)height;
    const size_t plane = (size_t)height * (size_t)width;
    int seen = 0, hid = 0, near[MT];
#pragma unroll
    for (int t = 0; t < MT; t++) near[t] = 0;
    for (int view = 0; view < V; view++) {   // wave-uniform
        NvCam c;
        nv_load_cam(c, intr, w2c, view);
        double u, v;
        const NvVerdict verdict = nv_verdict<GATED>(c, X, Y, Z, wd, hd, GATED ? depth + (size_t)view * plane : nullptr, width,
                                                    slack, u, v);
        if (verdict == NV_OUT) continue;
        if (GATED && verdict == NV_HIDDEN) {
            hid++;
            continue;
        }
        // 0 <= u < W, so 0 <= floor(u) <= W - 1 (likewise v): the pixel is inside the view's plane
        const int d = d2[(size_t)view * plane + (size_t)floor(v) * (size_t)width + (size_t)floor(u)];
        seen++;
#pragma unroll
        for (int t = 0; t < MT; t++) near[t] += d <= t2[t] ? 1 : 0;
    }
    int* __restrict__ out = tally + (size_t)i * (size_t)(1 + T);   // the thread's own row: a plain read-modify-write
    out[0] += seen;
#pragma unroll
    for (int t = 0; t < MT; t++)
        if (t < T) out[1 + t] += near[t];
    if (GATED && hidden) hidden[i] += hid;   // added, like the tally: the thread's own word
}

template <bool GATED>
static void sample_support_launch(hipStream_t s, int P, const float* points, int V, const double* intr, const double* w2c,
                                  int height, int width, const int* d2, int T, const int* tol2, int* tally, DepthGate gate,
                                  int* hidden) {
    const unsigned blocks = (unsigned)(((long long)P + TRIM_THREADS - 1) / TRIM_THREADS);   // at most 2^23: one grid dimension
    ProfScope p(GATED ? "sample_support_depth" : "sample_support", s);
    hipLaunchKernelGGL(k_sample_support<GATED>, dim3(blocks), dim3(TRIM_THREADS), 0, s, P, points, V, intr, w2c, height, width,
                       d2, T, tol2, tally, gate.depth, gate.slack, hidden);
}

void launch_sample_support(hipStream_t s, int P, const float* points, int V, const double* intr, const double* w2c,
                           int height, int width, const int* d2, int T, const int* tol2, const DepthGate* gate, int* tally,
                           int* hidden) {
    if (gate)
        sample_support_launch<true>(s, P, points, V, intr, w2c, height, width, d2, T, tol2, tally, *gate, hidden);
    else
        sample_support_launch<false>(s, P, points, V, intr, w2c, height, width, d2, T, tol2, tally, DepthGate{nullptr, 0.0},
                                     nullptr);
}

}  // namespace cgs
