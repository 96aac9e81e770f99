// The OTHER shape of the per-sample tally, kept as a probe only (profiles/edge_trim.md): the views in blockIdx.y, one thread
// per (sample, view) and integer atomicAdd into the sample's row, against k_sample_support (csrc/edge_trim.hip), which
// loops over the views inside the thread and owns its row.  Same contract: the call ADDS to the tally.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -I curve_gaussian_amd/csrc -I include \
//         profiles/probes/edge_trim_atomic.hip -o profiles/probes/libedge_trim_atomic.so
// profiles/probes/edge_trim.py --atomic_lib profiles/probes/libedge_trim_atomic.so then checks it against the library's
// kernel and times both.
#include <algorithm>
#include <cstdint>

#include <hip/hip_runtime.h>

#include "point_projection.h"

namespace {

constexpr int THREADS = 256;
constexpr int MAX_VIEWS = 65535;   // views per launch: grid.y
constexpr int MT = 4;

__global__ void __launch_bounds__(THREADS) k_sample_support_atomic(int P, const float* __restrict__ pts,
                                                                   const double* __restrict__ intr,
                                                                   const double* __restrict__ w2c, int height, int width,
                                                                   const int* __restrict__ d2, int T,
                                                                   const int* __restrict__ tol2, int* __restrict__ tally) {
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= P) return;
    const int view = blockIdx.y;
    cgs::NvCam c;
    cgs::nv_load_cam(c, intr, w2c, view);
    double u, v;
    if (!cgs::nv_project(c, pts, i, (double)width, (double)height, u, v)) return;
    const int d = d2[(size_t)view * (size_t)height * (size_t)width + (size_t)floor(v) * (size_t)width + (size_t)floor(u)];
    int* out = tally + (size_t)i * (size_t)(1 + T);
    atomicAdd(out, 1);
#pragma unroll
    for (int t = 0; t < MT; t++)
        if (t < T && d <= tol2[t]) atomicAdd(out + 1 + t, 1);
}

}  // namespace

extern "C" int sample_support_atomic(int P, const float* points, int V, const double* intr, const double* w2c, int height,
                                     int width, const int32_t* d2, int T, const int32_t* tol2, int32_t* tally, void* stream) {
    if (P <= 0 || V <= 0 || T < 1 || T > MT) return -1;
    const size_t plane = (size_t)height * (size_t)width;
    const unsigned blocks = (unsigned)(((long long)P + THREADS - 1) / THREADS);
    for (int v0 = 0; v0 < V; v0 += MAX_VIEWS)
        hipLaunchKernelGGL(k_sample_support_atomic, dim3(blocks, std::min(MAX_VIEWS, V - v0)), dim3(THREADS), 0,
                           (hipStream_t)stream, P, points, intr + 4 * (size_t)v0, w2c + 12 * (size_t)v0, height, width,
                           d2 + (size_t)v0 * plane, T, tol2, tally);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}
