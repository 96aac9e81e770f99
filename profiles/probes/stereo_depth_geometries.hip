// The launch geometry of cgs_stereo_sweep that did not ship, kept to be measured beside the library's kernel
// (profiles/probes/stereo_depth.py --geometry_lib; profiles/stereo_depth.md).  The rule is csrc/stereo_depth.h's, so the
// maps are the library's bit for bit, which the probe checks before it times anything.
//   k_stereo_sweep_plain   the library's grid and thread-to-pixel mapping -- (tiles, views), 16 x 16 pixels per 256-thread
//                          workgroup -- with nothing staged: a reference tap is a byte load from global memory each time it
//                          is used (once for sr / srr, then once per hypothesis and source), and the ray slopes
//                          (px - cx) / fx, (py - cy) / fy are divided out again at every tap.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -munsafe-fp-atomics -fno-slp-vectorize
//        -I curve_gaussian_amd/csrc -I include profiles/probes/stereo_depth_geometries.hip -o profiles/probes/libstereo_probe.so
#include <algorithm>

#include <hip/hip_runtime.h>

#include "stereo_depth.h"

namespace cgs {

constexpr int PROBE_TILE = 16;

__global__ void __launch_bounds__(PROBE_TILE* PROBE_TILE) k_stereo_sweep_plain(StereoArgs A, int v0, int tiles_x,
                                                                               float* __restrict__ depth) {
    const int v = v0 + (int)blockIdx.y, R = A.radius;
    const int i = ((int)blockIdx.x / tiles_x) * PROBE_TILE + (int)threadIdx.x / PROBE_TILE;
    const int j = ((int)blockIdx.x % tiles_x) * PROBE_TILE + (int)threadIdx.x % PROBE_TILE;
    if (i >= A.height || j >= A.width) return;
    const size_t plane = (size_t)A.height * (size_t)A.width;
    const double* f = A.intr + 4 * (size_t)v;
    float out = 0.0f;
    if (i - R >= 0 && i + R <= A.height - 1 && j - R >= 0 && j + R <= A.width - 1) {
        const StereoRefGlobal r{A.gray + (size_t)v * plane, A.width, i, j, f[0], f[1], f[2], f[3]};
        double sr, srr;
        stereo_ref_sums(r, R, sr, srr);
        out = stereo_sweep_pixel(A, v, r, sr, srr);
    }
    depth[(size_t)v * plane + (size_t)i * (size_t)A.width + (size_t)j] = out;
}

}  // namespace cgs

// cgs_stereo_sweep's arguments, unchecked: the probe passes what the library's entry has already accepted.
extern "C" int probe_stereo_sweep_plain(int V, int height, int width, const uint8_t* gray, const double* intr, int D,
                                        const double* inv, int S, const int* src, const double* rel, int radius, double min_var,
                                        double max_cost, int min_sources, float* depth, void* stream) {
    using namespace cgs;
    if (V <= 0 || height < 1 || width < 1 || D < 1 || S < 1 || radius < 0 || !gray || !intr || !inv || !src || !rel || !depth)
        return -1;
    const double n = (double)((2 * radius + 1) * (2 * radius + 1));
    const StereoArgs A{gray, intr, inv, src, rel, V, height, width, D, S, radius, min_sources, (min_var * n) * n, max_cost};
    const int tiles_x = (width + PROBE_TILE - 1) / PROBE_TILE, tiles_y = (height + PROBE_TILE - 1) / PROBE_TILE;
    for (int v0 = 0; v0 < V; v0 += 65535)
        hipLaunchKernelGGL(k_stereo_sweep_plain, dim3((unsigned)(tiles_x * tiles_y), std::min(65535, V - v0)),
                           dim3(PROBE_TILE * PROBE_TILE), 0, (hipStream_t)stream, A, v0, tiles_x, depth);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
