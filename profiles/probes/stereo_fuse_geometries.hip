// The launch geometry of cgs_stereo_warp that did not ship, kept to be measured beside the library's kernel
// (profiles/probes/stereo_fuse.py --geometry_lib; profiles/stereo_fuse.md).  The rule is csrc/stereo_fuse.h's, so the
// warped planes are the library's bit for bit, which the probe checks before it times anything.
//   k_stereo_warp_rows   grid (row segments, targets), 256 threads over 256 row-major source pixel POSITIONS -- a wave is
//                        64 neighbouring pixels of one row (or the end of one and the start of the next) -- with the slot
//                        loop inside: a thread reads its position in every source of the target in turn.  F times fewer
//                        threads, and the target's intrinsics are loaded once per thread instead of once per slot; the
//                        landing pixels of a wave lie along one target row instead of a 16 x 4 patch.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -munsafe-fp-atomics -fno-slp-vectorize
//        -I curve_gaussian_amd/csrc -I include profiles/probes/stereo_fuse_geometries.hip -o profiles/probes/libfuse_probe.so
#include <algorithm>

#include <hip/hip_runtime.h>

#include "stereo_fuse.h"

namespace cgs {

__global__ void __launch_bounds__(256) k_stereo_warp_rows(int V, int t0, int v0, int height, int width,
                                                          const float* __restrict__ depth, const double* __restrict__ intr, int F,
                                                          const int* __restrict__ fsrc, const double* __restrict__ into,
                                                          unsigned int* __restrict__ warped) {
    const size_t plane = (size_t)height * (size_t)width;
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= plane) return;
    const int t = t0 + (int)blockIdx.y, v = v0 + t;
    const int i = (int)(p / (size_t)width), j = (int)(p % (size_t)width);
    NvCam c;
#pragma unroll
    for (int k = 0; k < 4; k++) c.f[k] = intr[4 * (size_t)v + k];
    for (int s = 0; s < F; s++) {
        const size_t vs = (size_t)v * (size_t)F + (size_t)s;
        const int w = fsrc[vs];
        if (w < 0 || w >= V) continue;   // (uniform)
        const float z = depth[(size_t)w * plane + p];
        if (!stereo_is_depth(z)) continue;
#pragma unroll
        for (int k = 0; k < 12; k++) c.m[k] = into[12 * vs + k];
        stereo_warp_pixel(z, intr + 4 * (size_t)w, c, height, width, i, j, warped + ((size_t)t * (size_t)F + (size_t)s) * plane);
    }
}

}  // namespace cgs

// cgs_stereo_warp's arguments, unchecked: the probe passes what the library's entry has already accepted.
extern "C" int probe_stereo_warp_rows(int V, int height, int width, const float* depth, const double* intr, int F, const int* fsrc,
                                      const double* into, int v0, int nv, float* warped, void* stream) {
    using namespace cgs;
    if (V <= 0 || height < 1 || width < 1 || F < 1 || F > STEREO_MAX_FUSE || v0 < 0 || nv < 1 || nv > V - v0 || !depth || !intr ||
        !fsrc || !into || !warped)
        return -1;
    const size_t plane = (size_t)height * (size_t)width;
    if (hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(warped), (int)DEPTH_INF_BITS, (size_t)nv * (size_t)F * plane,
                          (hipStream_t)stream) != hipSuccess)
        return -2;
    for (int t0 = 0; t0 < nv; t0 += 65535)
        hipLaunchKernelGGL(k_stereo_warp_rows, dim3((unsigned)((plane + 255) / 256), std::min(65535, nv - t0)), dim3(256), 0,
                           (hipStream_t)stream, V, t0, v0, height, width, depth, intr, F, fsrc, into,
                           reinterpret_cast<unsigned int*>(warped));
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
