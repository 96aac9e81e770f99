// Fusing the stereo depth maps across views (include/curvegs.h, cgs_stereo_warp / cgs_stereo_fuse).  The rule is frozen in
// the header and stated once, in stereo_fuse.h; the geometry below is free: a warped pixel is the minimum of what lands
// on it, whatever the order, and a fused pixel is one plain store.
//   k_stereo_warp   grid (tiles, slots, targets), a 16 x 16 tile of SOURCE pixels per 256-thread workgroup, one thread per
//                   (target, slot, source pixel).  The target and the slot are blockIdx.z / .y, so the source's index, the
//                   pose and both intrinsics are uniform loads, and a slot without a source ends its workgroups at once.
//                   A wave is 16 x 4 neighbouring source pixels, which land on neighbouring target pixels: the read in
//                   front of the atomic touches a few rows' worth of cache lines.  A lane whose pixel has no depth leaves
//                   before any arithmetic.  The atomics are vector atomics (atomicMin on the float's bits).
//                   The other geometry -- a wave per source row segment with the slot loop inside -- is kept as a probe
//                   (profiles/probes/stereo_fuse_geometries.hip; profiles/stereo_fuse.md has the timings).
//   k_stereo_fuse   grid (pixel blocks, targets), one thread per target pixel: the own depth and the F planes read
//                   coalesced, the F + 1 candidates in registers, the O(F^2) support count unrolled.
// No scratch memory, 64-bit offsets, no indexed private array.  Targets beyond a grid dimension's limit go in runs.
#include <algorithm>

#include "kernels.h"
#include "stereo_fuse.h"

namespace cgs {

constexpr int FUSE_TILE = 16;                       // the tile's side: 256 threads, 4 waves of 16 x 4 source pixels
constexpr int FUSE_THREADS = FUSE_TILE * FUSE_TILE;
constexpr int FUSE_MAX_TARGETS = 65535;             // targets per launch: grid.z / grid.y

__global__ void __launch_bounds__(FUSE_THREADS) k_stereo_warp(int V, int t0, int v0, int height, int width, int tiles_x,
                                                              const float* __restrict__ depth, const double* __restrict__ intr,
                                                              int F, const int* __restrict__ fsrc,
                                                              const double* __restrict__ into, unsigned int* __restrict__ warped) {
    const int t = t0 + (int)blockIdx.z, v = v0 + t, s = (int)blockIdx.y;   // t: the target's place in the range
    const size_t vs = (size_t)v * (size_t)F + (size_t)s;
    const int w = fsrc[vs];
    if (w < 0 || w >= V) return;   // no source (uniform over the workgroup; no barrier in this kernel)
    const int i = ((int)blockIdx.x / tiles_x) * FUSE_TILE + (int)threadIdx.x / FUSE_TILE;
    const int j = ((int)blockIdx.x % tiles_x) * FUSE_TILE + (int)threadIdx.x % FUSE_TILE;
    if (i >= height || j >= width) return;
    const size_t plane = (size_t)height * (size_t)width;
    const float z = depth[(size_t)w * plane + (size_t)i * (size_t)width + (size_t)j];
    if (!stereo_is_depth(z)) return;
    NvCam c;
#pragma unroll
    for (int k = 0; k < 12; k++) c.m[k] = into[12 * vs + k];
#pragma unroll
    for (int k = 0; k < 4; k++) c.f[k] = intr[4 * (size_t)v + k];
    stereo_warp_pixel(z, intr + 4 * (size_t)w, c, height, width, i, j, warped + ((size_t)t * (size_t)F + (size_t)s) * plane);
}

__global__ void __launch_bounds__(256) k_stereo_fuse(int t0, int v0, int height, int width, const float* __restrict__ depth, int F,
                                                     const float* __restrict__ warped, const double* __restrict__ tol,
                                                     int min_support, float* __restrict__ out, uint8_t* __restrict__ support) {
    const size_t plane = (size_t)height * (size_t)width;
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= plane) return;
    const int t = t0 + (int)blockIdx.y, v = v0 + t;
    float o;
    uint8_t n;
    stereo_fuse_pixel(depth[(size_t)v * plane + p], warped + (size_t)t * (size_t)F * plane + p, plane, F, tol[v], min_support, o, n);
    out[(size_t)t * plane + p] = o;
    if (support) support[(size_t)t * plane + p] = n;
}

hipError_t launch_stereo_warp(hipStream_t s, int V, int height, int width, const float* depth, const double* intr, int F,
                              const int* fsrc, const double* into, int v0, int nv, float* warped) {
    const size_t plane = (size_t)height * (size_t)width;
    hipError_t e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(warped), (int)DEPTH_INF_BITS,
                                     (size_t)nv * (size_t)F * plane, s);
    if (e != hipSuccess) return e;
    const int tiles_x = (width + FUSE_TILE - 1) / FUSE_TILE, tiles_y = (height + FUSE_TILE - 1) / FUSE_TILE;
    ProfScope p("stereo_warp", s);
    for (int t0 = 0; t0 < nv; t0 += FUSE_MAX_TARGETS)
        hipLaunchKernelGGL(k_stereo_warp, dim3((unsigned)(tiles_x * tiles_y), (unsigned)F, std::min(FUSE_MAX_TARGETS, nv - t0)),
                           dim3(FUSE_THREADS), 0, s, V, t0, v0, height, width, tiles_x, depth, intr, F, fsrc, into,
                           reinterpret_cast<unsigned int*>(warped));
    return hipSuccess;
}

void launch_stereo_fuse(hipStream_t s, int height, int width, const float* depth, int F, const float* warped,
                        const double* tol, int min_support, int v0, int nv, float* out, uint8_t* support) {
    const size_t plane = (size_t)height * (size_t)width;
    ProfScope p("stereo_fuse", s);
    for (int t0 = 0; t0 < nv; t0 += FUSE_MAX_TARGETS)
        hipLaunchKernelGGL(k_stereo_fuse, dim3((unsigned)((plane + 255) / 256), std::min(FUSE_MAX_TARGETS, nv - t0)), dim3(256), 0,
                           s, t0, v0, height, width, depth, F, warped, tol, min_support, out, support);
}

}  // namespace cgs
