// Occlusion from an oriented point cloud (include/curvegs.h, cgs_surfel_depth): every point drawn as a disk -- a surfel --
// into the camera-z planes that cgs_mesh_depth draws a mesh into.  The rule is frozen in the header and stated once, in
// surfel_depth.h; the geometry below is free.
//   k_surfel_depth   grid (surfels / 4, views), one wave per (surfel, view) -- k_mesh_depth's shape.  The view is blockIdx.y,
//                    so the camera's 16 doubles are uniform loads; every lane sets up the wave's surfel (seven floats, the
//                    same addresses for the whole wave) and the lanes then stride over the pixels of its candidate box in
//                    row-major order, 64 at a time.  The store is the z-buffer's: a plain read, then the integer atomicMin on
//                    the float's bits; a minimum does not depend on the order of its operands, so the plane is the same for
//                    every launch geometry and every order of the points.  This is the geometry with no bad case, not the
//                    fastest on a real cloud: 2 million disks of a few pixels in 100 views of 1600 x 1200 take 104 ms here and
//                    25.2 ms with a LANE per (surfel, view), whether or not the boxes too large for a lane are handed to the
//                    whole wave (the hybrid, k_mesh_contours' shape).  But one stray point near a camera covers a whole image,
//                    and a lane alone then walks two million pixels: 100 such disks among the 2 million make it 3.2 s (261 ms
//                    here, 88 ms in the hybrid).  The hybrid was to ship only if it is behind neither pure geometry on that
//                    geometry's own cloud by more than the rounds of a run spread, and it is: by 330 ms of 387 on 1000
//                    image-filling disks, which a lane per surfel packs into 16 waves a view (level once small launches go
//                    to this kernel instead), and by 0.015 ms of 25.18 on the small disks, three times the spread of 0.005
//                    -- the ballot that a lane-per-surfel kernel needs to be safe is not free.  So this kernel ships and
//                    the other two are kept as probes (profiles/probes/surfel_depth_geometries.hip;
//                    profiles/surfel_depth.md has every timing and what a follow-up would gain).
// No LDS, no barrier, no floating-point atomics, no scratch memory, 64-bit offsets, no indexed private array.
#include <algorithm>

#include "kernels.h"
#include "surfel_depth.h"

namespace cgs {

constexpr int SURFEL_THREADS = 256;         // 4 waves
constexpr int SURFEL_WAVES = SURFEL_THREADS / 64;
constexpr int SURFEL_MAX_VIEWS = 65535;     // views per launch: grid.y

__global__ void __launch_bounds__(SURFEL_THREADS) k_surfel_depth(int P, const float* __restrict__ points,
                                                                const float* __restrict__ normals,
                                                                const float* __restrict__ radii,
                                                                const double* __restrict__ intr,
                                                                const double* __restrict__ w2c, int height, int width,
                                                                unsigned int* __restrict__ depth) {
    const long long p = (long long)blockIdx.x * SURFEL_WAVES + (threadIdx.x >> 6);
    if (p >= P) return;   // (uniform over the wave; no barrier in this kernel)
    NvCam c;
    nv_load_cam(c, intr, w2c, blockIdx.y);
    Surfel f;
    if (!surfel_setup(c, points + 3 * (size_t)p, normals ? normals + 3 * (size_t)p : nullptr, radii[p], height, width, f))
        return;           // (uniform)
    surfel_draw_wave(c, f, threadIdx.x & 63, depth + (size_t)blockIdx.y * (size_t)height * (size_t)width, width);
}

hipError_t launch_surfel_depth(hipStream_t s, int P, const float* points, const float* normals, const float* radii, int V,
                               const double* intr, const double* w2c, int height, int width, float* depth) {
    const size_t plane = (size_t)height * (size_t)width;
    hipError_t e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(depth), (int)DEPTH_INF_BITS, (size_t)V * plane, s);
    if (e != hipSuccess || P == 0) return e;
    const unsigned blocks = (unsigned)(((long long)P + SURFEL_WAVES - 1) / SURFEL_WAVES);
    ProfScope p("surfel_depth", s);
    for (int v0 = 0; v0 < V; v0 += SURFEL_MAX_VIEWS) {
        const int nv = std::min(SURFEL_MAX_VIEWS, V - v0);
        hipLaunchKernelGGL(k_surfel_depth, dim3(blocks, nv), dim3(SURFEL_THREADS), 0, s, P, points, normals, radii,
                           intr + 4 * (size_t)v0, w2c + 12 * (size_t)v0, height, width,
                           reinterpret_cast<unsigned int*>(depth) + (size_t)v0 * plane);
    }
    return hipSuccess;
}

}  // namespace cgs
