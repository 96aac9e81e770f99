// The launch geometries of the surfel z-buffer side by side, as a probe only (profiles/surfel_depth.md): one THREAD per
// (surfel, view) that walks its whole candidate box, one WAVE per (surfel, view) that shares it -- what
// csrc/surfel_depth.hip ships --, and the hybrid -- a lane per (surfel, view), the boxes above a threshold drawn by the
// whole wave -- with the threshold as an argument.  The rule is the same code (csrc/surfel_depth.h), so the planes are
// equal to the bit.  The calls do NOT fill the planes with +inf.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -munsafe-fp-atomics -fno-slp-vectorize \
//         -I curve_gaussian_amd/csrc -I include profiles/probes/surfel_depth_geometries.hip \
//         -o profiles/probes/libsurfel_depth_geometries.so
// profiles/probes/surfel_depth.py --geometry_lib profiles/probes/libsurfel_depth_geometries.so then checks all of them
// against the library's kernel and times them.
#include <algorithm>
#include <cstdint>

#include <hip/hip_runtime.h>

#include "surfel_depth.h"

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int MAX_VIEWS = 65535;   // views per launch: grid.y

// One lane over its own surfel's box, row by row.
__device__ inline void surfel_draw_lane(const cgs::NvCam& c, const cgs::Surfel& f, unsigned int* __restrict__ plane, int width) {
    for (int i = f.ilo; i <= f.ihi; i++)
        for (int j = f.jlo; j <= f.jhi; j++) cgs::surfel_pixel(c, f, i, j, plane, width);
}

// Lane `src`'s value in every lane; src is uniform over the wave.
__device__ inline int wave_read(int x, int src) { return __builtin_amdgcn_readlane(x, src); }
__device__ inline double wave_read(double x, int src) {
    return __hiloint2double(wave_read(__double2hiint(x), src), wave_read(__double2loint(x), src));
}

// The hybrid: every lane of the wave arrives with its own surfel (`live` false: none, or skipped by the view; `mine` must
// hold initialised values either way).  A lane whose box has at most small_max pixels draws it itself; the boxes above that
// are found by a ballot and drawn by the whole wave one after the other, the set-up read from the owner's registers by the
// ballot's lane index, which is uniform (k_mesh_contours' shape).  No lane may have left the kernel before the call.
__device__ inline void surfel_draw_hybrid(const cgs::NvCam& c, const cgs::Surfel& mine, bool live, unsigned int small_max,
                                          int lane, unsigned int* __restrict__ plane, int width) {
    const bool large = live && cgs::surfel_box_pixels(mine) > small_max;
    if (live && !large) surfel_draw_lane(c, mine, plane, width);
    unsigned long long todo = __ballot(large);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        cgs::Surfel f;
        f.c0 = wave_read(mine.c0, src);
        f.c1 = wave_read(mine.c1, src);
        f.c2 = wave_read(mine.c2, src);
        f.n0 = wave_read(mine.n0, src);
        f.n1 = wave_read(mine.n1, src);
        f.n2 = wave_read(mine.n2, src);
        f.num = wave_read(mine.num, src);
        f.r2 = wave_read(mine.r2, src);
        f.jlo = wave_read(mine.jlo, src);
        f.jhi = wave_read(mine.jhi, src);
        f.ilo = wave_read(mine.ilo, src);
        f.ihi = wave_read(mine.ihi, src);
        cgs::surfel_draw_wave(c, f, lane, plane, width);
    }
}

__global__ void __launch_bounds__(THREADS) k_surfel_depth_thread(int P, const float* __restrict__ points,
                                                                const float* __restrict__ normals,
                                                                const float* __restrict__ radii,
                                                                const double* __restrict__ intr,
                                                                const double* __restrict__ w2c, int height, int width,
                                                                unsigned int* __restrict__ depth) {
    const long long p = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (p >= P) return;
    cgs::NvCam c;
    cgs::nv_load_cam(c, intr, w2c, blockIdx.y);
    cgs::Surfel f;
    if (!cgs::surfel_setup(c, points + 3 * (size_t)p, normals ? normals + 3 * (size_t)p : nullptr, radii[p], height, width, f))
        return;
    surfel_draw_lane(c, f, depth + (size_t)blockIdx.y * (size_t)height * (size_t)width, width);
}

__global__ void __launch_bounds__(THREADS) k_surfel_depth_wave(int P, const float* __restrict__ points,
                                                              const float* __restrict__ normals,
                                                              const float* __restrict__ radii,
                                                              const double* __restrict__ intr,
                                                              const double* __restrict__ w2c, int height, int width,
                                                              unsigned int* __restrict__ depth) {
    const long long p = (long long)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (p >= P) return;   // (uniform over the wave; no barrier in this kernel)
    cgs::NvCam c;
    cgs::nv_load_cam(c, intr, w2c, blockIdx.y);
    cgs::Surfel f;
    if (!cgs::surfel_setup(c, points + 3 * (size_t)p, normals ? normals + 3 * (size_t)p : nullptr, radii[p], height, width, f))
        return;           // (uniform)
    cgs::surfel_draw_wave(c, f, threadIdx.x & 63, depth + (size_t)blockIdx.y * (size_t)height * (size_t)width, width);
}

__global__ void __launch_bounds__(THREADS) k_surfel_depth_hybrid(int P, const float* __restrict__ points,
                                                                const float* __restrict__ normals,
                                                                const float* __restrict__ radii,
                                                                const double* __restrict__ intr,
                                                                const double* __restrict__ w2c, int height, int width,
                                                                unsigned int small_max, unsigned int* __restrict__ depth) {
    cgs::NvCam c;
    cgs::nv_load_cam(c, intr, w2c, blockIdx.y);
    const long long p = (long long)blockIdx.x * THREADS + threadIdx.x;
    cgs::Surfel mine = {0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 1.0, 0.0, 0, -1, 0, -1};
    const bool live = p < P && cgs::surfel_setup(c, points + 3 * (size_t)p, normals ? normals + 3 * (size_t)p : nullptr,
                                                 radii[p], height, width, mine);
    surfel_draw_hybrid(c, mine, live, small_max, threadIdx.x & 63,
                            depth + (size_t)blockIdx.y * (size_t)height * (size_t)width, width);
}

}  // namespace

// geometry: 0 thread, 1 wave, 2 hybrid (small_max: the largest box, in pixels, that a lane draws alone)
extern "C" int surfel_depth_geometry(int geometry, int P, const float* points, const float* normals, const float* radii, int V,
                                     const double* intr, const double* w2c, int height, int width, unsigned int small_max,
                                     float* depth, void* stream) {
    if (P <= 0 || V <= 0 || height <= 0 || width <= 0 || geometry < 0 || geometry > 2) return -1;
    const size_t plane = (size_t)height * (size_t)width;
    const int per_block = geometry == 1 ? WAVES : THREADS;
    const unsigned blocks = (unsigned)(((long long)P + per_block - 1) / per_block);
    for (int v0 = 0; v0 < V; v0 += MAX_VIEWS) {
        const dim3 grid(blocks, std::min(MAX_VIEWS, V - v0));
        const double* K = intr + 4 * (size_t)v0;
        const double* M = w2c + 12 * (size_t)v0;
        unsigned int* out = reinterpret_cast<unsigned int*>(depth) + (size_t)v0 * plane;
        if (geometry == 0)
            hipLaunchKernelGGL(k_surfel_depth_thread, grid, dim3(THREADS), 0, (hipStream_t)stream, P, points, normals, radii, K, M,
                               height, width, out);
        else if (geometry == 1)
            hipLaunchKernelGGL(k_surfel_depth_wave, grid, dim3(THREADS), 0, (hipStream_t)stream, P, points, normals, radii, K, M,
                               height, width, out);
        else
            hipLaunchKernelGGL(k_surfel_depth_hybrid, grid, dim3(THREADS), 0, (hipStream_t)stream, P, points, normals, radii, K, M,
                               height, width, small_max, out);
    }
    return hipGetLastError() == hipSuccess ? 0 : -3;
}
