// Depth maps from a scan's own photographs (include/curvegs.h, cgs_stereo_sweep / cgs_stereo_consistency): plane-sweep
// stereo.  The rule is frozen in the header and stated once, in stereo_depth.h; the geometry below is free, because every
// output is one plain store of a value that does not depend on it.
//   k_stereo_sweep         grid (tiles, views), a 16 x 16 tile of reference pixels per 256-thread workgroup, one thread per
//                          pixel with the hypotheses, the sources and the taps inside.  The tile's bytes plus a halo of the
//                          patch radius are staged ONCE in LDS as bytes, with the columns' and rows' ray slopes
//                          ((px - cx) / fx, (py - cy) / fy: two float64 divisions a tap otherwise) beside them as doubles;
//                          sr / srr are summed once per pixel.  The view is blockIdx.y, so a hypothesis' depth, a source's
//                          pose and intrinsics are uniform loads.  The source bytes are gathered from global memory: the
//                          four bytes of a bilinear footprint, neighbouring lanes reading neighbouring footprints; the
//                          views of a run stay in the Infinity Cache (100 views of 1600 x 1200 are 192 MB).  The winner
//                          and its two neighbours ride along the hypothesis loop in registers: no cost volume.
//                          The plain geometry -- the same thread per pixel reading everything from global memory -- is
//                          kept as a probe (profiles/probes/stereo_depth_geometries.hip; profiles/stereo_depth.md has
//                          the timings).
//   k_stereo_consistency   grid (pixel blocks, views), one thread per pixel.
// No atomics, no scratch memory, 64-bit offsets, no indexed private array.  Views beyond grid.y's limit go in runs.
#include <algorithm>

#include "kernels.h"
#include "stereo_depth.h"

namespace cgs {

constexpr int STEREO_TILE = 16;                              // the tile's side: 256 threads, 4 waves of 16 x 4 pixels
constexpr int STEREO_THREADS = STEREO_TILE * STEREO_TILE;
constexpr int STEREO_MAX_RADIUS = 8;                         // CGS_STEREO_MAX_RADIUS
constexpr int STEREO_SPAN = STEREO_TILE + 2 * STEREO_MAX_RADIUS;   // the staged tile's largest side
constexpr int STEREO_MAX_VIEWS = 65535;                      // views per launch: grid.y

// The reference pixel's numbers from the staged tile: the pointers are centred on the pixel.
struct StereoRefLds {
    const uint8_t* patch;
    int pitch;
    const double* dxs;
    const double* dys;
    __device__ double tap(int di, int dj) const { return (double)patch[di * pitch + dj]; }
    __device__ double dx(int dj) const { return dxs[dj]; }
    __device__ double dy(int di) const { return dys[di]; }
};

__global__ void __launch_bounds__(STEREO_THREADS) k_stereo_sweep(StereoArgs A, int v0, int tiles_x, float* __restrict__ depth) {
    __shared__ uint8_t s_bytes[STEREO_SPAN * STEREO_SPAN];
    __shared__ double s_dx[STEREO_SPAN], s_dy[STEREO_SPAN];
    const int v = v0 + (int)blockIdx.y, R = A.radius, span = STEREO_TILE + 2 * R;
    const int ty0 = ((int)blockIdx.x / tiles_x) * STEREO_TILE, tx0 = ((int)blockIdx.x % tiles_x) * STEREO_TILE;
    const size_t plane = (size_t)A.height * (size_t)A.width;
    const uint8_t* __restrict__ ref = A.gray + (size_t)v * plane;
    const double* f = A.intr + 4 * (size_t)v;
    for (int k = (int)threadIdx.x; k < span * span; k += STEREO_THREADS) {
        const int y = ty0 - R + k / span, x = tx0 - R + k % span;
        s_bytes[k] = (y >= 0 && y < A.height && x >= 0 && x < A.width) ? ref[(size_t)y * (size_t)A.width + (size_t)x] : (uint8_t)0;
    }
    if ((int)threadIdx.x < span) {
        StereoRefGlobal g{ref, A.width, ty0 - R + (int)threadIdx.x, tx0 - R + (int)threadIdx.x, f[0], f[1], f[2], f[3]};
        s_dx[threadIdx.x] = g.dx(0);   // column tx0 - R + k
        s_dy[threadIdx.x] = g.dy(0);   // row ty0 - R + k
    }
    __syncthreads();   // the only barrier: every thread of the workgroup reaches it
    const int ly = (int)threadIdx.x / STEREO_TILE, lx = (int)threadIdx.x % STEREO_TILE;
    const int i = ty0 + ly, j = tx0 + lx;
    if (i >= A.height || j >= A.width) return;
    float out = 0.0f;
    if (i - R >= 0 && i + R <= A.height - 1 && j - R >= 0 && j + R <= A.width - 1) {
        const StereoRefLds r{s_bytes + (ly + R) * span + (lx + R), span, s_dx + (lx + R), s_dy + (ly + R)};
        double sr, srr;
        stereo_ref_sums(r, R, sr, srr);
        out = stereo_sweep_pixel(A, v, r, sr, srr);
    }
    depth[(size_t)v * plane + (size_t)i * (size_t)A.width + (size_t)j] = out;
}

__global__ void __launch_bounds__(256) k_stereo_consistency(int V, int v0, int height, int width,
                                                            const float* __restrict__ depth, const double* __restrict__ intr,
                                                            int S, const int* __restrict__ src, const double* __restrict__ rel,
                                                            const double* __restrict__ tol, int min_consistent,
                                                            float* __restrict__ out) {
    const size_t plane = (size_t)height * (size_t)width;
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= plane) return;
    const int v = v0 + (int)blockIdx.y;
    out[(size_t)v * plane + p] = stereo_consistent_pixel(depth, intr, src, rel, tol, V, height, width, S, min_consistent, v,
                                                         (int)(p / (size_t)width), (int)(p % (size_t)width));
}

void launch_stereo_sweep(hipStream_t s, int V, int height, int width, const uint8_t* gray, const double* intr, int D,
                         const double* inv, int S, const int* src, const double* rel, int radius, double min_var,
                         double max_cost, int min_sources, float* depth) {
    const double n = (double)((2 * radius + 1) * (2 * radius + 1));
    const StereoArgs A{gray, intr, inv, src, rel, V, height, width, D, S, radius, min_sources, (min_var * n) * n, max_cost};
    const int tiles_x = (width + STEREO_TILE - 1) / STEREO_TILE, tiles_y = (height + STEREO_TILE - 1) / STEREO_TILE;
    ProfScope p("stereo_sweep", s);
    for (int v0 = 0; v0 < V; v0 += STEREO_MAX_VIEWS)
        hipLaunchKernelGGL(k_stereo_sweep, dim3((unsigned)(tiles_x * tiles_y), std::min(STEREO_MAX_VIEWS, V - v0)),
                           dim3(STEREO_THREADS), 0, s, A, v0, tiles_x, depth);
}

void launch_stereo_consistency(hipStream_t s, int V, int height, int width, const float* depth, const double* intr, int S,
                               const int* src, const double* rel, const double* tol, int min_consistent, float* out) {
    const size_t plane = (size_t)height * (size_t)width;
    ProfScope p("stereo_consistency", s);
    for (int v0 = 0; v0 < V; v0 += STEREO_MAX_VIEWS)
        hipLaunchKernelGGL(k_stereo_consistency, dim3((unsigned)((plane + 255) / 256), std::min(STEREO_MAX_VIEWS, V - v0)),
                           dim3(256), 0, s, V, v0, height, width, depth, intr, S, src, rel, tol, min_consistent, out);
}

}  // namespace cgs
