// Occlusion for the 2D operators (include/curvegs.h, cgs_mesh_depth / cgs_depth_window_max / cgs_point_mask_depth): a
// triangle mesh rendered into one camera-z plane per view, the plane widened by a window maximum, and the prediction mask of
// edge_score.hip gated by it.  The rules are frozen in the header; the geometry below is free.
//   k_mesh_depth        grid (triangles / 4, views), one wave per (triangle, view).  The view is blockIdx.y, so the camera's 16
//                       doubles are uniform loads; every lane projects the triangle's three vertices (nine floats, the same
//                       address for the whole wave) and the lanes then stride over the pixels of the bounding box in row-major
//                       order, 64 at a time.  The rule itself -- set-up, coverage, depth, the integer atomicMin on the
//                       float's bits behind a plain read -- is mesh_depth.h.  A minimum does not depend on the order of its
//                       operands: the plane is the same for every launch geometry and every order of the triangles.  The
//                       other geometry, one THREAD per (triangle, view), is kept as a probe: on a mesh of triangles of a few
//                       pixels it takes 5.5 ms where this one takes 7.4, on 12 triangles that fill the image 1.26 s
//                       against 21 ms (profiles/edge_occlusion.md) -- this one has no bad case.  k_mesh_depth<true> is
//                       cgs_mesh_depth_clipped: the same wave rasterises the one or two pieces that the plane c2 == near
//                       leaves of its triangle, one after the other (profiles/edge_clip.md).
//   k_depth_window_max  grid (tiles of 64 x 16, 1, views), one pass: the tile and its halo staged in LDS (pixels outside the
//                       image as -inf: they never win, which is the clipping), the row maximum into a second LDS array, the
//                       column maximum out.  A maximum is exact, so the separable form is the window's maximum to the bit.
//                       Both barriers are reached by every thread; every output word is written by its one owner.
//   k_point_mask_depth  k_point_mask with the gate: nv_project_xyz_depth decides SEEN, nv_hidden decides HIDDEN.
// No floating-point atomics, no scratch memory, 64-bit offsets.
#include <algorithm>

#include "kernels.h"
#include "mesh_depth.h"

namespace cgs {

constexpr int OCC_THREADS = 256;            // 4 waves
constexpr int OCC_WAVES = OCC_THREADS / 64;
constexpr int OCC_MAX_VIEWS = 65535;        // views per launch: grid.y / grid.z
constexpr int OCC_POINT_BLOCKS_MAX = 1024;
constexpr int OCC_TILE_W = 64, OCC_TILE_H = 16;
constexpr int OCC_HALO = CGS_DEPTH_MAX_WINDOW;

// ------------------------------------------------------------------------------------------------ z-buffer
// The wave's 64 lanes over the candidate pixels of one set-up triangle (or clipped piece), row-major, 64 at a time.
__device__ inline void mesh_tri_raster(const MeshTri& t, int height, int width, unsigned int* __restrict__ depth) {
    const unsigned int bw = (unsigned int)(t.jhi - t.jlo + 1);
    const unsigned int n = bw * (unsigned int)(t.ihi - t.ilo + 1);   // at most 2^28
    unsigned int* __restrict__ plane = depth + (size_t)blockIdx.y * (size_t)height * (size_t)width;
    for (unsigned int idx = threadIdx.x & 63; idx < n; idx += 64) {
        const unsigned int r = idx / bw;
        mesh_tri_pixel(t, t.ilo + (int)r, t.jlo + (int)(idx - r * bw), plane, width);
    }
}

// CLIP = false is cgs_mesh_depth and reads no `near`; CLIP = true is cgs_mesh_depth_clipped: the triangle's one or two
// pieces in front of the plane c2 == near (mesh_depth.h), rasterised one after the other.  The classification is uniform
// over the wave -- every lane holds the same nine floats -- so nothing diverges, and there is still no barrier.
template <bool CLIP>
__global__ void __launch_bounds__(OCC_THREADS) k_mesh_depth(int F, const float* __restrict__ tris,
                                                           const double* __restrict__ intr,
                                                           const double* __restrict__ w2c, int height, int width,
                                                           double near, unsigned int* __restrict__ depth) {
    const long long f = (long long)blockIdx.x * OCC_WAVES + (threadIdx.x >> 6);
    if (f >= F) return;   // (uniform over the wave; no barrier in this kernel)
    NvCam c;
    nv_load_cam(c, intr, w2c, blockIdx.y);
    MeshTri t;
    if constexpr (!CLIP) {
        if (!mesh_tri_setup(c, tris + 9 * f, height, width, t)) return;   // (uniform)
        mesh_tri_raster(t, height, width, depth);
    } else {
        const float* __restrict__ p = tris + 9 * f;
        CamPt v[3], q[4];
#pragma unroll
        for (int k = 0; k < 3; k++)
            nv_camera_xyz(c, (double)p[3 * k + 0], (double)p[3 * k + 1], (double)p[3 * k + 2], v[k].x, v[k].y, v[k].z);
        const int pieces = mesh_tri_clip(v[0], v[1], v[2], near, q);   // (uniform)
        for (int k = 0; k < pieces; k++) {   // piece 0 is (q0, q1, q2), piece 1 (q0, q2, q3): selects, one rasteriser body
            const CamPt b = k == 0 ? q[1] : q[2], d = k == 0 ? q[2] : q[3];
            if (mesh_tri_setup_cam(c, q[0], b, d, height, width, t)) mesh_tri_raster(t, height, width, depth);
        }
    }
}

// ------------------------------------------------------------------------------------------------ window maximum
__global__ void __launch_bounds__(OCC_THREADS) k_depth_window_max(int height, int width, int radius,
                                                                 const float* __restrict__ depth,
                                                                 float* __restrict__ out) {
    __shared__ float s_in[OCC_TILE_H + 2 * OCC_HALO][OCC_TILE_W + 2 * OCC_HALO];
    __shared__ float s_row[OCC_TILE_H + 2 * OCC_HALO][OCC_TILE_W];
    const size_t base = (size_t)blockIdx.z * (size_t)height * (size_t)width;
    const int tiles_x = (width + OCC_TILE_W - 1) / OCC_TILE_W;
    const int x0 = (int)(blockIdx.x % (unsigned)tiles_x) * OCC_TILE_W, y0 = (int)(blockIdx.x / (unsigned)tiles_x) * OCC_TILE_H;
    const int sw = OCC_TILE_W + 2 * radius, sh = OCC_TILE_H + 2 * radius;
    const float ninf = -__uint_as_float(DEPTH_INF_BITS);
    for (int k = threadIdx.x; k < sw * sh; k += OCC_THREADS) {
        const int sy = k / sw, sx = k - sy * sw;
        const int y = y0 + sy - radius, x = x0 + sx - radius;
        s_in[sy][sx] = (y >= 0 && y < height && x >= 0 && x < width) ? depth[base + (size_t)y * (size_t)width + (size_t)x] : ninf;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < OCC_TILE_W * sh; k += OCC_THREADS) {
        const int sy = k / OCC_TILE_W, sx = k - sy * OCC_TILE_W;
        float m = ninf;
        for (int d = 0; d <= 2 * radius; d++) {
            const float a = s_in[sy][sx + d];
            m = a > m ? a : m;
        }
        s_row[sy][sx] = m;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < OCC_TILE_W * OCC_TILE_H; k += OCC_THREADS) {
        const int ty = k / OCC_TILE_W, tx = k - ty * OCC_TILE_W;
        const int y = y0 + ty, x = x0 + tx;
        if (y >= height || x >= width) continue;
        float m = ninf;
        for (int d = 0; d <= 2 * radius; d++) {
            const float a = s_row[ty + d][tx];
            m = a > m ? a : m;
        }
        out[base + (size_t)y * (size_t)width + (size_t)x] = m;
    }
}

// ------------------------------------------------------------------------------------------------ gated point mask
__global__ void __launch_bounds__(OCC_THREADS) k_point_mask_depth(int P, const float* __restrict__ pts,
                                                                 const double* __restrict__ intr,
                                                                 const double* __restrict__ w2c, int height, int width,
                                                                 const float* __restrict__ depth, double slack,
                                                                 uint8_t* __restrict__ mask, int* __restrict__ kept,
                                                                 int* __restrict__ hidden) {
    const int view = blockIdx.y;
    NvCam c;
    nv_load_cam(c, intr, w2c, view);
    const double wd = (double)width, hd = (double)height;
    const size_t off = (size_t)view * (size_t)height * (size_t)width;
    uint8_t* __restrict__ plane = mask + off;
    const float* __restrict__ dplane = depth + off;
    int n = 0, h = 0;
    for (long long i = (long long)blockIdx.x * OCC_THREADS + threadIdx.x; i < P; i += (long long)gridDim.x * OCC_THREADS) {
        double u, v, c2;
        if (!nv_project_xyz_depth(c, (double)pts[3 * i + 0], (double)pts[3 * i + 1], (double)pts[3 * i + 2], wd, hd, u, v, c2))
            continue;
        if (nv_hidden(dplane, width, u, v, c2, slack)) {
            h++;
            continue;
        }
        // 0 <= u < W, so 0 <= floor(u) <= W - 1 (likewise v): the pixel is inside the view's plane
        plane[(size_t)floor(v) * (size_t)width + (size_t)floor(u)] = 1;
        n++;
    }
#pragma unroll
    for (int off2 = 32; off2 >= 1; off2 >>= 1) {
        n += __shfl_xor(n, off2, 64);
        h += __shfl_xor(h, off2, 64);
    }
    if ((threadIdx.x & 63) != 0) return;
    if (kept && n) atomicAdd(&kept[view], n);
    if (hidden && h) atomicAdd(&hidden[view], h);
}

// ------------------------------------------------------------------------------------------------ launchers
template <bool CLIP>
static hipError_t mesh_depth_launches(hipStream_t s, int F, const float* tris, int V, const double* intr, const double* w2c,
                                      int height, int width, double near, float* depth) {
    const size_t plane = (size_t)height * (size_t)width;
    hipError_t e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(depth), (int)DEPTH_INF_BITS, (size_t)V * plane, s);
    if (e != hipSuccess || F == 0) return e;
    const unsigned blocks = (unsigned)(((long long)F + OCC_WAVES - 1) / OCC_WAVES);
    ProfScope p(CLIP ? "mesh_depth_clipped" : "mesh_depth", s);
    for (int v0 = 0; v0 < V; v0 += OCC_MAX_VIEWS) {
        const int nv = std::min(OCC_MAX_VIEWS, V - v0);
        hipLaunchKernelGGL(k_mesh_depth<CLIP>, dim3(blocks, nv), dim3(OCC_THREADS), 0, s, F, tris, intr + 4 * (size_t)v0,
                           w2c + 12 * (size_t)v0, height, width, near,
                           reinterpret_cast<unsigned int*>(depth) + (size_t)v0 * plane);
    }
    return hipSuccess;
}

hipError_t launch_mesh_depth(hipStream_t s, int F, const float* tris, int V, const double* intr, const double* w2c,
                             int height, int width, const double* near, float* depth) {
    return near ? mesh_depth_launches<true>(s, F, tris, V, intr, w2c, height, width, *near, depth)
                : mesh_depth_launches<false>(s, F, tris, V, intr, w2c, height, width, 0.0, depth);
}

void launch_depth_window_max(hipStream_t s, int V, int height, int width, int radius, const float* depth, float* out) {
    const size_t plane = (size_t)height * (size_t)width;
    const unsigned tiles = (unsigned)((width + OCC_TILE_W - 1) / OCC_TILE_W) * (unsigned)((height + OCC_TILE_H - 1) / OCC_TILE_H);
    ProfScope p("depth_window_max", s);
    for (int v0 = 0; v0 < V; v0 += OCC_MAX_VIEWS) {
        const int nv = std::min(OCC_MAX_VIEWS, V - v0);
        hipLaunchKernelGGL(k_depth_window_max, dim3(tiles, 1, nv), dim3(OCC_THREADS), 0, s, height, width, radius,
                           depth + (size_t)v0 * plane, out + (size_t)v0 * plane);
    }
}

hipError_t launch_point_mask_depth(hipStream_t s, int P, const float* points, int V, const double* intr, const double* w2c,
                                   int height, int width, const float* depth, double slack, uint8_t* mask, int* kept,
                                   int* hidden) {
    const size_t plane = (size_t)height * (size_t)width;
    hipError_t e = hipMemsetAsync(mask, 0, (size_t)V * plane, s);
    if (e != hipSuccess) return e;
    if (kept && (e = hipMemsetAsync(kept, 0, (size_t)V * sizeof(int), s)) != hipSuccess) return e;
    if (hidden && (e = hipMemsetAsync(hidden, 0, (size_t)V * sizeof(int), s)) != hipSuccess) return e;
    if (P == 0) return hipSuccess;
    const int blocks = std::max(1, (int)std::min<long long>(OCC_POINT_BLOCKS_MAX, ((long long)P + OCC_THREADS - 1) / OCC_THREADS));
    ProfScope p("point_mask_depth", s);
    for (int v0 = 0; v0 < V; v0 += OCC_MAX_VIEWS) {
        const int nv = std::min(OCC_MAX_VIEWS, V - v0);
        hipLaunchKernelGGL(k_point_mask_depth, dim3(blocks, nv), dim3(OCC_THREADS), 0, s, P, points, intr + 4 * (size_t)v0,
                           w2c + 12 * (size_t)v0, height, width, depth + (size_t)v0 * plane, slack, mask + (size_t)v0 * plane,
                           kept ? kept + v0 : nullptr, hidden ? hidden + v0 : nullptr);
    }
    return hipSuccess;
}

}  // namespace cgs
