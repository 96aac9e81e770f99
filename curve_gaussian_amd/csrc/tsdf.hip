// A truncated signed distance field from per-view depth maps, and its surface by marching tetrahedra (include/curvegs.h,
// cgs_tsdf_integrate / cgs_tsdf_mesh_count / cgs_tsdf_mesh_emit).  The rule is frozen in the header and stated once, in
// tsdf.h.  Three kernels:
//   k_tsdf_integrate   one thread per lattice point, one 256-thread workgroup per 8 x 8 x 4 BRICK of points: a wave is the
//                      8 x 8 slab of one z, so its footprint in a view is compact in both image directions and its 64
//                      gathers share cache lines.  The view loop is inside; the view index is wave-uniform, so the 16
//                      doubles of a camera are scalar loads.  One float32 gather per kept (point, view) pair.  The running
//                      sum and the weight stay in registers; one plain 64-bit and one plain 16-bit store at the end, behind
//                      a load of the thread's own pair with `accumulate`.  No atomics, no LDS, no barrier (a lane outside
//                      the lattice leaves at once): the result does not depend on the launch geometry, and a chunked walk
//                      continues the very sum a single call forms.  The geometry of k_voxel_votes<true> (edge_seed.hip) --
//                      a thread per point in linear order, a wave 64 neighbours along x -- was the baseline and measured
//                      4.4 times slower on 256^3 points x 100 views of 1600 x 1200 (20.1 against 4.5 ms); it is kept as a
//                      probe (profiles/probes/tsdf_geometries.hip; profiles/tsdf_mesh.md has the timings).
//   k_tsdf_count       one thread per cell, x fastest: the 8 corner pairs by plain loads, the case of each of the 6
//                      tetrahedra from the derived table in __constant__ memory, one uint8 store.
//   k_tsdf_emit        the same thread per cell, which finds its triangles again and writes them at its offset: the offsets
//                      carry the order, there is no atomic.  A cell whose range does not fit [0, T] writes nothing.
// No scratch memory, no indexed private array (every index into one is a compile-time constant after unrolling), 64-bit
// offsets.
#include "kernels.h"
#include "tsdf.h"

namespace cgs {

constexpr int TSDF_THREADS = 256;   // 4 waves

constexpr int TSDF_BRICK_X = 8, TSDF_BRICK_Y = 8, TSDF_BRICK_Z = 4;   // 256 points: a wave per z
static_assert(TSDF_BRICK_X * TSDF_BRICK_Y == 64 && TSDF_BRICK_X * TSDF_BRICK_Y * TSDF_BRICK_Z == TSDF_THREADS, "a brick is a workgroup");

__global__ void __launch_bounds__(TSDF_THREADS) k_tsdf_integrate(const SeedGrid g, const TsdfViews s, int bricks_x, int bricks_y,
                                                                double trunc, int accumulate, double* __restrict__ sum,
                                                                unsigned short* __restrict__ weight) {
    const int b = (int)blockIdx.x;   // < 2^31: there are no more bricks than points
    const int bx = b % bricks_x, by = (b / bricks_x) % bricks_y, bz = b / (bricks_x * bricks_y);
    const int t = (int)threadIdx.x;
    const int i = TSDF_BRICK_X * bx + (t & 7), j = TSDF_BRICK_Y * by + ((t >> 3) & 7), k = TSDF_BRICK_Z * bz + (t >> 6);
    if (i >= g.nx || j >= g.ny || k >= g.nz) return;   // the lattice's edge; the kernel has no barrier
    const long long id = (long long)i + (long long)g.nx * ((long long)j + (long long)g.ny * (long long)k);   // < nx ny nz
    double X, Y, Z;
    seed_centre(g, id, X, Y, Z);
    const double wd = (double)s.width, hd = (double)s.height;
    const size_t image = (size_t)s.height * (size_t)s.width;
    double acc = 0.0;
    unsigned int w = 0u;
    if (accumulate) {
        acc = sum[id];
        w = weight[id];
    }
    for (int v = 0; v < s.V; v++) {   // v is uniform: scalar loads of the camera
        NvCam c;
        nv_load_cam(c, s.intr, s.w2c, v);
        tsdf_observe(c, X, Y, Z, wd, hd, s.depth + (size_t)v * image, s.width, trunc, acc, w);
    }
    sum[id] = acc;
    weight[id] = (unsigned short)w;
}

__global__ void __launch_bounds__(TSDF_THREADS) k_tsdf_count(const SeedGrid g, long long cells,
                                                            const double* __restrict__ sum,
                                                            const unsigned short* __restrict__ weight,
                                                            unsigned int min_weight, uint8_t* __restrict__ counts) {
    const long long cell = (long long)blockIdx.x * TSDF_THREADS + threadIdx.x;
    if (cell >= cells) return;
    counts[cell] = (uint8_t)tsdf_cell<false>(g, sum, weight, min_weight, cell, 0, 0, nullptr);
}

__global__ void __launch_bounds__(TSDF_THREADS) k_tsdf_emit(const SeedGrid g, long long cells,
                                                           const double* __restrict__ sum,
                                                           const unsigned short* __restrict__ weight,
                                                           unsigned int min_weight, const long long* __restrict__ offsets,
                                                           long long T, float* __restrict__ tris) {
    const long long cell = (long long)blockIdx.x * TSDF_THREADS + threadIdx.x;
    if (cell >= cells) return;
    tsdf_cell<true>(g, sum, weight, min_weight, cell, offsets[cell], T, tris);
}

void launch_tsdf_integrate(hipStream_t s, SeedGrid g, TsdfViews views, double trunc, int accumulate, double* sum,
                           unsigned short* weight) {
    const int bricks_x = (g.nx + TSDF_BRICK_X - 1) / TSDF_BRICK_X, bricks_y = (g.ny + TSDF_BRICK_Y - 1) / TSDF_BRICK_Y;
    const int bricks_z = (g.nz + TSDF_BRICK_Z - 1) / TSDF_BRICK_Z;
    const long long bricks = (long long)bricks_x * bricks_y * bricks_z;   // <= nx ny nz <= 2^31 - 1
    ProfScope p("tsdf_integrate", s);
    hipLaunchKernelGGL(k_tsdf_integrate, dim3((unsigned)bricks), dim3(TSDF_THREADS), 0, s, g, views, bricks_x, bricks_y, trunc,
                       accumulate, sum, weight);
}

static long long tsdf_cells(const SeedGrid& g) { return (long long)(g.nx - 1) * (g.ny - 1) * (g.nz - 1); }

void launch_tsdf_count(hipStream_t s, SeedGrid g, const double* sum, const unsigned short* weight, int min_weight,
                       uint8_t* counts) {
    const long long cells = tsdf_cells(g);   // >= 1: the entry returns before an empty launch
    const unsigned blocks = (unsigned)((cells + TSDF_THREADS - 1) / TSDF_THREADS);
    ProfScope p("tsdf_mesh_count", s);
    hipLaunchKernelGGL(k_tsdf_count, dim3(blocks), dim3(TSDF_THREADS), 0, s, g, cells, sum, weight, (unsigned int)min_weight,
                       counts);
}

void launch_tsdf_emit(hipStream_t s, SeedGrid g, const double* sum, const unsigned short* weight, int min_weight,
                      const long long* offsets, long long T, float* tris) {
    const long long cells = tsdf_cells(g);
    const unsigned blocks = (unsigned)((cells + TSDF_THREADS - 1) / TSDF_THREADS);
    ProfScope p("tsdf_mesh_emit", s);
    hipLaunchKernelGGL(k_tsdf_emit, dim3(blocks), dim3(TSDF_THREADS), 0, s, g, cells, sum, weight, (unsigned int)min_weight,
                       offsets, T, tris);
}

}  // namespace cgs
