// The launch geometry of cgs_tsdf_integrate that did not ship, kept to be measured beside the library's kernel
// (profiles/probes/tsdf_mesh.py --geometry_lib; profiles/tsdf_mesh.md).  The rule is csrc/tsdf.h's, so the state is the
// library's bit for bit, which the probe checks before it times anything.
//   k_tsdf_integrate_linear   the geometry of k_voxel_votes<true> (edge_seed.hip), the baseline: one thread per lattice
//                             point in linear order, x fastest, so a wave is a run of 64 points along x and its footprint
//                             in a view is a line, where the library's wave is an 8 x 8 slab of a brick.  The same view
//                             loop, scalar camera loads, registers only.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -munsafe-fp-atomics -fno-slp-vectorize
//        -I curve_gaussian_amd/csrc -I include profiles/probes/tsdf_geometries.hip -o profiles/probes/libtsdf_probe.so
#include <hip/hip_runtime.h>

#include "tsdf.h"

namespace cgs {

__global__ void __launch_bounds__(256) k_tsdf_integrate_linear(const SeedGrid g, const TsdfViews s, double trunc, int accumulate,
                                                               double* __restrict__ sum, unsigned short* __restrict__ weight) {
    const long long n = (long long)g.nx * g.ny * g.nz;   // <= 2^31 - 1
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    if (id >= n) return;
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
    for (int v = 0; v < s.V; v++) {
        NvCam c;
        nv_load_cam(c, s.intr, s.w2c, v);
        tsdf_observe(c, X, Y, Z, wd, hd, s.depth + (size_t)v * image, s.width, trunc, acc, w);
    }
    sum[id] = acc;
    weight[id] = (unsigned short)w;
}

}  // namespace cgs

// cgs_tsdf_integrate's arguments, unchecked but for what keeps the launch inside its buffers: the probe passes what the
// library's entry has already accepted.
extern "C" int probe_tsdf_integrate_linear(int nx, int ny, int nz, const double* lo, const double* step, int V, const double* intr,
                                           const double* w2c, int height, int width, const float* depth, double trunc,
                                           int accumulate, double* sum, unsigned short* weight, void* stream) {
    using namespace cgs;
    if (nx < 1 || ny < 1 || nz < 1 || (long long)nx * ny * nz > 2147483647ll || V < 1 || height < 1 || width < 1 || !lo || !step ||
        !intr || !w2c || !depth || !sum || !weight || !(trunc > 0.0))
        return -1;
    const long long n = (long long)nx * ny * nz;
    hipLaunchKernelGGL(k_tsdf_integrate_linear, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       SeedGrid{{lo[0], lo[1], lo[2]}, {step[0], step[1], step[2]}, nx, ny, nz},
                       TsdfViews{V, height, width, intr, w2c, depth}, trunc, accumulate, sum, weight);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
