// The OTHER geometry of the mesh z-buffer, kept as a probe only (profiles/edge_occlusion.md): one THREAD per (triangle, view)
// that walks its whole bounding box, against k_mesh_depth (csrc/edge_occlusion.hip), where a wave shares one.  The rule is
// the same code (csrc/mesh_depth.h), so the planes are equal to the bit.  The call does NOT fill the planes with +inf.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -I curve_gaussian_amd/csrc -I include \
//         profiles/probes/edge_occlusion_thread.hip -o profiles/probes/libedge_occlusion_thread.so
// profiles/probes/edge_occlusion.py --thread_lib profiles/probes/libedge_occlusion_thread.so then checks it against the
// library's kernel and times both.
#include <algorithm>
#include <cstdint>

#include <hip/hip_runtime.h>

#include "mesh_depth.h"

namespace {

constexpr int THREADS = 256;
constexpr int MAX_VIEWS = 65535;   // views per launch: grid.y

__global__ void __launch_bounds__(THREADS) k_mesh_depth_thread(int F, const float* __restrict__ tris,
                                                              const double* __restrict__ intr,
                                                              const double* __restrict__ w2c, int height, int width,
                                                              unsigned int* __restrict__ depth) {
    const long long f = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (f >= F) return;
    cgs::NvCam c;
    cgs::nv_load_cam(c, intr, w2c, blockIdx.y);
    cgs::MeshTri t;
    if (!cgs::mesh_tri_setup(c, tris + 9 * f, height, width, t)) return;
    unsigned int* __restrict__ plane = depth + (size_t)blockIdx.y * (size_t)height * (size_t)width;
    for (int i = t.ilo; i <= t.ihi; i++)
        for (int j = t.jlo; j <= t.jhi; j++) cgs::mesh_tri_pixel(t, i, j, plane, width);
}

}  // namespace

extern "C" int mesh_depth_thread(int F, const float* tris, int V, const double* intr, const double* w2c, int height, int width,
                                 float* depth, void* stream) {
    if (F <= 0 || V <= 0 || height <= 0 || width <= 0) return -1;
    const size_t plane = (size_t)height * (size_t)width;
    const unsigned blocks = (unsigned)(((long long)F + THREADS - 1) / THREADS);
    for (int v0 = 0; v0 < V; v0 += MAX_VIEWS)
        hipLaunchKernelGGL(k_mesh_depth_thread, dim3(blocks, std::min(MAX_VIEWS, V - v0)), dim3(THREADS), 0, (hipStream_t)stream,
                           F, tris, intr + 4 * (size_t)v0, w2c + 12 * (size_t)v0, height, width,
                           reinterpret_cast<unsigned int*>(depth) + (size_t)v0 * plane);
    return hipGetLastError() == hipSuccess ? 0 : -3;
}
