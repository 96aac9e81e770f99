// Densification statistics (reference train.py:184-187): for every splat that the view rasterised (radii > 0)
//   max_radii2D[i]        = max(max_radii2D[i], radii[i])
//   xyz_gradient_accum[i] += |dL/dmeans2D[i][0:2]|
//   denom[i]              += 1
// in one pass over the splats, without the visible-index list the reference builds (a device-to-host sync) and without
// its ~10 gather / scatter launches.  Each splat is owned by one thread: no atomics, the result does not depend on the
// schedule.  Memory-bound: 4 B radii + 8 of the grad_stride floats + 3 x (4 B read + 4 B write) = ~36-40 B per splat.
#include <algorithm>

#include "kernels.h"

namespace cgs {

constexpr int DENSIFY_THREADS = 256;  // 4 waves
constexpr int DENSIFY_MAX_BLOCKS = 2048;

__global__ void __launch_bounds__(DENSIFY_THREADS) k_densification_stats(long long P, const int* __restrict__ radii,
                                                                         const float* __restrict__ grad, long long stride,
                                                                         float* __restrict__ max_radii,
                                                                         float* __restrict__ accum,
                                                                         float* __restrict__ denom,
                                                                         const unsigned int* __restrict__ skip_flag) {
    // a raised flag (bucket overflow of a replayed forward, the convention of k_adam_flat_dev) leaves every buffer as it is
    if (skip_flag && *skip_flag != 0u) return;
    for (long long i = (long long)blockIdx.x * DENSIFY_THREADS + threadIdx.x; i < P;
         i += (long long)gridDim.x * DENSIFY_THREADS) {
        const int r = radii[i];
        if (r <= 0) continue;
        const float gx = grad[i * stride], gy = grad[i * stride + 1];
        max_radii[i] = fmaxf(max_radii[i], (float)r);   // torch.max(float, int -> float): (float)r is exact below 2^24
        accum[i] += sqrtf(gx * gx + gy * gy);           // torch.norm over two elements, correctly rounded sqrt
        denom[i] += 1.f;
    }
}

void launch_densification_stats(hipStream_t s, long long P, const int* radii, const float* grad, long long stride,
                                float* max_radii, float* accum, float* denom, const unsigned int* skip_flag) {
    ProfScope pr("densification_stats", s);
    const int blocks = (int)std::min<long long>((P + DENSIFY_THREADS - 1) / DENSIFY_THREADS, DENSIFY_MAX_BLOCKS);
    hipLaunchKernelGGL(k_densification_stats, dim3(blocks), dim3(DENSIFY_THREADS), 0, s, P, radii, grad, stride, max_radii,
                       accum, denom, skip_flag);
}

}  // namespace cgs
