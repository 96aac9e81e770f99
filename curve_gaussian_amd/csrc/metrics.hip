// Held-out image metrics (reference train.py:321-376, training_report): for every view of a batch, in ONE launch,
//   sum |d| and sum d^2 in float64,  d = clamp(image, 0, 1) - clamp(gt_c, 0, 1)  (float32, as torch computes it)
// over the gt's channels (the one-channel render broadcast against a [Cg,H,W] gt, as l1_loss / psnr broadcast) and the
// columns x0 .. W-1 (train_test_exp's right half).  Deterministic: each view is cut into METRIC_BLOCKS fixed slices,
// every workgroup writes its partial sums, and the last workgroup of the view to finish (an integer counter decides which)
// adds the partials in index order.  The bits of a view depend on its own size only, never on the run or the batch.
#include <algorithm>
#include <cstring>
#include <vector>

#include "kernels.h"

namespace cgs {

constexpr int METRIC_BLOCKS = 64;    // workgroups per view
constexpr int METRIC_THREADS = 256;  // 4 waves

struct MetricWs {  // device workspace layout: the descriptor table and counters are copied in by every call
    static size_t counters_offset(int V) { return (size_t)V * sizeof(cgs_metric_view); }
    static size_t partials_offset(int V) { return (counters_offset(V) + (size_t)V * sizeof(unsigned int) + 15) & ~(size_t)15; }
    static size_t bytes(int V) { return partials_offset(V) + (size_t)V * METRIC_BLOCKS * 2 * sizeof(double); }
};

__device__ __forceinline__ float clamp01(float x) { return x < 0.f ? 0.f : (x > 1.f ? 1.f : x); }  // NaN stays NaN

__global__ void __launch_bounds__(METRIC_THREADS) k_view_metrics(const cgs_metric_view* __restrict__ views,
                                                                 unsigned int* __restrict__ counters,
                                                                 double* __restrict__ partials, double* __restrict__ sums,
                                                                 double* __restrict__ means) {
    const int v = blockIdx.y;
    const cgs_metric_view d = views[v];
    const int Wp = d.width - d.x0;
    const int64_t plane = (int64_t)d.height * Wp;
    const int64_t n = plane * d.channels;
    const int64_t HW = (int64_t)d.height * d.width;
    double a1 = 0.0, a2 = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * METRIC_THREADS + threadIdx.x; i < n; i += (int64_t)METRIC_BLOCKS * METRIC_THREADS) {
        const int64_t c = i / plane, r = i - c * plane;
        const int64_t y = r / Wp, x = r - y * Wp + d.x0;
        const float diff = clamp01(d.image[y * d.width + x]) - clamp01(d.gt[c * HW + y * d.width + x]);
        a1 += (double)fabsf(diff);
        a2 += (double)diff * (double)diff;   // exact: the product of two floats fits a double
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        a1 += __shfl_xor(a1, off, 64);
        a2 += __shfl_xor(a2, off, 64);
    }
    __shared__ double s_part[2][METRIC_THREADS / 64];
    if ((threadIdx.x & 63) == 0) { s_part[0][threadIdx.x >> 6] = a1; s_part[1][threadIdx.x >> 6] = a2; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double* mine = partials + ((size_t)v * METRIC_BLOCKS + blockIdx.x) * 2;
    mine[0] = ((s_part[0][0] + s_part[0][1]) + s_part[0][2]) + s_part[0][3];
    mine[1] = ((s_part[1][0] + s_part[1][1]) + s_part[1][2]) + s_part[1][3];
    __threadfence();
    if (atomicAdd(&counters[v], 1u) != METRIC_BLOCKS - 1) return;
    __threadfence();
    // the last workgroup of view v: every partial is visible; add them in index order (volatile: past the local cache)
    const volatile double* p = partials + (size_t)v * METRIC_BLOCKS * 2;
    double s1 = 0.0, s2 = 0.0;
    for (int b = 0; b < METRIC_BLOCKS; b++) {
        s1 += p[2 * b];
        s2 += p[2 * b + 1];
    }
    sums[2 * v] = s1;
    sums[2 * v + 1] = s2;
    if (means) {
        means[2 * v] = s1 / (double)n;
        means[2 * v + 1] = s2 / (double)n;
    }
}

size_t view_metrics_workspace_bytes(int n_views) { return MetricWs::bytes(n_views > 0 ? n_views : 1); }

hipError_t launch_view_metrics(hipStream_t s, int n_views, const cgs_metric_view* views_host, void* workspace,
                               double* sums, double* means) {
    // one host -> device copy of the descriptor table with zeroed counters, then one kernel
    const size_t head = MetricWs::partials_offset(n_views);
    std::vector<unsigned char> blob(head, 0);
    std::memcpy(blob.data(), views_host, (size_t)n_views * sizeof(cgs_metric_view));
    hipError_t e = hipMemcpyAsync(workspace, blob.data(), head, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return e;
    char* ws = static_cast<char*>(workspace);
    ProfScope p("view_metrics", s);
    hipLaunchKernelGGL(k_view_metrics, dim3(METRIC_BLOCKS, n_views), dim3(METRIC_THREADS), 0, s,
                       reinterpret_cast<const cgs_metric_view*>(ws),
                       reinterpret_cast<unsigned int*>(ws + MetricWs::counters_offset(n_views)),
                       reinterpret_cast<double*>(ws + MetricWs::partials_offset(n_views)), sums, means);
    return hipSuccess;
}

}  // namespace cgs
