// Undistortion of a COLMAP scan's edge maps when the scan is loaded (include/curvegs.h, cgs_undistort_images): every pixel
// of the ideal pinhole camera is pushed forward through the lens model and the detected map is sampled there with bilinear
// weights.  ONE launch for all views of a call, grid (pixel blocks of the largest view, n_views):
//   k_undistort   one thread per output pixel, all channels: the float64 coordinates are computed once; consecutive lanes
//                 take consecutive columns, so every store is a coalesced row segment and the four taps of a wave lie in two
//                 (slightly bent) source rows.  A memory-bound gather that runs once per scan: nothing is staged or tuned.
// The descriptor table is a kernel argument (CGS_UNDISTORT_MAX_VIEWS entries of 144 bytes): no host -> device copy.
// Blank pixels are counted per wave with a ballot, per workgroup through LDS, and added with at most one integer atomic
// per workgroup.
#include <cstring>

#include "kernels.h"

namespace cgs {

constexpr int UNDISTORT_THREADS = 256;   // 4 waves
static_assert(sizeof(cgs_undistort_view) == 144, "cgs_undistort_view: unexpected layout");
static_assert(sizeof(cgs_undistort_view) * CGS_UNDISTORT_MAX_VIEWS + 64 <= 4096,
              "the descriptor table must stay within the kernel-argument segment");

struct UndistortTable {  // passed by value
    cgs_undistort_view v[CGS_UNDISTORT_MAX_VIEWS];
};

__global__ void __launch_bounds__(UNDISTORT_THREADS) k_undistort(const UndistortTable t, float fill,
                                                                 int* __restrict__ blank_counts) {
#pragma clang fp contract(off)
    const cgs_undistort_view& d = t.v[blockIdx.y];
    const int W = d.width, H = d.height;
    const int64_t n = (int64_t)H * W;
    if ((int64_t)blockIdx.x * UNDISTORT_THREADS >= n) return;   // (uniform) a smaller view of a mixed batch
    const int64_t p = (int64_t)blockIdx.x * UNDISTORT_THREADS + threadIdx.x;
    bool blank = false;
    if (p < n) {
        const int j = (int)(p / W), i = (int)(p - (int64_t)j * W);
        const double x = ((double)i + 0.5 - (double)W / 2.0) / d.out_fx;
        const double y = ((double)j + 0.5 - (double)H / 2.0) / d.out_fy;
        double xd = x, yd = y;
        if (d.model >= 2) {   // (uniform) 0, 1: the pinhole models
            const double r2 = x * x + y * y;
            double s;
            if (d.model == 2) {
                s = 1.0 + d.k[0] * r2;
            } else if (d.model == 6) {
                s = (1.0 + d.k[0] * r2 + d.k[1] * r2 * r2 + d.k[4] * r2 * r2 * r2) /
                    (1.0 + d.k[5] * r2 + d.k[6] * r2 * r2 + d.k[7] * r2 * r2 * r2);
            } else {
                s = 1.0 + d.k[0] * r2 + d.k[1] * r2 * r2;
            }
            xd = x * s;
            yd = y * s;
            if (d.model == 4 || d.model == 6) {
                const double p1 = d.k[2], p2 = d.k[3];
                xd = xd + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x);
                yd = yd + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y;
            }
        }
        const double u = d.fx * xd + d.cx - 0.5;
        const double v = d.fy * yd + d.cy - 0.5;
        float w[4] = {0.f, 0.f, 0.f, 0.f};
        int64_t at[4] = {0, 0, 0, 0};
        bool in[4] = {false, false, false, false};
        // u in (-1, W) and v in (-1, H): a tap of non-zero weight is inside (x0 = -1 has a > 0, y0 = -1 has b > 0), and
        // x0, y0 fit an int.  Anything else, a NaN included (it compares false), is blank
        if (u > -1.0 && u < (double)W && v > -1.0 && v < (double)H) {
            const double fu = floor(u), fv = floor(v);
            const int x0 = (int)fu, y0 = (int)fv;
            const double a = u - fu, b = v - fv;
            const bool cx0 = x0 >= 0, cx1 = x0 + 1 <= W - 1, ry0 = y0 >= 0, ry1 = y0 + 1 <= H - 1;
            in[0] = cx0 && ry0; in[1] = cx1 && ry0; in[2] = cx0 && ry1; in[3] = cx1 && ry1;
            w[0] = (float)((1.0 - a) * (1.0 - b)); w[1] = (float)(a * (1.0 - b));
            w[2] = (float)((1.0 - a) * b);         w[3] = (float)(a * b);
            at[0] = (int64_t)y0 * W + x0; at[1] = at[0] + 1; at[2] = at[0] + W; at[3] = at[2] + 1;
        } else {
            blank = true;
        }
        if (blank) {
            for (int c = 0; c < d.channels; c++) d.dst[c * n + p] = fill;
        } else {
            for (int c = 0; c < d.channels; c++) {
                const float* __restrict__ s = d.src + c * n;
                const float t0 = in[0] ? s[at[0]] : fill, t1 = in[1] ? s[at[1]] : fill;
                const float t2 = in[2] ? s[at[2]] : fill, t3 = in[3] ? s[at[3]] : fill;
                d.dst[c * n + p] = ((w[0] * t0 + w[1] * t1) + w[2] * t2) + w[3] * t3;
            }
        }
    }
    __shared__ int s_cnt[UNDISTORT_THREADS / 64];
    const int wave_cnt = __popcll(__ballot(blank));
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = wave_cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int cnt = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
        if (cnt) atomicAdd(&blank_counts[blockIdx.y], cnt);
    }
}

void launch_undistort_images(hipStream_t s, int n_views, const cgs_undistort_view* views_host, float fill, int* blank_counts) {
    UndistortTable t;
    std::memset(&t, 0, sizeof(t));
    std::memcpy(t.v, views_host, (size_t)n_views * sizeof(cgs_undistort_view));
    int64_t max_pixels = 1;
    for (int v = 0; v < n_views; v++) {
        const int64_t n = (int64_t)views_host[v].height * views_host[v].width;
        if (n > max_pixels) max_pixels = n;
    }
    const int64_t gx = (max_pixels + UNDISTORT_THREADS - 1) / UNDISTORT_THREADS;
    ProfScope p("undistort_images", s);
    hipLaunchKernelGGL(k_undistort, dim3((unsigned)gx, n_views), dim3(UNDISTORT_THREADS), 0, s, t, fill, blank_counts);
}

}  // namespace cgs
