// Image summaries of the training report (reference train.py:346-364): for every view of a batch, five 8-bit RGB panels
// (render, ground truth, turbo-coloured depth, normalised direction map, alpha) in TWO launches:
//   k_report_depth_max   per-view depth maximum as REPORT_RED_BLOCKS partial maxima per view (plain stores, every slot
//                        written by every call: nothing to clear, no atomics, the same bits on every run)
//   k_report_panels      a streaming map: each lane takes four consecutive pixels of one view through all five panels --
//                        one 16-byte load per input plane, one 12-byte store per panel -- after its workgroup has folded
//                        the view's partial maxima and quantised the colour map into LDS
// The arithmetic and its order are the contract (include/curvegs.h): float32, no fused multiply-add, correctly rounded
// divide and square root, so that a float32 restatement of the same expressions gives the same bytes.
// The descriptor table is a kernel argument (CGS_REPORT_MAX_VIEWS entries of 64 bytes): no host -> device copy, and a
// stream capture of the two launches is self-contained.
#include <cstring>

#include "kernels.h"
#include "turbo_table.h"

namespace cgs {

constexpr int REPORT_THREADS = 256;       // 4 waves
constexpr int REPORT_RED_BLOCKS = 256;    // partial maxima per view; == REPORT_THREADS: the panel kernel reads one per lane
constexpr int REPORT_PANEL_BLOCKS = 1024; // most workgroups per view of the panel kernel (grid-stride beyond)
static_assert(REPORT_RED_BLOCKS == REPORT_THREADS, "k_report_panels folds one partial maximum per thread");
static_assert(CGS_TURBO_ENTRIES == REPORT_THREADS, "k_report_panels quantises one colour-map entry per thread");
static_assert(sizeof(cgs_report_view) == 64, "the descriptor table must stay within the kernel-argument segment");

struct ReportTable {  // passed by value
    cgs_report_view v[CGS_REPORT_MAX_VIEWS];
};

__device__ __forceinline__ float max_skip_nan(float m, float x) { return x > m ? x : m; }  // a NaN x compares false

// max over the workgroup of a non-NaN, non-negative value; the result is valid in every thread
__device__ __forceinline__ float block_max(float m, float* s_part) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = m;
    __syncthreads();
    return fmaxf(fmaxf(s_part[0], s_part[1]), fmaxf(s_part[2], s_part[3]));
}

__global__ void __launch_bounds__(REPORT_THREADS) k_report_depth_max(const ReportTable t, float* __restrict__ partials) {
    const cgs_report_view& d = t.v[blockIdx.y];
    float m = 0.f;   // depth >= 0 (curvegs.h); NaN pixels are skipped
    if (d.depth) {
        const int64_t n = (int64_t)d.height * d.width;
        const int64_t tid = (int64_t)blockIdx.x * REPORT_THREADS + threadIdx.x;
        const int64_t stride = (int64_t)REPORT_RED_BLOCKS * REPORT_THREADS;
        if ((reinterpret_cast<uintptr_t>(d.depth) & 15) == 0) {
            const float4* p4 = reinterpret_cast<const float4*>(d.depth);
            const int64_t n4 = n >> 2;
            for (int64_t i = tid; i < n4; i += stride) {
                const float4 q = p4[i];
                m = max_skip_nan(max_skip_nan(max_skip_nan(max_skip_nan(m, q.x), q.y), q.z), q.w);
            }
            if (tid < n - n4 * 4) m = max_skip_nan(m, d.depth[n4 * 4 + tid]);   // the last n % 4 pixels
        } else {
            for (int64_t i = tid; i < n; i += stride) m = max_skip_nan(m, d.depth[i]);
        }
    }
    __shared__ float s_part[REPORT_THREADS / 64];
    m = block_max(m, s_part);
    if (threadIdx.x == 0) partials[(size_t)blockIdx.y * REPORT_RED_BLOCKS + blockIdx.x] = m;
}

__device__ __forceinline__ float report_clamp01(float x) { return x < 0.f ? 0.f : (x > 1.f ? 1.f : x); }  // NaN stays NaN

// (uint8) clip(x * 255, 0, 255), truncated; NaN -> 0
__device__ __forceinline__ uint32_t q8(float x) {
    float y = x * 255.f;
    y = y > 0.f ? y : 0.f;   // NaN -> 0
    y = y < 255.f ? y : 255.f;
    return (uint32_t)y;
}

__device__ __forceinline__ uint32_t grey(uint32_t b) { return b * 0x010101u; }

// four consecutive floats of a plane from pixel i on (cnt < 4 at the end of the plane: the rest reads as 0)
__device__ __forceinline__ void load_quad(const float* __restrict__ p, int64_t i, int cnt, float (&x)[4]) {
    if (cnt == 4 && (reinterpret_cast<uintptr_t>(p + i) & 15) == 0) {
        const float4 q = *reinterpret_cast<const float4*>(p + i);
        x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) x[k] = k < cnt ? p[i + k] : 0.f;
    }
}

// four pixels 0x00BBGGRR -> 12 bytes R G B R G B ... at dst: one 12-byte store where dst is 4-byte aligned
__device__ __forceinline__ void store_quad(uint8_t* __restrict__ dst, const uint32_t (&px)[4], int cnt) {
    if (cnt == 4 && (reinterpret_cast<uintptr_t>(dst) & 3) == 0) {
        uint3 w;
        w.x = px[0] | (px[1] << 24);
        w.y = (px[1] >> 8) | (px[2] << 16);
        w.z = (px[2] >> 16) | (px[3] << 8);
        *reinterpret_cast<uint3*>(dst) = w;
    } else {
        for (int k = 0; k < cnt; k++) {
            dst[3 * k] = (uint8_t)px[k];
            dst[3 * k + 1] = (uint8_t)(px[k] >> 8);
            dst[3 * k + 2] = (uint8_t)(px[k] >> 16);
        }
    }
}

__global__ void __launch_bounds__(REPORT_THREADS) k_report_panels(const ReportTable t, const float* __restrict__ partials,
                                                                  uint8_t* __restrict__ out) {
#pragma clang fp contract(off)
    const cgs_report_view& d = t.v[blockIdx.y];
    const int64_t n = (int64_t)d.height * d.width;
    const int64_t nq = (n + 3) >> 2;   // quads: four consecutive pixels each, the last one possibly short
    if ((int64_t)blockIdx.x * REPORT_THREADS >= nq) return;   // (uniform) a smaller view of a mixed batch
    __shared__ uint32_t s_turbo[CGS_TURBO_ENTRIES];
    __shared__ float s_part[REPORT_THREADS / 64];
    float dmax = 0.f;
    if (d.depth) {   // (uniform)
        const float* c = cgs_turbo_table[threadIdx.x];
        s_turbo[threadIdx.x] = q8(c[0]) | (q8(c[1]) << 8) | (q8(c[2]) << 16);
        dmax = block_max(partials[(size_t)blockIdx.y * REPORT_RED_BLOCKS + threadIdx.x], s_part);   // (barrier inside)
    }
    uint8_t* __restrict__ o = out + d.out_offset;
    const int64_t panel = n * 3;
    for (int64_t q = (int64_t)blockIdx.x * REPORT_THREADS + threadIdx.x; q < nq; q += (int64_t)gridDim.x * REPORT_THREADS) {
        const int64_t i = q * 4;
        const int cnt = (int)(n - i < 4 ? n - i : 4);
        float x[4], y[4], z[4];
        uint32_t px[4];
        if (d.render) {
            load_quad(d.render, i, cnt, x);
#pragma unroll
            for (int k = 0; k < 4; k++) px[k] = grey(q8(report_clamp01(x[k])));
            store_quad(o + i * 3, px, cnt);
        }
        if (d.gt) {
            load_quad(d.gt, i, cnt, x);
            if (d.gt_channels == 3) {
                load_quad(d.gt + n, i, cnt, y);
                load_quad(d.gt + 2 * n, i, cnt, z);
#pragma unroll
                for (int k = 0; k < 4; k++)
                    px[k] = q8(report_clamp01(x[k])) | (q8(report_clamp01(y[k])) << 8) | (q8(report_clamp01(z[k])) << 16);
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++) px[k] = grey(q8(report_clamp01(x[k])));
            }
            store_quad(o + panel + i * 3, px, cnt);
        }
        if (d.depth) {
            load_quad(d.depth, i, cnt, x);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const float s = x[k] / dmax * 256.f;
                const int idx = s >= 255.f ? 255 : (s > 0.f ? (int)s : 0);
                px[k] = (dmax > 0.f && s == s) ? s_turbo[idx] : 0u;   // an all-zero view, NaN pixels: black
            }
            store_quad(o + 2 * panel + i * 3, px, cnt);
        }
        if (d.rend_dir) {
            load_quad(d.rend_dir, i, cnt, x);
            load_quad(d.rend_dir + n, i, cnt, y);
            load_quad(d.rend_dir + 2 * n, i, cnt, z);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const float len = sqrtf((x[k] * x[k] + y[k] * y[k]) + z[k] * z[k]);
                const float den = len < 1e-12f ? 1e-12f : len;   // clamp_min(eps): a NaN length stays NaN
                px[k] = q8(x[k] / den * 0.5f + 0.5f) | (q8(y[k] / den * 0.5f + 0.5f) << 8) | (q8(z[k] / den * 0.5f + 0.5f) << 16);
            }
            store_quad(o + 3 * panel + i * 3, px, cnt);
        }
        if (d.rend_alpha) {
            load_quad(d.rend_alpha, i, cnt, x);
#pragma unroll
            for (int k = 0; k < 4; k++) px[k] = grey(q8(report_clamp01(x[k])));
            store_quad(o + 4 * panel + i * 3, px, cnt);
        }
    }
}

size_t report_panels_workspace_bytes(int n_views) {
    return (size_t)(n_views > 0 ? n_views : 1) * REPORT_RED_BLOCKS * sizeof(float);
}

void launch_report_panels(hipStream_t s, int n_views, const cgs_report_view* views_host, void* workspace, unsigned char* out) {
    ReportTable t;
    std::memset(&t, 0, sizeof(t));
    std::memcpy(t.v, views_host, (size_t)n_views * sizeof(cgs_report_view));
    int64_t max_quads = 1;
    for (int v = 0; v < n_views; v++) {
        const int64_t nq = ((int64_t)views_host[v].height * views_host[v].width + 3) >> 2;
        if (nq > max_quads) max_quads = nq;
    }
    // about four quads per lane for the largest view, never more than REPORT_PANEL_BLOCKS workgroups per view
    int64_t gx = (max_quads + 4 * REPORT_THREADS - 1) / (4 * REPORT_THREADS);
    if (gx > REPORT_PANEL_BLOCKS) gx = REPORT_PANEL_BLOCKS;
    float* partials = static_cast<float*>(workspace);
    {
        ProfScope p("report_depth_max", s);
        hipLaunchKernelGGL(k_report_depth_max, dim3(REPORT_RED_BLOCKS, n_views), dim3(REPORT_THREADS), 0, s, t, partials);
    }
    ProfScope p("report_panels", s);
    hipLaunchKernelGGL(k_report_panels, dim3((unsigned)gx, n_views), dim3(REPORT_THREADS), 0, s, t,
                       static_cast<const float*>(partials), out);
}

}  // namespace cgs
