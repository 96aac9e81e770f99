// Edge maps from photographs (include/curvegs.h, cgs_edge_gradients / cgs_edge_trace): a Canny detector with a soft
// response.  Every launch covers all views of a call, grid (tiles or pixel blocks of the largest view, n_views); the blocks a
// smaller view does not need exit uniformly.  The descriptor tables are kernel arguments (CGS_EDGE_MAX_VIEWS entries of 48
// bytes, plus the taps): no host -> device copy.
//   k_edge_gradients   one 64x16 tile per workgroup, ONE kernel from the uint8 pixels to gx, gy, m: the luminance of the tile
//                      plus a halo of radius + 1 is staged in LDS, blurred along rows into a second tile (halo radius + 1 in y,
//                      1 in x), along columns into a third (halo 1), and Sobel reads that.  Fused because the split would put
//                      the smoothed image through memory for nothing: the two blur passes need the same halo exchange
//                      either way, and Sobel adds one pixel to it.  Per pixel: channels bytes read (about 2x with the halo at
//                      radius 5, served by L2), 12 bytes written.
//   k_edge_classify    one thread per pixel: thinning against the two neighbours along the gradient, m' and the state byte.
//   k_edge_propagate   one 64x16 tile per workgroup: the states of the tile plus a 1-pixel halo in LDS, candidates next to a
//                      kept pixel are promoted until the tile is stable, the tile is written back, and a tile that changed
//                      sets the flag with an ordinary store.  A neighbouring tile may be read before or after its workgroup
//                      wrote it back: states only ever go from candidate to kept, so either value is a valid input, and a
//                      tile that missed a promotion sees it in the next round -- which there is, because that promotion
//                      set the flag.  The host repeats the launch until a round changes nothing.
//   k_edge_response    one thread per pixel: e = min(m' / high, 1) where kept, else 0, in place.
// No floating-point atomics and no integer ones.
#include <algorithm>
#include <cstring>

#include "kernels.h"

namespace cgs {

constexpr int EDGE_THREADS = 256;   // 4 waves
constexpr int EDGE_TW = 64, EDGE_TH = 16;   // output tile
constexpr int EDGE_R = CGS_EDGE_MAX_RADIUS;
constexpr int EDGE_LW = EDGE_TW + 2 * (EDGE_R + 1), EDGE_LH = EDGE_TH + 2 * (EDGE_R + 1);   // luminance tile, at most
constexpr int EDGE_SW = EDGE_TW + 2, EDGE_SH = EDGE_TH + 2;                                 // smoothed tile
static_assert(sizeof(cgs_edge_gradient_view) == 48, "cgs_edge_gradient_view: unexpected layout");
static_assert(sizeof(cgs_edge_trace_view) == 48, "cgs_edge_trace_view: unexpected layout");
static_assert(48 * CGS_EDGE_MAX_VIEWS + sizeof(float) * (2 * EDGE_R + 1) + 64 <= 4096,
              "the descriptor table must stay within the kernel-argument segment");
static_assert((EDGE_LW * EDGE_LH + EDGE_SW * EDGE_LH + EDGE_SW * EDGE_SH) * sizeof(float) <= 64 * 1024, "LDS tiles");

struct EdgeGradientTable {  // passed by value
    cgs_edge_gradient_view v[CGS_EDGE_MAX_VIEWS];
    float taps[2 * EDGE_R + 1];
};
struct EdgeTraceTable {  // passed by value
    cgs_edge_trace_view v[CGS_EDGE_MAX_VIEWS];
};

__device__ __forceinline__ int clampi(int a, int lo, int hi) { return a < lo ? lo : (a > hi ? hi : a); }

__global__ void __launch_bounds__(EDGE_THREADS) k_edge_gradients(const EdgeGradientTable t, int radius) {
#pragma clang fp contract(off)
    const cgs_edge_gradient_view& d = t.v[blockIdx.z];
    const int W = d.width, H = d.height, C = d.channels;
    const int x0 = blockIdx.x * EDGE_TW, y0 = blockIdx.y * EDGE_TH;
    if (x0 >= W || y0 >= H) return;   // (uniform) a smaller view of a mixed batch
    __shared__ float s_lum[EDGE_LH * EDGE_LW];   // coordinates (x0 - 1 - radius + c, y0 - 1 - radius + r), clamped
    __shared__ float s_row[EDGE_LH * EDGE_SW];   // blurred along x: (x0 - 1 + c, y0 - 1 - radius + r)
    __shared__ float s_sm[EDGE_SH * EDGE_SW];    // blurred along both: (x0 - 1 + c, y0 - 1 + r)
    const int halo = radius + 1;
    const int lw = EDGE_TW + 2 * halo, lh = EDGE_TH + 2 * halo;

    for (int k = threadIdx.x; k < lw * lh; k += EDGE_THREADS) {
        const int r = k / lw, c = k - r * lw;
        const int x = clampi(x0 - halo + c, 0, W - 1), y = clampi(y0 - halo + r, 0, H - 1);
        const uint8_t* __restrict__ p = d.pixels + ((int64_t)y * W + x) * C;
        float lum;
        if (C == 1) lum = (float)p[0] / 255.0f;
        else lum = ((0.299f * (float)p[0] + 0.587f * (float)p[1]) + 0.114f * (float)p[2]) / 255.0f;
        s_lum[r * EDGE_LW + c] = lum;
    }
    __syncthreads();
    // rows: the centre is the clamped coordinate, so a position outside the image repeats the border's result
    for (int k = threadIdx.x; k < EDGE_SW * lh; k += EDGE_THREADS) {
        const int r = k / EDGE_SW, c = k - r * EDGE_SW;
        const int cx = clampi(x0 - 1 + c, 0, W - 1) - (x0 - halo);   // in [radius, lw - 1 - radius]
        const float* __restrict__ row = s_lum + r * EDGE_LW + cx;
        float acc = t.taps[0] * row[-radius];
        for (int o = 1 - radius; o <= radius; o++) acc = acc + t.taps[o + radius] * row[o];
        s_row[r * EDGE_SW + c] = acc;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < EDGE_SW * EDGE_SH; k += EDGE_THREADS) {
        const int r = k / EDGE_SW, c = k - r * EDGE_SW;
        const int cy = clampi(y0 - 1 + r, 0, H - 1) - (y0 - halo);   // in [radius, lh - 1 - radius]
        const float* __restrict__ col = s_row + cy * EDGE_SW + c;
        float acc = t.taps[0] * col[-radius * EDGE_SW];
        for (int o = 1 - radius; o <= radius; o++) acc = acc + t.taps[o + radius] * col[o * EDGE_SW];
        s_sm[r * EDGE_SW + c] = acc;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < EDGE_TW * EDGE_TH; k += EDGE_THREADS) {
        const int r = k / EDGE_TW, c = k - r * EDGE_TW;
        const int x = x0 + c, y = y0 + r;
        if (x >= W || y >= H) continue;
        // the clamped neighbours: at a border the tile holds the repeated value already (see the centres above)
        const float* __restrict__ s = s_sm + (r + 1) * EDGE_SW + (c + 1);
        const float a00 = s[-EDGE_SW - 1], a01 = s[-EDGE_SW], a02 = s[-EDGE_SW + 1];
        const float a10 = s[-1], a12 = s[1];
        const float a20 = s[EDGE_SW - 1], a21 = s[EDGE_SW], a22 = s[EDGE_SW + 1];
        const float gx = (((a02 + 2.0f * a12) + a22) - ((a00 + 2.0f * a10) + a20)) * 0.25f;
        const float gy = (((a20 + 2.0f * a21) + a22) - ((a00 + 2.0f * a01) + a02)) * 0.25f;
        const int64_t at = (int64_t)y * W + x;
        d.gx[at] = gx;
        d.gy[at] = gy;
        d.m[at] = sqrtf(gx * gx + gy * gy);
    }
}

enum : uint8_t { EDGE_NONE = 0, EDGE_CANDIDATE = 1, EDGE_KEPT = 2 };

__global__ void __launch_bounds__(EDGE_THREADS) k_edge_classify(const EdgeTraceTable t, float low, float high, int thin) {
#pragma clang fp contract(off)
    const cgs_edge_trace_view& d = t.v[blockIdx.y];
    const int W = d.width, H = d.height;
    const int64_t n = (int64_t)H * W;
    const int64_t p = (int64_t)blockIdx.x * EDGE_THREADS + threadIdx.x;
    if (p >= n) return;
    const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
    const float m = d.m[p];
    float keep = m;
    if (thin) {
        const float gx = d.gx[p], gy = d.gy[p];
        const float ax = fabsf(gx), ay = fabsf(gy), T = 0.41421357f;
        int dx, dy;   // the first neighbour is (x + dx, y + dy), the second (x - dx, y - dy)
        if (ay <= T * ax) { dx = -1; dy = 0; }
        else if (ax <= T * ay) { dx = 0; dy = -1; }
        else if (gx * gy > 0.0f) { dx = -1; dy = -1; }
        else { dx = 1; dy = -1; }
        const int x1 = x + dx, y1 = y + dy, x2 = x - dx, y2 = y - dy;
        const float m1 = (x1 >= 0 && x1 < W && y1 >= 0 && y1 < H) ? d.m[(int64_t)y1 * W + x1] : 0.0f;
        const float m2 = (x2 >= 0 && x2 < W && y2 >= 0 && y2 < H) ? d.m[(int64_t)y2 * W + x2] : 0.0f;
        if (!(m > m1 && m >= m2)) keep = 0.0f;
    }
    d.e[p] = keep;
    d.state[p] = keep >= high ? EDGE_KEPT : (keep >= low ? EDGE_CANDIDATE : EDGE_NONE);
}

constexpr int EDGE_PW = EDGE_TW + 2, EDGE_PH = EDGE_TH + 2;           // states of a tile plus its halo
constexpr int EDGE_PER_THREAD = EDGE_TW * EDGE_TH / EDGE_THREADS;     // 4: thread (c, q) owns rows q, q + 4, q + 8, q + 12
static_assert(EDGE_THREADS % EDGE_TW == 0 && EDGE_PER_THREAD * EDGE_THREADS == EDGE_TW * EDGE_TH, "tile ownership");

__global__ void __launch_bounds__(EDGE_THREADS) k_edge_propagate(const EdgeTraceTable t, int* __restrict__ changed_flag) {
    const cgs_edge_trace_view& d = t.v[blockIdx.z];
    const int W = d.width, H = d.height;
    const int x0 = blockIdx.x * EDGE_TW, y0 = blockIdx.y * EDGE_TH;
    if (x0 >= W || y0 >= H) return;   // (uniform)
    __shared__ uint8_t s_state[EDGE_PH * EDGE_PW];
    int any_candidate = 0;
    for (int k = threadIdx.x; k < EDGE_PW * EDGE_PH; k += EDGE_THREADS) {
        const int r = k / EDGE_PW, c = k - r * EDGE_PW;
        const int x = x0 - 1 + c, y = y0 - 1 + r;
        uint8_t st = EDGE_NONE;
        if (x >= 0 && x < W && y >= 0 && y < H) st = d.state[(int64_t)y * W + x];
        s_state[k] = st;
        if (st == EDGE_CANDIDATE && r >= 1 && r <= EDGE_TH && c >= 1 && c <= EDGE_TW) any_candidate = 1;
    }
    if (!__syncthreads_or(any_candidate)) return;   // (uniform; also the barrier after the staging) nothing to promote
    const int c = (threadIdx.x & (EDGE_TW - 1)) + 1, q = threadIdx.x / EDGE_TW;
    int changed = 0;
    for (;;) {
        int promote = 0;   // bit i: the pixel in row q + 4 i
#pragma unroll
        for (int i = 0; i < EDGE_PER_THREAD; i++) {
            const uint8_t* s = s_state + (q + (EDGE_THREADS / EDGE_TW) * i + 1) * EDGE_PW + c;
            if (s[0] != EDGE_CANDIDATE) continue;
            const int kept = (s[-EDGE_PW - 1] == EDGE_KEPT) | (s[-EDGE_PW] == EDGE_KEPT) | (s[-EDGE_PW + 1] == EDGE_KEPT) |
                             (s[-1] == EDGE_KEPT) | (s[1] == EDGE_KEPT) | (s[EDGE_PW - 1] == EDGE_KEPT) |
                             (s[EDGE_PW] == EDGE_KEPT) | (s[EDGE_PW + 1] == EDGE_KEPT);
            promote |= kept << i;
        }
        __syncthreads();   // every read of this sweep is done
#pragma unroll
        for (int i = 0; i < EDGE_PER_THREAD; i++)
            if (promote >> i & 1) s_state[(q + (EDGE_THREADS / EDGE_TW) * i + 1) * EDGE_PW + c] = EDGE_KEPT;
        changed |= promote;
        if (!__syncthreads_or(promote)) break;   // (uniform)
    }
    // only promoted pixels are written: byte stores, each to a pixel this workgroup owns
#pragma unroll
    for (int i = 0; i < EDGE_PER_THREAD; i++) {
        const int r = q + (EDGE_THREADS / EDGE_TW) * i;
        const int x = x0 + c - 1, y = y0 + r;
        if ((changed >> i & 1) && x < W && y < H) d.state[(int64_t)y * W + x] = EDGE_KEPT;
    }
    if (__syncthreads_or(changed) && threadIdx.x == 0) *changed_flag = 1;
}

__global__ void __launch_bounds__(EDGE_THREADS) k_edge_response(const EdgeTraceTable t, float high) {
#pragma clang fp contract(off)
    const cgs_edge_trace_view& d = t.v[blockIdx.y];
    const int64_t n = (int64_t)d.height * d.width;
    const int64_t p = (int64_t)blockIdx.x * EDGE_THREADS + threadIdx.x;
    if (p >= n) return;
    d.e[p] = d.state[p] == EDGE_KEPT ? fminf(d.e[p] / high, 1.0f) : 0.0f;
}

void launch_edge_gradients(hipStream_t s, int n_views, const cgs_edge_gradient_view* views_host, const float* taps,
                           int radius) {
    EdgeGradientTable t;
    std::memset(&t, 0, sizeof(t));
    std::memcpy(t.v, views_host, (size_t)n_views * sizeof(cgs_edge_gradient_view));
    std::memcpy(t.taps, taps, (size_t)(2 * radius + 1) * sizeof(float));
    int tx = 1, ty = 1;
    for (int v = 0; v < n_views; v++) {
        tx = std::max(tx, (views_host[v].width + EDGE_TW - 1) / EDGE_TW);
        ty = std::max(ty, (views_host[v].height + EDGE_TH - 1) / EDGE_TH);
    }
    ProfScope p("edge_gradients", s);
    hipLaunchKernelGGL(k_edge_gradients, dim3(tx, ty, n_views), dim3(EDGE_THREADS), 0, s, t, radius);
}

// The number of propagation rounds, or -1 when a HIP call failed (*err holds it)
int launch_edge_trace(hipStream_t s, int n_views, const cgs_edge_trace_view* views_host, float low, float high, int thin,
                      int* changed_flag, hipError_t* err) {
    EdgeTraceTable t;
    std::memset(&t, 0, sizeof(t));
    std::memcpy(t.v, views_host, (size_t)n_views * sizeof(cgs_edge_trace_view));
    int tx = 1, ty = 1;
    int64_t max_pixels = 1;
    for (int v = 0; v < n_views; v++) {
        tx = std::max(tx, (views_host[v].width + EDGE_TW - 1) / EDGE_TW);
        ty = std::max(ty, (views_host[v].height + EDGE_TH - 1) / EDGE_TH);
        max_pixels = std::max(max_pixels, (int64_t)views_host[v].height * views_host[v].width);
    }
    const dim3 per_pixel((unsigned)((max_pixels + EDGE_THREADS - 1) / EDGE_THREADS), n_views);
    {
        ProfScope p("edge_classify", s);
        hipLaunchKernelGGL(k_edge_classify, per_pixel, dim3(EDGE_THREADS), 0, s, t, low, high, thin);
    }
    int rounds = 0;
    for (int changed = 1; changed;) {
        if ((*err = hipMemsetAsync(changed_flag, 0, sizeof(int), s)) != hipSuccess) return -1;
        {
            ProfScope p("edge_propagate", s);
            hipLaunchKernelGGL(k_edge_propagate, dim3(tx, ty, n_views), dim3(EDGE_THREADS), 0, s, t, changed_flag);
        }
        rounds++;
        if ((*err = hipMemcpyAsync(&changed, changed_flag, sizeof(int), hipMemcpyDeviceToHost, s)) != hipSuccess) return -1;
        if ((*err = hipStreamSynchronize(s)) != hipSuccess) return -1;
    }
    ProfScope p("edge_response", s);
    hipLaunchKernelGGL(k_edge_response, per_pixel, dim3(EDGE_THREADS), 0, s, t, high);
    return rounds;
}

}  // namespace cgs
