// Multi-view projection of extracted edges: every sampled edge point into every camera of a scan, as the reference's
// eval_ABC.py --render_mv (project_points_to_camera / visualize_projection, :66-138) and eval_replica.py (process_scan,
// :100-212) do with a Python loop over points inside a Python loop over views.
//
// Projection (exact, the reference's operation order): X float32 widened to float64, c = R X + T with every row
// ((r0*X + r1*Y) + r2*Z) + t, dropped if c2 <= 0 (a NaN depth is dropped too: it fails the image test below), then
// u = fx * (c0 / c2) + cx, v = fy * (c1 / c2) + cy, kept if 0 <= u < W and 0 <= v < H.  Contraction into FMAs is off
// and divisions are IEEE, as in visibility.hip.
//
// Raster (the project's own contract; the reference draws through matplotlib): a kept point covers pixel
// (floor(u), floor(v)); the n points of a pixel are composited in ascending point index with a constant alpha over the
// background, out = bg (1-a)^n + sum_j a c_j (1-a)^r_j, r_j = the number of later points in the pixel.  Points with
// (1-a)^r_j <= 2^-25 are left out: only the newest K = min{k : (1-a)^k <= 2^-25} points of a pixel are composited, so the
// dropped terms sum to at most (1-a)^K max|c| <= 2^-25 max|c| (K = 25 at a = 0.5, 1 at a = 1, 165 at a = 0.1); the
// background term always uses the full n.  Accumulation is float64, rounded to float32 once.
//
// Shape, per chunk of views that fits the workspace: (1) count the kept points of every pixel with integer atomics,
// (2) exclusive scan of the per-pixel counts (multi-block: block sums, one-workgroup scan of the sums, block rescan),
// (3) recompute the projection and scatter point indices into the per-pixel lists (integer atomics on the offsets, which
// become end offsets), (4) one thread per pixel selects the newest K indices by repeated maximum below the previous one
// (O(n min(n, K)) reads of the pixel's list, from L1 / L2) and composites them.  The list order the atomics produce never
// reaches the result: the output depends only on the set of points in each pixel, so two runs are bit-identical.  Pixel
// offsets are 64-bit; list offsets are 32-bit because a chunk holds at most 2^31 (view, point) pairs.
#include "kernels.h"
#include "point_projection.h"

#include <math.h>

#include <algorithm>

namespace cgs {

constexpr int NV_BLOCK = 256;                  // threads per workgroup, every kernel here
constexpr int NV_SCAN_ITEMS = 8;               // counts per thread in the block-level scan
constexpr int NV_SCAN_TILE = NV_BLOCK * NV_SCAN_ITEMS;
constexpr int NV_POINT_BLOCKS_MAX = 1024;      // grid.x of the projection passes (points loop inside)
constexpr long long NV_MAX_PAIRS = 1LL << 31;  // (view, point) pairs per chunk: 32-bit list offsets
constexpr int NV_MAX_VIEWS = 65535;            // views per launch: grid.y

// NvCam, nv_load_cam, nv_project: point_projection.h (shared with edge_score.hip)

// The depth gate (include/curvegs.h, cgs_project_points_depth / cgs_render_points_depth): k_nv_project and k_nv_bin are
// templates over GATED and take what a view says of a point from nv_verdict<GATED> (point_projection.h).  false is the
// projection as it always was: depth, slack and the hidden outputs are not touched.  true drops a point that the view's
// depth plane hides, as a point outside the image is dropped; the count pass and the fill pass call the same function on
// the same data, so they reach the same verdict and the lists are exactly as long as their counts.

// uv[v][i] = (u, v) of a kept point, (NaN, NaN) for a dropped one.  GATED: a hidden point is dropped too, and
// hidden_out[v][i] (optional) = 1 iff the projection kept the point and the gate hid it.
template <bool GATED>
__global__ void __launch_bounds__(NV_BLOCK) k_nv_project(int P, const float* __restrict__ pts,
                                                        const double* __restrict__ intr, const double* __restrict__ w2c,
                                                        int height, int width, double* __restrict__ uv,
                                                        const float* __restrict__ depth, double slack,
                                                        uint8_t* __restrict__ hidden_out) {
    const int view = blockIdx.y;
    NvCam c;
    nv_load_cam(c, intr, w2c, view);
    const double wd = (double)width, hd = (double)height;
    const float* __restrict__ dplane = GATED ? depth + (size_t)view * (size_t)height * (size_t)width : nullptr;
    for (long long i = (long long)blockIdx.x * NV_BLOCK + threadIdx.x; i < P; i += (long long)gridDim.x * NV_BLOCK) {
        double u, v;
        const NvVerdict verdict = nv_verdict<GATED>(c, (double)pts[3 * i + 0], (double)pts[3 * i + 1], (double)pts[3 * i + 2],
                                                    wd, hd, dplane, width, slack, u, v);
        const bool keep = verdict == NV_VISIBLE;
        double* o = uv + 2 * ((size_t)view * (size_t)P + (size_t)i);
        o[0] = keep ? u : (double)NAN;
        o[1] = keep ? v : (double)NAN;
        if (GATED && hidden_out) hidden_out[(size_t)view * (size_t)P + (size_t)i] = verdict == NV_HIDDEN ? 1 : 0;
    }
}

__global__ void __launch_bounds__(NV_BLOCK) k_nv_zero(long long n, unsigned int* __restrict__ a) {
    for (long long i = (long long)blockIdx.x * NV_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * NV_BLOCK) a[i] = 0u;
}

// Pass 1 (fill = 0): counts[pixel] += 1 per kept point.  Pass 3 (fill = 1): list[ends[pixel]++] = i.
// grid.y = views of the chunk (view v0 + blockIdx.y), pixel index (size_t)blockIdx.y * H * W + y * W + x.
// GATED: depth [V,H,W] and hidden [V] (optional) belong to ALL views and are indexed by the absolute view v0 + blockIdx.y; a
// hidden point is in neither pass, and the count pass alone tallies it: a register count per thread, one shuffle
// reduction per wave (every lane leaves the loop and reaches it) and one integer atomicAdd per wave that has any, as
// k_point_mask_depth does.
template <bool GATED>
__global__ void __launch_bounds__(NV_BLOCK) k_nv_bin(int P, const float* __restrict__ pts, const double* __restrict__ intr,
                                                    const double* __restrict__ w2c, int v0, int height, int width,
                                                    unsigned int* __restrict__ cells, unsigned int* __restrict__ list,
                                                    int fill, const float* __restrict__ depth, double slack,
                                                    int* __restrict__ hidden) {
    const int view = v0 + (int)blockIdx.y;
    NvCam c;
    nv_load_cam(c, intr, w2c, view);
    const double wd = (double)width, hd = (double)height;
    const size_t base = (size_t)blockIdx.y * (size_t)height * (size_t)width;
    const float* __restrict__ dplane = GATED ? depth + (size_t)view * (size_t)height * (size_t)width : nullptr;
    int h = 0;   // GATED only
    for (long long i = (long long)blockIdx.x * NV_BLOCK + threadIdx.x; i < P; i += (long long)gridDim.x * NV_BLOCK) {
        double u, v;
        const NvVerdict verdict = nv_verdict<GATED>(c, (double)pts[3 * i + 0], (double)pts[3 * i + 1], (double)pts[3 * i + 2],
                                                    wd, hd, dplane, width, slack, u, v);
        if (verdict == NV_OUT) continue;
        if (GATED && verdict == NV_HIDDEN) {
            h++;
            continue;
        }
        // 0 <= u < W, so 0 <= floor(u) <= W - 1 (likewise v): the pixel is inside the view's plane
        const size_t pix = base + (size_t)floor(v) * (size_t)width + (size_t)floor(u);
        const unsigned int slot = atomicAdd(&cells[pix], 1u);
        if (fill) list[slot] = (unsigned int)i;
    }
    if constexpr (GATED) {
        if (fill || !hidden) return;   // (uniform over the grid)
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) h += __shfl_xor(h, off, 64);
        if ((threadIdx.x & 63) == 0 && h) atomicAdd(&hidden[view], h);
    }
}

// Exclusive scan of a workgroup's values (one per thread) in LDS; returns the thread's prefix, *total the sum.
__device__ inline unsigned int nv_block_scan(unsigned int x, unsigned int* s, unsigned int* total) {
    const int t = threadIdx.x;
    s[t] = x;
    __syncthreads();
    for (int d = 1; d < NV_BLOCK; d <<= 1) {
        const unsigned int y = t >= d ? s[t - d] : 0u;
        __syncthreads();
        s[t] += y;
        __syncthreads();
    }
    const unsigned int incl = s[t];
    *total = s[NV_BLOCK - 1];
    __syncthreads();
    return incl - x;
}

// Scan step 1: the sum of each NV_SCAN_TILE counts.
__global__ void __launch_bounds__(NV_BLOCK) k_nv_scan_sums(long long n, const unsigned int* __restrict__ counts,
                                                          unsigned int* __restrict__ sums) {
    __shared__ unsigned int s[NV_BLOCK];
    const long long b0 = (long long)blockIdx.x * NV_SCAN_TILE + (long long)threadIdx.x * NV_SCAN_ITEMS;
    unsigned int x = 0;
#pragma unroll
    for (int k = 0; k < NV_SCAN_ITEMS; k++)
        if (b0 + k < n) x += counts[b0 + k];
    unsigned int total;
    nv_block_scan(x, s, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// Scan step 2: exclusive scan of the tile sums in place, one workgroup, NV_BLOCK at a time with a carry.
__global__ void __launch_bounds__(NV_BLOCK) k_nv_scan_tiles(int n_tiles, unsigned int* __restrict__ sums) {
    __shared__ unsigned int s[NV_BLOCK];
    unsigned int carry = 0;
    for (int b = 0; b < n_tiles; b += NV_BLOCK) {
        const int i = b + threadIdx.x;
        const unsigned int x = i < n_tiles ? sums[i] : 0u;
        unsigned int total;
        const unsigned int ex = nv_block_scan(x, s, &total);
        if (i < n_tiles) sums[i] = carry + ex;
        carry += total;
    }
}

// Scan step 3: offsets[i] = exclusive prefix of counts[i] over the whole chunk.
__global__ void __launch_bounds__(NV_BLOCK) k_nv_scan_apply(long long n, const unsigned int* __restrict__ counts,
                                                           const unsigned int* __restrict__ sums,
                                                           unsigned int* __restrict__ offsets) {
    __shared__ unsigned int s[NV_BLOCK];
    const long long b0 = (long long)blockIdx.x * NV_SCAN_TILE + (long long)threadIdx.x * NV_SCAN_ITEMS;
    unsigned int c[NV_SCAN_ITEMS];
    unsigned int x = 0;
#pragma unroll
    for (int k = 0; k < NV_SCAN_ITEMS; k++) {
        c[k] = b0 + k < n ? counts[b0 + k] : 0u;
        x += c[k];
    }
    unsigned int total;
    unsigned int run = sums[blockIdx.x] + nv_block_scan(x, s, &total);
#pragma unroll
    for (int k = 0; k < NV_SCAN_ITEMS; k++) {
        if (b0 + k < n) offsets[b0 + k] = run;
        run += c[k];
    }
}

// kept[v0 + v] = kept points of view v of the chunk (from the start offsets: before the fill pass moves them).
__global__ void __launch_bounds__(NV_BLOCK) k_nv_kept(int nv, long long plane, const unsigned int* __restrict__ counts,
                                                     const unsigned int* __restrict__ offsets, int* __restrict__ kept) {
    const int v = blockIdx.x * NV_BLOCK + threadIdx.x;
    if (v >= nv) return;
    const long long first = (long long)v * plane;
    const long long last = first + plane - 1;
    kept[v] = (int)(offsets[last] + counts[last] - offsets[first]);
}

// Pass 4: one thread per pixel of the chunk; ends[] are the fill pass's end offsets, counts[] the list lengths.
__global__ void __launch_bounds__(NV_BLOCK) k_nv_composite(long long n_pix, const unsigned int* __restrict__ counts,
                                                          const unsigned int* __restrict__ ends,
                                                          const unsigned int* __restrict__ list,
                                                          const float* __restrict__ colors, double alpha, int keep_max,
                                                          double bg0, double bg1, double bg2, float* __restrict__ out) {
    for (long long g = (long long)blockIdx.x * NV_BLOCK + threadIdx.x; g < n_pix; g += (long long)gridDim.x * NV_BLOCK) {
        const unsigned int n = counts[g];
        double r = 0.0, gr = 0.0, b = 0.0, T = 1.0;
        const double om = 1.0 - alpha;
        if (n > 0) {
            const unsigned int e = ends[g], s0 = e - n;
            const unsigned int m = n < (unsigned int)keep_max ? n : (unsigned int)keep_max;
            long long prev = 0x7fffffffffffLL;   // above every point index
            for (unsigned int k = 0; k < m; k++) {
                long long best = -1;
                for (unsigned int j = s0; j < e; j++) {
                    const long long id = (long long)list[j];
                    if (id < prev && id > best) best = id;
                }
                const double w = alpha * T;
                r += w * (double)colors[3 * best + 0];
                gr += w * (double)colors[3 * best + 1];
                b += w * (double)colors[3 * best + 2];
                T *= om;
                prev = best;
            }
            if (m < n) T = pow(om, (double)n);
        }
        float* o = out + 3 * (size_t)g;
        o[0] = (float)(r + bg0 * T);
        o[1] = (float)(gr + bg1 * T);
        o[2] = (float)(b + bg2 * T);
    }
}

// Views per chunk and the workspace they need.
static size_t nv_align(size_t b) { return (b + 255) & ~(size_t)255; }

static size_t nv_chunk_bytes(long long P, long long nv, long long plane) {
    const long long n = nv * plane;
    const long long tiles = (n + NV_SCAN_TILE - 1) / NV_SCAN_TILE;
    return 2 * nv_align((size_t)n * 4) + nv_align((size_t)(nv * P) * 4) + nv_align((size_t)tiles * 4);
}

size_t render_points_workspace_bytes(int P, int V, int H, int W) {
    if (P < 0 || V <= 0 || H <= 0 || W <= 0) return 0;
    const long long plane = (long long)H * W;
    long long nv = std::min(V, NV_MAX_VIEWS);
    if (P > 0) nv = std::min(nv, NV_MAX_PAIRS / P);
    return nv_chunk_bytes(P, std::max(nv, 1LL), plane);
}

int render_points_views_per_chunk(int P, int V, int H, int W, size_t ws_bytes) {
    const long long plane = (long long)H * W;
    long long hi = std::min(V, NV_MAX_VIEWS);
    if (P > 0) hi = std::min(hi, NV_MAX_PAIRS / P);
    if (hi < 1 || nv_chunk_bytes(P, 1, plane) > ws_bytes) return 0;
    long long lo = 1;   // largest nv in [1, hi] with nv_chunk_bytes <= ws_bytes (monotone in nv)
    while (lo < hi) {
        const long long mid = (lo + hi + 1) / 2;
        if (nv_chunk_bytes(P, mid, plane) <= ws_bytes) lo = mid; else hi = mid - 1;
    }
    return (int)lo;
}

// The newest K points of a pixel are composited: K = min{k >= 1 : (1-a)^k <= 2^-25} (1 at a = 1), 0 at a = 0 (every point
// has weight 0: the pixel is the background), capped at 2^31 - 1.
int render_points_keep(double alpha) {
    const double om = 1.0 - alpha;
    if (om <= 0.0) return 1;
    if (om >= 1.0) return 0;
    const double cut = 1.0 / 33554432.0;   // 2^-25
    double k = ceil(-25.0 / log2(om));
    while (k > 1.0 && pow(om, k - 1.0) <= cut) k -= 1.0;
    while (pow(om, k) > cut && k < 2147483647.0) k += 1.0;
    return (int)std::min(k, 2147483647.0);
}

static int nv_point_blocks(int P) { return std::max(1, std::min(NV_POINT_BLOCKS_MAX, (P + NV_BLOCK - 1) / NV_BLOCK)); }

template <bool GATED>
static void project_points_launches(hipStream_t s, int P, const float* points, int V, const double* intr, const double* w2c,
                                    int height, int width, double* uv, DepthGate gate, uint8_t* hidden_out) {
    const size_t plane = (size_t)height * (size_t)width;
    ProfScope p(GATED ? "project_points_depth" : "project_points", s);
    for (int v0 = 0; v0 < V; v0 += NV_MAX_VIEWS) {
        const int nv = std::min(NV_MAX_VIEWS, V - v0);
        hipLaunchKernelGGL(k_nv_project<GATED>, dim3(nv_point_blocks(P), nv), dim3(NV_BLOCK), 0, s, P, points,
                           intr + 4 * (size_t)v0, w2c + 12 * (size_t)v0, height, width, uv + 2 * (size_t)v0 * (size_t)P,
                           GATED ? gate.depth + (size_t)v0 * plane : nullptr, gate.slack,
                           GATED && hidden_out ? hidden_out + (size_t)v0 * (size_t)P : nullptr);
    }
}

void launch_project_points(hipStream_t s, int P, const float* points, int V, const double* intr, const double* w2c,
                           int height, int width, const DepthGate* gate, double* uv, uint8_t* hidden_out) {
    if (gate) project_points_launches<true>(s, P, points, V, intr, w2c, height, width, uv, *gate, hidden_out);
    else project_points_launches<false>(s, P, points, V, intr, w2c, height, width, uv, DepthGate{nullptr, 0.0}, nullptr);
}

template <bool GATED>
static void render_points_launches(hipStream_t s, int P, const float* points, const float* colors, int V, const double* intr,
                                   const double* w2c, int height, int width, double alpha, const double* bg, float* out,
                                   int* kept, void* ws, int views_per_chunk, DepthGate gate, int* hidden) {
    const long long plane = (long long)height * width;
    const int keep_max = render_points_keep(alpha);
    if (GATED && hidden)   // cleared by a kernel: a captured memset node clears once (zero_async in api.hip)
        hipLaunchKernelGGL(k_nv_zero, dim3((V + NV_BLOCK - 1) / NV_BLOCK), dim3(NV_BLOCK), 0, s, (long long)V,
                           reinterpret_cast<unsigned int*>(hidden));
    for (int v0 = 0; v0 < V; v0 += views_per_chunk) {
        const int nv = std::min(views_per_chunk, V - v0);
        const long long n = (long long)nv * plane;
        const long long tiles = (n + NV_SCAN_TILE - 1) / NV_SCAN_TILE;
        char* w = (char*)ws;
        unsigned int* counts = (unsigned int*)w;
        w += nv_align((size_t)n * 4);
        unsigned int* offsets = (unsigned int*)w;
        w += nv_align((size_t)n * 4);
        unsigned int* list = (unsigned int*)w;
        w += nv_align((size_t)((long long)nv * P) * 4);
        unsigned int* sums = (unsigned int*)w;
        const int zblocks = (int)std::min<long long>(4096, (n + NV_BLOCK - 1) / NV_BLOCK);
        const int pblocks = (int)std::min<long long>(65536, (n + NV_BLOCK - 1) / NV_BLOCK);
        {
            ProfScope p("render_points_count", s);
            hipLaunchKernelGGL(k_nv_zero, dim3(zblocks), dim3(NV_BLOCK), 0, s, n, counts);
            if (P > 0)
                hipLaunchKernelGGL(k_nv_bin<GATED>, dim3(nv_point_blocks(P), nv), dim3(NV_BLOCK), 0, s, P, points, intr, w2c,
                                   v0, height, width, counts, (unsigned int*)nullptr, 0, gate.depth, gate.slack, hidden);
        }
        {
            ProfScope p("render_points_scan", s);
            hipLaunchKernelGGL(k_nv_scan_sums, dim3((unsigned)tiles), dim3(NV_BLOCK), 0, s, n, counts, sums);
            hipLaunchKernelGGL(k_nv_scan_tiles, dim3(1), dim3(NV_BLOCK), 0, s, (int)tiles, sums);
            hipLaunchKernelGGL(k_nv_scan_apply, dim3((unsigned)tiles), dim3(NV_BLOCK), 0, s, n, counts, sums, offsets);
            if (kept)
                hipLaunchKernelGGL(k_nv_kept, dim3((nv + NV_BLOCK - 1) / NV_BLOCK), dim3(NV_BLOCK), 0, s, nv, plane,
                                   counts, offsets, kept + v0);
        }
        if (P > 0) {
            ProfScope p("render_points_fill", s);
            hipLaunchKernelGGL(k_nv_bin<GATED>, dim3(nv_point_blocks(P), nv), dim3(NV_BLOCK), 0, s, P, points, intr, w2c, v0,
                               height, width, offsets, list, 1, gate.depth, gate.slack, hidden);
        }
        {
            ProfScope p("render_points_composite", s);
            hipLaunchKernelGGL(k_nv_composite, dim3(pblocks), dim3(NV_BLOCK), 0, s, n, counts, offsets, list, colors,
                               alpha, keep_max, bg[0], bg[1], bg[2], out + 3 * (size_t)v0 * (size_t)plane);
        }
    }
}

// The lists of the gated form can only be shorter: the workspace of cgs_render_points holds them.
void launch_render_points(hipStream_t s, int P, const float* points, const float* colors, int V, const double* intr,
                          const double* w2c, int height, int width, const DepthGate* gate, double alpha, const double* bg,
                          float* out, int* kept, int* hidden, void* ws, int views_per_chunk) {
    if (gate)
        render_points_launches<true>(s, P, points, colors, V, intr, w2c, height, width, alpha, bg, out, kept, ws,
                                     views_per_chunk, *gate, hidden);
    else
        render_points_launches<false>(s, P, points, colors, V, intr, w2c, height, width, alpha, bg, out, kept, ws,
                                      views_per_chunk, DepthGate{nullptr, 0.0}, nullptr);
}

}  // namespace cgs
