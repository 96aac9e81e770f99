// Reprojection score of extracted edges (include/curvegs.h, cgs_point_mask / cgs_edt_squared / cgs_edge_score_reduce):
// the edges projected into a camera against that camera's edge map, in pixels.  Three steps, all views of a call at once:
//   k_point_mask       grid (point blocks, views): the projection of novel_view.hip (point_projection.h, the same device
//                      function), a kept point stores the byte 1 at (floor(u), floor(v)).  Several points of one pixel store
//                      the same value: plain byte stores, no atomics on the mask.  The kept count of a view is a per-wave
//                      shuffle sum added with one integer atomic per wave.
//   k_edt_columns      exact squared Euclidean distance transform, pass 1: one thread per (view, x), so a wave reads 64
//                      consecutive mask bytes and writes 64 consecutive uint16 per row.  Down the column it writes the
//                      distance to the nearest feature above, up the column the minimum with the nearest below:
//                      g[v][y][x] = min |y - y'| over the features of column x, EDT_NO_FEATURE where the column has none.
//   k_edt_rows         pass 2: one thread per pixel.  best = g[x]^2, then outward over d = 1, 2, ... while d^2 < best:
//                      best = min(best, d^2 + g[x -+ d]^2).  Every candidate left out has d^2 >= best, so the minimum is
//                      exact; int32 throughout (d, g <= 16383: a finite value is below 2^29).  g is read through L1 / L2: a
//                      row of g is 2 W bytes (3.2 KB at W = 1600), far below the cache, and the reach of a search has no
//                      bound that an LDS tile with a fixed halo could serve.  Cost per pixel: the true distance, O(W) on a
//                      view with (almost) no feature.
//   k_edge_score       the counts and sums of a view: SCORE_BLOCKS fixed slices, every workgroup writes its partials, the
//                      last workgroup of the view (an integer counter decides which) adds them in index order, as
//                      k_view_metrics does.  Counts are integers; the two float64 sums are added in an order fixed by the
//                      view's size alone, so two runs agree bit for bit.
// No floating-point atomics.
#include <algorithm>
#include <climits>

#include "kernels.h"
#include "point_projection.h"

namespace cgs {

constexpr int SCORE_THREADS = 256;         // 4 waves: point mask, row pass, reduction
constexpr int EDT_COL_THREADS = 64;        // one wave per workgroup in the column pass: V * W / 64 workgroups to spread
constexpr int SCORE_POINT_BLOCKS_MAX = 1024;
constexpr int SCORE_MAX_VIEWS = 65535;     // views per launch: grid.y
constexpr int SCORE_BLOCKS = 64;           // workgroups per view in the reduction
constexpr int SCORE_SLOTS = 2 + 2 * CGS_EDGE_SCORE_MAX_TOL + 2;   // n_pred, n_det, pred_hits[8], det_hits[8], two sums
constexpr unsigned short EDT_NO_FEATURE = 0xffffu;
static_assert(CGS_EDT_MAX_SIZE < EDT_NO_FEATURE, "a column distance must fit below the sentinel");
static_assert(CGS_EDT_INF == INT_MAX, "CGS_EDT_INF");

struct ScoreTol {  // passed by value
    int n;
    int tol2[CGS_EDGE_SCORE_MAX_TOL];
};

// ------------------------------------------------------------------------------------------------ point mask
__global__ void __launch_bounds__(SCORE_THREADS) k_point_mask(int P, const float* __restrict__ pts,
                                                             const double* __restrict__ intr,
                                                             const double* __restrict__ w2c, int height, int width,
                                                             uint8_t* __restrict__ mask, int* __restrict__ kept) {
    const int view = blockIdx.y;
    NvCam c;
    nv_load_cam(c, intr, w2c, view);
    const double wd = (double)width, hd = (double)height;
    uint8_t* __restrict__ plane = mask + (size_t)view * (size_t)height * (size_t)width;
    int n = 0;
    for (long long i = (long long)blockIdx.x * SCORE_THREADS + threadIdx.x; i < P; i += (long long)gridDim.x * SCORE_THREADS) {
        double u, v;
        if (!nv_project(c, pts, i, wd, hd, u, v)) continue;
        // 0 <= u < W, so 0 <= floor(u) <= W - 1 (likewise v): the pixel is inside the view's plane
        plane[(size_t)floor(v) * (size_t)width + (size_t)floor(u)] = 1;
        n++;
    }
    if (!kept) return;   // (uniform)
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) n += __shfl_xor(n, off, 64);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(&kept[view], n);
}

// ------------------------------------------------------------------------------------------------ distance transform
__global__ void __launch_bounds__(EDT_COL_THREADS) k_edt_columns(int height, int width, const uint8_t* __restrict__ mask,
                                                                unsigned short* __restrict__ g) {
    const int x = blockIdx.x * EDT_COL_THREADS + threadIdx.x;
    if (x >= width) return;
    const size_t base = (size_t)blockIdx.y * (size_t)height * (size_t)width + (size_t)x;
    const uint8_t* __restrict__ m = mask + base;
    unsigned short* __restrict__ o = g + base;
    int run = EDT_NO_FEATURE;   // distance to the nearest feature above, or the sentinel
    for (int y = 0; y < height; y++) {
        const size_t at = (size_t)y * (size_t)width;
        run = m[at] ? 0 : (run == EDT_NO_FEATURE ? EDT_NO_FEATURE : run + 1);   // run + 1 <= height - 1 < the sentinel
        o[at] = (unsigned short)run;
    }
    run = EDT_NO_FEATURE;       // now: the nearest feature below
    for (int y = height - 1; y >= 0; y--) {
        const size_t at = (size_t)y * (size_t)width;
        const int down = o[at];
        run = down == 0 ? 0 : (run == EDT_NO_FEATURE ? EDT_NO_FEATURE : run + 1);
        if (run < down) o[at] = (unsigned short)run;
    }
}

__global__ void __launch_bounds__(SCORE_THREADS) k_edt_rows(int height, int width, const unsigned short* __restrict__ g,
                                                           int* __restrict__ dist2) {
    const long long plane = (long long)height * width;
    const long long p = (long long)blockIdx.x * SCORE_THREADS + threadIdx.x;
    if (p >= plane) return;
    const int y = (int)(p / width), x = (int)(p - (long long)y * width);
    const size_t row = (size_t)blockIdx.y * (size_t)plane + (size_t)y * (size_t)width;
    const unsigned short* __restrict__ gr = g + row;
    const int g0 = gr[x];
    int best = g0 == EDT_NO_FEATURE ? CGS_EDT_INF : g0 * g0;
    const int reach = max(x, width - 1 - x);
    for (int d = 1; d <= reach; d++) {
        const int d2 = d * d;
        if (d2 >= best) break;
        if (x - d >= 0) {
            const int a = gr[x - d];
            if (a != EDT_NO_FEATURE) best = min(best, d2 + a * a);
        }
        if (x + d < width) {
            const int b = gr[x + d];
            if (b != EDT_NO_FEATURE) best = min(best, d2 + b * b);
        }
    }
    dist2[row + (size_t)x] = best;
}

// ------------------------------------------------------------------------------------------------ reduction
struct ScoreWs {  // device workspace layout
    static size_t partials_offset(int V) { return ((size_t)V * sizeof(unsigned int) + 15) & ~(size_t)15; }
    static size_t bytes(int V) { return partials_offset(V) + (size_t)V * SCORE_BLOCKS * SCORE_SLOTS * 8; }
};

__global__ void __launch_bounds__(SCORE_THREADS) k_edge_score(int height, int width, const uint8_t* __restrict__ pred_mask,
                                                             const uint8_t* __restrict__ det_mask,
                                                             const int* __restrict__ pred_dist2,
                                                             const int* __restrict__ det_dist2, const ScoreTol tol,
                                                             unsigned int* __restrict__ counters,
                                                             long long* __restrict__ partials, long long* __restrict__ counts,
                                                             double* __restrict__ sums, uint8_t* __restrict__ both_nonempty) {
    constexpr int T = CGS_EDGE_SCORE_MAX_TOL, NI = 2 + 2 * T;   // integer slots
    const int v = blockIdx.y;
    const long long plane = (long long)height * width;
    const size_t base = (size_t)v * (size_t)plane;
    int cnt[NI];
#pragma unroll
    for (int k = 0; k < NI; k++) cnt[k] = 0;
    double s_pd = 0.0, s_dp = 0.0;
    // a thread sees at most 2^28 / (64 * 256) = 2^14 pixels: int counts
    for (long long i = (long long)blockIdx.x * SCORE_THREADS + threadIdx.x; i < plane; i += (long long)SCORE_BLOCKS * SCORE_THREADS) {
        if (pred_mask[base + i]) {
            const int d2 = det_dist2[base + i];
            cnt[0]++;
#pragma unroll
            for (int t = 0; t < T; t++) cnt[2 + t] += (t < tol.n && d2 <= tol.tol2[t]) ? 1 : 0;
            s_pd += sqrt((double)d2);
        }
        if (det_mask[base + i]) {
            const int d2 = pred_dist2[base + i];
            cnt[1]++;
#pragma unroll
            for (int t = 0; t < T; t++) cnt[2 + T + t] += (t < tol.n && d2 <= tol.tol2[t]) ? 1 : 0;
            s_dp += sqrt((double)d2);
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int k = 0; k < NI; k++) cnt[k] += __shfl_xor(cnt[k], off, 64);
        s_pd += __shfl_xor(s_pd, off, 64);
        s_dp += __shfl_xor(s_dp, off, 64);
    }
    constexpr int WAVES = SCORE_THREADS / 64;
    __shared__ int s_cnt[WAVES][NI];
    __shared__ double s_sum[WAVES][2];
    __shared__ long long s_tot[SCORE_SLOTS];
    __shared__ int s_last;
    if ((threadIdx.x & 63) == 0) {
        const int w = threadIdx.x >> 6;
#pragma unroll
        for (int k = 0; k < NI; k++) s_cnt[w][k] = cnt[k];
        s_sum[w][0] = s_pd;
        s_sum[w][1] = s_dp;
    }
    __syncthreads();
    long long* mine = partials + ((size_t)v * SCORE_BLOCKS + blockIdx.x) * SCORE_SLOTS;
    if (threadIdx.x < NI) {
        long long a = 0;
#pragma unroll
        for (int w = 0; w < WAVES; w++) a += s_cnt[w][threadIdx.x];
        mine[threadIdx.x] = a;
    } else if (threadIdx.x < SCORE_SLOTS) {
        const int k = threadIdx.x - NI;
        const double a = ((s_sum[0][k] + s_sum[1][k]) + s_sum[2][k]) + s_sum[3][k];
        mine[threadIdx.x] = __double_as_longlong(a);
    }
    __threadfence();
    __syncthreads();   // every slot of this workgroup is written and fenced before the counter moves
    if (threadIdx.x == 0) s_last = atomicAdd(&counters[v], 1u) == SCORE_BLOCKS - 1;
    __syncthreads();
    if (!s_last) return;   // (uniform)
    __threadfence();
    // the last workgroup of view v: every partial is visible; add them in index order (volatile: past the local cache)
    if (threadIdx.x < SCORE_SLOTS) {
        const volatile long long* p = partials + (size_t)v * SCORE_BLOCKS * SCORE_SLOTS + threadIdx.x;
        if (threadIdx.x < NI) {
            long long a = 0;
            for (int b = 0; b < SCORE_BLOCKS; b++) a += p[(size_t)b * SCORE_SLOTS];
            s_tot[threadIdx.x] = a;
        } else {
            double a = 0.0;
            for (int b = 0; b < SCORE_BLOCKS; b++) a += __longlong_as_double(p[(size_t)b * SCORE_SLOTS]);
            s_tot[threadIdx.x] = __double_as_longlong(a);
        }
    }
    __syncthreads();
    const bool both = s_tot[0] > 0 && s_tot[1] > 0;
    const int n_out = 2 + 2 * tol.n;   // counts[v] = (n_pred, n_det, pred_hits[n_tol], det_hits[n_tol])
    if ((int)threadIdx.x < n_out) {
        const int t = (int)threadIdx.x - 2;
        const int slot = t < 0 ? (int)threadIdx.x : (t < tol.n ? 2 + t : 2 + T + (t - tol.n));
        counts[(size_t)v * n_out + threadIdx.x] = (t < 0 || both) ? s_tot[slot] : 0;
    }
    if (threadIdx.x < 2) sums[2 * (size_t)v + threadIdx.x] = both ? __longlong_as_double(s_tot[NI + threadIdx.x]) : 0.0;
    if (threadIdx.x == 0) both_nonempty[v] = both ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------ launchers
hipError_t launch_point_mask(hipStream_t s, int P, const float* points, int V, const double* intr, const double* w2c,
                             int height, int width, uint8_t* mask, int* kept) {
    const size_t plane = (size_t)height * (size_t)width;
    hipError_t e = hipMemsetAsync(mask, 0, (size_t)V * plane, s);
    if (e != hipSuccess) return e;
    if (kept && (e = hipMemsetAsync(kept, 0, (size_t)V * sizeof(int), s)) != hipSuccess) return e;
    if (P == 0) return hipSuccess;
    const int blocks = std::max(1, (int)std::min<long long>(SCORE_POINT_BLOCKS_MAX, ((long long)P + SCORE_THREADS - 1) / SCORE_THREADS));
    ProfScope p("point_mask", s);
    for (int v0 = 0; v0 < V; v0 += SCORE_MAX_VIEWS) {
        const int nv = std::min(SCORE_MAX_VIEWS, V - v0);
        hipLaunchKernelGGL(k_point_mask, dim3(blocks, nv), dim3(SCORE_THREADS), 0, s, P, points, intr + 4 * (size_t)v0,
                           w2c + 12 * (size_t)v0, height, width, mask + (size_t)v0 * plane, kept ? kept + v0 : nullptr);
    }
    return hipSuccess;
}

size_t edt_workspace_bytes(int V, int height, int width) {
    return (size_t)std::max(V, 1) * (size_t)height * (size_t)width * sizeof(unsigned short);
}

void launch_edt_squared(hipStream_t s, int V, int height, int width, const uint8_t* mask, void* workspace, int* dist2) {
    const size_t plane = (size_t)height * (size_t)width;
    unsigned short* g = static_cast<unsigned short*>(workspace);
    const unsigned col_blocks = (unsigned)((width + EDT_COL_THREADS - 1) / EDT_COL_THREADS);
    const unsigned row_blocks = (unsigned)((plane + SCORE_THREADS - 1) / SCORE_THREADS);   // <= 2^28 / 256
    for (int v0 = 0; v0 < V; v0 += SCORE_MAX_VIEWS) {
        const int nv = std::min(SCORE_MAX_VIEWS, V - v0);
        const size_t off = (size_t)v0 * plane;
        {
            ProfScope p("edt_columns", s);
            hipLaunchKernelGGL(k_edt_columns, dim3(col_blocks, nv), dim3(EDT_COL_THREADS), 0, s, height, width, mask + off,
                               g + off);
        }
        ProfScope p("edt_rows", s);
        hipLaunchKernelGGL(k_edt_rows, dim3(row_blocks, nv), dim3(SCORE_THREADS), 0, s, height, width, g + off, dist2 + off);
    }
}

size_t edge_score_workspace_bytes(int V) { return ScoreWs::bytes(std::max(V, 1)); }

hipError_t launch_edge_score_reduce(hipStream_t s, int V, int height, int width, const uint8_t* pred_mask,
                                    const uint8_t* det_mask, const int* pred_dist2, const int* det_dist2, int n_tol,
                                    const int* tol2, void* workspace, int64_t* counts, double* sums,
                                    uint8_t* both_nonempty) {
    ScoreTol tol;
    tol.n = n_tol;
    for (int t = 0; t < CGS_EDGE_SCORE_MAX_TOL; t++) tol.tol2[t] = t < n_tol ? tol2[t] : 0;
    char* ws = static_cast<char*>(workspace);
    hipError_t e = hipMemsetAsync(ws, 0, (size_t)V * sizeof(unsigned int), s);   // the views' arrival counters
    if (e != hipSuccess) return e;
    const size_t plane = (size_t)height * (size_t)width;
    const int n_out = 2 + 2 * n_tol;
    ProfScope p("edge_score_reduce", s);
    for (int v0 = 0; v0 < V; v0 += SCORE_MAX_VIEWS) {
        const int nv = std::min(SCORE_MAX_VIEWS, V - v0);
        const size_t off = (size_t)v0 * plane;
        hipLaunchKernelGGL(k_edge_score, dim3(SCORE_BLOCKS, nv), dim3(SCORE_THREADS), 0, s, height, width, pred_mask + off,
                           det_mask + off, pred_dist2 + off, det_dist2 + off, tol,
                           reinterpret_cast<unsigned int*>(ws) + v0,
                           reinterpret_cast<long long*>(ws + ScoreWs::partials_offset(V)) + (size_t)v0 * SCORE_BLOCKS * SCORE_SLOTS,
                           reinterpret_cast<long long*>(counts) + (size_t)v0 * n_out, sums + 2 * (size_t)v0, both_nonempty + v0);
    }
    return hipSuccess;
}

}  // namespace cgs
