// Which samples of the extracted edges a higher-ranked edge already covers (include/curvegs.h, cgs_sample_cover): an
// all-pairs, sample-against-sample test in 3D -- the shape of cgs_nn1 (nn.hip) plus a direction test, a priority and culling.
//
// The rule, frozen; every operation below is one IEEE fp32 operation in the written order (contraction
// into FMAs is off in this file), so numpy float32 arrays reproduce it bit for bit.  Sample i is sample k of the n samples
// of edge a, sample j lies on edge b:
//   t_i = p[off[a] + min(k + 1, n - 1)] - p[off[a] + max(k - 1, 0)],  q_i = (t.x*t.x + t.y*t.y) + t.z*t.z
//   j COVERS i iff  rank[b] < rank[a]
//              and  d2 = (dx*dx + dy*dy) + dz*dz <= tol2,  dx = p_i.x - p_j.x ...
//              and  dot*dot >= (cos2 * q_i) * q_j,  dot = (t_i.x*t_j.x + t_i.y*t_j.y) + t_i.z*t_j.z
//   cover[i] = the minimum of rank[b] over the samples that cover i, INT32_MAX when there is none
// An integer minimum does not depend on the order of arrival: the result cannot depend on the launch geometry.
//
//   k_cover_prepare   one thread per sample: the edge of the sample (a binary search of the offsets), the two float4 that
//                     the cover kernel stages -- (x, y, z, rank bits) and (tx, ty, tz, q) --, INT32_MAX into cover[i]; per
//                     tile of 256 consecutive samples the fp32 bounding box and the least and greatest rank, by wave
//                     reductions.  The samples of one edge are consecutive, so the boxes are tight.
//   k_sample_cover    256 queries per workgroup, one per lane, point, tangent, q and rank in registers; the candidates in
//                     tiles of 256 through LDS (two float4 per sample, 8 KB, every lane reads the same address: broadcast
//                     reads); the candidate tiles split over grid.y as nn1_per_split does; one atomicMin per (query,
//                     split), none when the lane found nothing.  Before a tile is staged a workgroup-uniform cull skips it:
//       (a) its least rank is >= the query tile's greatest rank: nothing in it outranks any query;
//       (b) on some axis the gap g = fl(lo_tile - hi_queries), or the mirrored one, is positive and fl(g*g) > tol2.
//     (b) IS CONSERVATIVE.  Take any query p and candidate r inside the two boxes and the axis of the gap, say x with
//     lo_tile.x > hi_queries.x.  Exactly, r.x - p.x >= lo_tile.x - hi_queries.x > 0.  Rounding to nearest is monotone, so
//     |dx| = fl(r.x - p.x) >= fl(lo_tile.x - hi_queries.x) = g > 0, and fl(dx*dx) >= fl(g*g) for the same reason (a product
//     of non-negative factors grows with each factor).  The other two squares are >= 0, and fl(a + b) >= a for b >= 0 (a
//     is itself representable), so d2 = fl(fl(dx*dx + dy*dy) + dz*dz) >= fl(dx*dx) >= fl(g*g) > tol2: the pair fails the
//     distance test.  The points are finite (the ops layer rejects others), so no comparison meets a NaN.
#include <algorithm>
#include <climits>

#include "kernels.h"

namespace cgs {

constexpr int DD_BLOCK = 256;        // lanes per workgroup = queries per workgroup = samples per tile
constexpr int DD_WAVES = DD_BLOCK / 64;
constexpr int DD_TARGET_WGS = 2048;  // ~8 workgroups per CU on 256 CUs before the candidates are split further

struct CoverWork {       // carved from the workspace; M = the tiles of 256 samples
    float4* pr;          // [P]  x, y, z, rank bits
    float4* tq;          // [P]  tx, ty, tz, q
    float4* lo;          // [M]  the least x, y, z and (bits) the least rank of the tile
    float4* hi;          // [M]  the greatest
};

__host__ __device__ static inline long long cover_tiles(int P) { return ((long long)P + DD_BLOCK - 1) / DD_BLOCK; }

static CoverWork cover_work(void* workspace, int P) {
    char* c = (char*)workspace;
    CoverWork w;
    carve(c, w.pr, (size_t)P);
    carve(c, w.tq, (size_t)P);
    carve(c, w.lo, (size_t)cover_tiles(P));
    carve(c, w.hi, (size_t)cover_tiles(P));
    return w;
}

size_t sample_cover_workspace_bytes(int P) {
    const size_t n = (size_t)(P > 0 ? P : 0), m = (size_t)cover_tiles(P > 0 ? P : 0);
    return 4 * 128 + 2 * n * sizeof(float4) + 2 * m * sizeof(float4);
}

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v = fminf(v, __shfl_xor(v, s, 64));
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v = fmaxf(v, __shfl_xor(v, s, 64));
    return v;
}
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v = min(v, __shfl_xor(v, s, 64));
    return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v = max(v, __shfl_xor(v, s, 64));
    return v;
}

__global__ void __launch_bounds__(DD_BLOCK) k_cover_prepare(int P, const float* __restrict__ pts, int E,
                                                            const int* __restrict__ off, const int* __restrict__ rank,
                                                            CoverWork w, int* __restrict__ cover) {
#pragma clang fp contract(off)
    __shared__ float s_lo[DD_WAVES][3], s_hi[DD_WAVES][3];
    __shared__ int s_rlo[DD_WAVES], s_rhi[DD_WAVES];
    const long long i = (long long)blockIdx.x * DD_BLOCK + threadIdx.x;
    const bool live = i < P;
    const float inf = __int_as_float(0x7f800000);
    float x = inf, y = inf, z = inf, X = -inf, Y = -inf, Z = -inf;   // a dead lane is neutral in both reductions
    int rlo = INT_MAX, rhi = INT_MIN;
    if (live) {
        // the edge of sample i: the last e with off[e] <= i; empty edges repeat an offset and are stepped over.
        // off[0] = 0 <= i < P = off[E], so 0 <= e < E and off[e + 1] > i
        int a = 0, b = E;   // off[a] <= i < off[b]
        while (b - a > 1) {
            const int m = a + (b - a) / 2;
            if ((long long)off[m] <= i) a = m; else b = m;
        }
        const long long first = off[a], n = (long long)off[a + 1] - first, k = i - first;
        const size_t self = 3 * (size_t)i, next = 3 * (size_t)(first + min(k + 1, n - 1)), prev = 3 * (size_t)(first + max(k - 1, 0ll));
        x = X = pts[self], y = Y = pts[self + 1], z = Z = pts[self + 2];
        const float tx = pts[next] - pts[prev], ty = pts[next + 1] - pts[prev + 1], tz = pts[next + 2] - pts[prev + 2];
        const float q = (tx * tx + ty * ty) + tz * tz;
        rlo = rhi = rank[a];
        w.pr[i] = make_float4(x, y, z, __int_as_float(rlo));
        w.tq[i] = make_float4(tx, ty, tz, q);
        cover[i] = INT_MAX;
    }
    x = wave_min(x), y = wave_min(y), z = wave_min(z), X = wave_max(X), Y = wave_max(Y), Z = wave_max(Z);
    rlo = wave_min(rlo), rhi = wave_max(rhi);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s_lo[wave][0] = x, s_lo[wave][1] = y, s_lo[wave][2] = z, s_hi[wave][0] = X, s_hi[wave][1] = Y, s_hi[wave][2] = Z;
        s_rlo[wave] = rlo, s_rhi[wave] = rhi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {   // the tile's first sample exists: the grid has no empty tile
#pragma unroll
        for (int v = 1; v < DD_WAVES; v++) {
            x = fminf(x, s_lo[v][0]), y = fminf(y, s_lo[v][1]), z = fminf(z, s_lo[v][2]);
            X = fmaxf(X, s_hi[v][0]), Y = fmaxf(Y, s_hi[v][1]), Z = fmaxf(Z, s_hi[v][2]);
            rlo = min(rlo, s_rlo[v]), rhi = max(rhi, s_rhi[v]);
        }
        w.lo[blockIdx.x] = make_float4(x, y, z, __int_as_float(rlo));
        w.hi[blockIdx.x] = make_float4(X, Y, Z, __int_as_float(rhi));
    }
}

// the gap between two intervals on one axis rules every pair out (see the head of the file)
__device__ __forceinline__ bool axis_apart(float lo_a, float hi_a, float lo_b, float hi_b, float tol2) {
    const float g = lo_a - hi_b, h = lo_b - hi_a;
    return (g > 0.f && g * g > tol2) || (h > 0.f && h * h > tol2);
}

__global__ void __launch_bounds__(DD_BLOCK) k_sample_cover(int P, CoverWork w, int tiles_per_split, float tol2, float cos2,
                                                           int* __restrict__ cover) {
#pragma clang fp contract(off)
    __shared__ float4 s_pr[DD_BLOCK], s_tq[DD_BLOCK];
    const long long i = (long long)blockIdx.x * DD_BLOCK + threadIdx.x;
    const bool live = i < P;
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f), t = p;
    int ra = INT_MIN;   // a dead lane: nothing outranks it
    if (live) {
        p = w.pr[i];
        t = w.tq[i];
        ra = __float_as_int(p.w);
    }
    const float cq = cos2 * t.w;
    const float4 qlo = w.lo[blockIdx.x], qhi = w.hi[blockIdx.x];   // the queries are tile blockIdx.x: its box, its ranks
    const int q_rank_max = __float_as_int(qhi.w);
    const long long tiles = cover_tiles(P);
    const long long t0 = (long long)blockIdx.y * tiles_per_split;
    const long long t1 = t0 + tiles_per_split < tiles ? t0 + tiles_per_split : tiles;
    int best = INT_MAX;
    for (long long tile = t0; tile < t1; tile++) {
        const float4 lo = w.lo[tile], hi = w.hi[tile];   // workgroup-uniform
        if (__float_as_int(lo.w) >= q_rank_max) continue;
        if (axis_apart(lo.x, hi.x, qlo.x, qhi.x, tol2) || axis_apart(lo.y, hi.y, qlo.y, qhi.y, tol2) ||
            axis_apart(lo.z, hi.z, qlo.z, qhi.z, tol2))
            continue;
        const long long j = tile * DD_BLOCK + threadIdx.x;
        // past the last sample: a rank that outranks nothing
        s_pr[threadIdx.x] = j < P ? w.pr[j] : make_float4(0.f, 0.f, 0.f, __int_as_float(INT_MAX));
        s_tq[threadIdx.x] = j < P ? w.tq[j] : make_float4(0.f, 0.f, 0.f, 0.f);
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < DD_BLOCK; k++) {
            const float4 r = s_pr[k], u = s_tq[k];
            const int rb = __float_as_int(r.w);
            const float dx = p.x - r.x, dy = p.y - r.y, dz = p.z - r.z;
            const float d2 = (dx * dx + dy * dy) + dz * dz;
            const float dot = (t.x * u.x + t.y * u.y) + t.z * u.z;
            const bool covers = rb < ra && d2 <= tol2 && dot * dot >= cq * u.w;
            best = covers ? min(best, rb) : best;
        }
        __syncthreads();
    }
    if (live && best != INT_MAX) atomicMin(&cover[i], best);
}

// Tiles per split: enough splits to bring the grid to ~DD_TARGET_WGS workgroups, as nn1_per_split.
static int cover_tiles_per_split(long long tiles) {
    long long splits = (DD_TARGET_WGS + tiles - 1) / tiles;
    splits = std::max(1ll, std::min(splits, tiles));
    return (int)((tiles + splits - 1) / splits);
}

void launch_sample_cover(hipStream_t s, int P, const float* points, int E, const int* offsets, const int* rank, float tol2,
                         float cos2, int* cover, void* workspace) {
    const CoverWork w = cover_work(workspace, P);
    const long long tiles = cover_tiles(P);   // at most 2^23: one grid dimension
    const int per = cover_tiles_per_split(tiles);
    const unsigned splits = (unsigned)((tiles + per - 1) / per);   // at most DD_TARGET_WGS
    { ProfScope p("cover_prepare", s);
      hipLaunchKernelGGL(k_cover_prepare, dim3((unsigned)tiles), dim3(DD_BLOCK), 0, s, P, points, E, offsets, rank, w, cover); }
    { ProfScope p("sample_cover", s);
      hipLaunchKernelGGL(k_sample_cover, dim3((unsigned)tiles, splits), dim3(DD_BLOCK), 0, s, P, w, per, tol2, cos2, cover); }
}

}  // namespace cgs
