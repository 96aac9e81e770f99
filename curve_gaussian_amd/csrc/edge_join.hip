// Where the ends of the extracted edges land on OTHER edges (include/curvegs.h, cgs_end_attach): a test of all ends against
// all samples in 3D with a direction -- the shape of cgs_sample_cover (edge_dedupe.hip) with the 64-bit key of cgs_nn1
// (nn.hip).  ops/edge_join.py turns the keys into vertices, T-junctions and moved end points.
//
// The rule, frozen; every operation below is one IEEE fp32 operation in the written order (contraction
// into FMAs is off in this file), so numpy float32 arrays reproduce it bit for bit.  Edge e with n >= 1 samples has end 2e
// at its first sample i = off[e] and end 2e+1 at its last, i = off[e+1] - 1; an edge without samples has no end and its
// two keys stay NO_ATTACH.  For an end at sample i with point p:
//   t = pts[i] - pts[inner],  inner = i + min(1, n-1) (first end) or i - min(1, n-1) (last end): the OUTWARD tangent
//   q = (t.x*t.x + t.y*t.y) + t.z*t.z,  rq = reach2*q,  tq = tol2*q         (an edge of one sample: t = 0, q = 0)
// Sample j of edge b, w = pts[j] - p, w2 = (w.x*w.x + w.y*w.y) + w.z*w.z, s = (w.x*t.x + w.y*t.y) + w.z*t.z, is ACCEPTED
// iff b != a and
//   NEAR  w2 <= tol2                                                     or
//   TUBE  s > 0 and s*s <= rq and (w2*q) - (s*s) <= tq                    or
//   ENDS  j is the first or the last sample of b and s > 0 and w2 <= reach2
//   key[end] = the minimum over the accepted samples of (uint64(bits(w2)) << 32) | uint32(j), NO_ATTACH = 2^64 - 1
// w2 >= +0, so its bits order like its value: the least key is the nearest accepted sample, the lowest index among equals.
// An integer minimum does not depend on the order of arrival: the result cannot depend on the launch geometry.
//
//   k_attach_prepare  one thread per sample and per end.  Per sample the float4 that the attach kernel stages: (x, y, z,
//                     tag), tag = the edge of the sample (a binary search of the offsets) with bit 31 set on the first
//                     and the last sample of an edge.  Per end its query record -- (p, edge), (t, q), (rq, tq) -- and
//                     NO_ATTACH into its key; an end that does not exist gets edge -1.
//   k_end_attach      256 queries per workgroup, one per lane, the record in registers; the candidates in tiles of 256
//                     through LDS (one float4 per sample, every lane reads the same address: broadcast reads); the
//                     candidate tiles split over grid.y as cover_tiles_per_split does -- the queries are few (2E) and the
//                     candidates many --; one 64-bit atomicMin per (query, split), none when the lane found nothing.
//                     A lane past the last sample stages a NaN point: every comparison of the rule is false for it,
//                     so the tail takes the same path as a full tile.  No cull: the ends of consecutive edges are not
//                     spatially coherent, a query box would be loose.
#include <algorithm>

#include "kernels.h"

namespace cgs {

constexpr int EJ_BLOCK = 256;        // lanes per workgroup = queries per workgroup = samples per tile
constexpr int EJ_TARGET_WGS = 2048;  // ~8 workgroups per CU on 256 CUs
constexpr unsigned EJ_END_FLAG = 0x80000000u;   // in a sample's tag: the first or the last sample of its edge
constexpr unsigned EJ_NONE = 0xffffffffu;       // no accepted sample yet: above the bits of every w2 (+inf is 0x7f800000)

struct AttachWork {      // carved from the workspace
    float4* sm;          // [P]   x, y, z, tag
    float4* qp;          // [2E]  p.x, p.y, p.z, edge (bits; -1: no such end)
    float4* qt;          // [2E]  t.x, t.y, t.z, q
    float2* qr;          // [2E]  rq, tq
};

static AttachWork attach_work(void* workspace, int P, int E) {
    char* c = (char*)workspace;
    AttachWork w;
    carve(c, w.sm, (size_t)P);
    carve(c, w.qp, 2 * (size_t)E);
    carve(c, w.qt, 2 * (size_t)E);
    carve(c, w.qr, 2 * (size_t)E);
    return w;
}

size_t end_attach_workspace_bytes(int P, int E) {
    const size_t n = (size_t)(P > 0 ? P : 0), m = 2 * (size_t)(E > 0 ? E : 0);
    return 4 * 128 + n * sizeof(float4) + m * (2 * sizeof(float4) + sizeof(float2));
}

__global__ void __launch_bounds__(EJ_BLOCK) k_attach_prepare(int P, const float* __restrict__ pts, int E,
                                                             const int* __restrict__ off, float tol2, float reach2,
                                                             AttachWork w, unsigned long long* __restrict__ keys) {
#pragma clang fp contract(off)
    const long long i = (long long)blockIdx.x * EJ_BLOCK + threadIdx.x;
    if (i < P) {
        // the edge of sample i: the last e with off[e] <= i; empty edges repeat an offset and are stepped over.
        // off[0] = 0 <= i < P = off[E], so 0 <= e < E and off[e + 1] > i
        int a = 0, b = E;   // off[a] <= i < off[b]
        while (b - a > 1) {
            const int m = a + (b - a) / 2;
            if ((long long)off[m] <= i) a = m; else b = m;
        }
        const bool end = i == (long long)off[a] || i == (long long)off[a + 1] - 1;
        const size_t self = 3 * (size_t)i;
        w.sm[i] = make_float4(pts[self], pts[self + 1], pts[self + 2], __uint_as_float((unsigned)a | (end ? EJ_END_FLAG : 0u)));
    }
    if (i < 2 * (long long)E) {
        const int e = (int)(i >> 1);
        const long long first = off[e], n = (long long)off[e + 1] - first;
        float4 p = make_float4(0.f, 0.f, 0.f, __int_as_float(-1)), t = make_float4(0.f, 0.f, 0.f, 0.f);
        if (n > 0) {
            const long long step = n > 1 ? 1 : 0;
            const long long at = (i & 1) ? first + n - 1 : first, inner = (i & 1) ? at - step : at + step;
            const size_t self = 3 * (size_t)at, in = 3 * (size_t)inner;
            p = make_float4(pts[self], pts[self + 1], pts[self + 2], __int_as_float(e));
            t.x = p.x - pts[in], t.y = p.y - pts[in + 1], t.z = p.z - pts[in + 2];
            t.w = (t.x * t.x + t.y * t.y) + t.z * t.z;
        }
        w.qp[i] = p;
        w.qt[i] = t;
        w.qr[i] = make_float2(reach2 * t.w, tol2 * t.w);
        keys[i] = ~0ull;
    }
}

__global__ void __launch_bounds__(EJ_BLOCK) k_end_attach(int P, int E, AttachWork w, int tiles_per_split, float tol2,
                                                         float reach2, unsigned long long* __restrict__ keys) {
#pragma clang fp contract(off)
    __shared__ float4 s_sm[EJ_BLOCK];
    const long long i = (long long)blockIdx.x * EJ_BLOCK + threadIdx.x;
    float4 p = make_float4(0.f, 0.f, 0.f, __int_as_float(-1)), t = make_float4(0.f, 0.f, 0.f, 0.f);
    float2 r = make_float2(0.f, 0.f);
    if (i < 2 * (long long)E) {
        p = w.qp[i];
        t = w.qt[i];
        r = w.qr[i];
    }
    const unsigned ea = __float_as_uint(p.w);
    const bool live = (int)ea >= 0;   // past the last end, or the end of an edge without samples: nothing to attach
    const long long tiles = ((long long)P + EJ_BLOCK - 1) / EJ_BLOCK;
    const long long t0 = (long long)blockIdx.y * tiles_per_split;
    const long long t1 = t0 + tiles_per_split < tiles ? t0 + tiles_per_split : tiles;
    const float nan = __uint_as_float(0x7fc00000u);
    unsigned best = EJ_NONE, best_j = 0;
    for (long long tile = t0; tile < t1; tile++) {
        const long long j = tile * EJ_BLOCK + threadIdx.x;
        s_sm[threadIdx.x] = j < P ? w.sm[j] : make_float4(nan, nan, nan, __uint_as_float(~EJ_END_FLAG));
        __syncthreads();
        const unsigned j0 = (unsigned)(tile * EJ_BLOCK);   // sample indices fit 31 bits
#pragma unroll 8
        for (int k = 0; k < EJ_BLOCK; k++) {
            const float4 c = s_sm[k];
            const unsigned tag = __float_as_uint(c.w);
            const float wx = c.x - p.x, wy = c.y - p.y, wz = c.z - p.z;
            const float w2 = (wx * wx + wy * wy) + wz * wz;
            const float s = (wx * t.x + wy * t.y) + wz * t.z;
            const float ss = s * s;
            const float side = w2 * t.w - ss;
            const bool near = w2 <= tol2;
            const bool tube = ss <= r.x && side <= r.y;
            const bool ends = (tag & EJ_END_FLAG) != 0u && w2 <= reach2;
            const bool ok = (tag & ~EJ_END_FLAG) != ea && (near || (s > 0.f && (tube || ends)));
            const unsigned bits = __float_as_uint(w2);
            // strict: within a split j ascends, so the lowest index of equal distances stays
            const bool take = ok && bits < best;
            best = take ? bits : best;
            best_j = take ? j0 + (unsigned)k : best_j;
        }
        __syncthreads();
    }
    if (live && best != EJ_NONE) atomicMin(&keys[i], ((unsigned long long)best << 32) | best_j);
}

// Candidate tiles per split: enough splits to bring the grid to ~EJ_TARGET_WGS workgroups, as cover_tiles_per_split.
static int attach_tiles_per_split(long long query_tiles, long long tiles) {
    long long splits = (EJ_TARGET_WGS + query_tiles - 1) / query_tiles;
    splits = std::max(1ll, std::min(splits, tiles));
    return (int)((tiles + splits - 1) / splits);
}

void launch_end_attach(hipStream_t s, int P, const float* points, int E, const int* offsets, float tol2, float reach2,
                       unsigned long long* keys, void* workspace) {
    const AttachWork w = attach_work(workspace, P, E);
    const long long query_tiles = (2ll * E + EJ_BLOCK - 1) / EJ_BLOCK;   // at most 2^24: one grid dimension
    const long long tiles = ((long long)P + EJ_BLOCK - 1) / EJ_BLOCK;
    { ProfScope p("attach_prepare", s);
      hipLaunchKernelGGL(k_attach_prepare, dim3((unsigned)std::max(query_tiles, tiles)), dim3(EJ_BLOCK), 0, s, P, points, E,
                         offsets, tol2, reach2, w, keys); }
    if (P == 0) return;   // no candidate: every key stays NO_ATTACH
    const int per = attach_tiles_per_split(query_tiles, tiles);
    const unsigned splits = (unsigned)((tiles + per - 1) / per);   // at most EJ_TARGET_WGS
    { ProfScope p("end_attach", s);
      hipLaunchKernelGGL(k_end_attach, dim3((unsigned)query_tiles, splits), dim3(EJ_BLOCK), 0, s, P, E, w, per, tol2, reach2,
                         keys); }
}

}  // namespace cgs
