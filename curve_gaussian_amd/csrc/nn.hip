// Exact 1-nearest-neighbour between two point sets, brute force: for every query point the distance to, and the index
// of, its nearest reference point.  Replaces the point_cloud_utils.k_nearest_neighbors(x, y, k=1) KD-tree queries of the
// reference's evaluator (edge_extraction/eval_utils.py:77-115, 195-249) and its cKDTree query (eval_ABC.py:27-38).
//
// Shape: one query per lane, 256-lane workgroups; the reference set is cut into `splits` contiguous chunks (grid.y) so
// that a few thousand queries still fill the chip, and each workgroup stages its chunk through LDS 256 points at a time
// as float4 (every lane reads the same address: broadcast reads).  The running minimum stays in registers; the splits
// are merged with one 64-bit atomicMin per (query, split) on key = (float_bits(d2) << 32) | index.  d2 >= 0, so its bit
// pattern orders like its value and the smallest key is the smallest distance with the LOWEST index among equals: the
// result does not depend on the order the workgroups arrive in, with no second pass.  A closing pass takes the root.
//
// d2 is the IEEE fp32 value of (dx*dx + dy*dy) + dz*dz (contraction into FMAs is off in this file), never the GEMM
// expansion |q|^2 + |r|^2 - 2 q.r, which cancels to ~1e-2 relative error at the 5 mm thresholds of the metrics.
#include <cfloat>

#include "kernels.h"

namespace cgs {

constexpr int NN_BLOCK = 256;        // lanes per workgroup = queries per workgroup = reference points per LDS tile
constexpr int NN_TARGET_WGS = 2048;  // ~8 workgroups per CU on 256 CUs before the reference set is split further

__global__ void __launch_bounds__(NN_BLOCK) k_nn1_init(int n, unsigned long long* __restrict__ keys) {
    const int i = blockIdx.x * NN_BLOCK + threadIdx.x;
    if (i < n) keys[i] = ~0ull;
}

__global__ void __launch_bounds__(NN_BLOCK) k_nn1_partial(int n_query, const float* __restrict__ query, int n_ref,
                                                         const float* __restrict__ ref, int per_split,
                                                         unsigned long long* __restrict__ keys) {
#pragma clang fp contract(off)
    __shared__ float4 tile[NN_BLOCK];
    const int i = blockIdx.x * NN_BLOCK + threadIdx.x;
    const bool live = i < n_query;
    float qx = 0.f, qy = 0.f, qz = 0.f;
    if (live) {
        qx = query[3 * (size_t)i];
        qy = query[3 * (size_t)i + 1];
        qz = query[3 * (size_t)i + 2];
    }
    const int r0 = blockIdx.y * per_split;
    const int r1 = min(n_ref, r0 + per_split);
    float best = __int_as_float(0x7f800000);   // +inf: an all-inf (or NaN) row keeps the chunk's first index
    int bi = r0;
    for (int t0 = r0; t0 < r1; t0 += NN_BLOCK) {
        const int cnt = min(NN_BLOCK, r1 - t0);
        if ((int)threadIdx.x < cnt) {
            const size_t j = (size_t)(t0 + threadIdx.x);
            tile[threadIdx.x] = make_float4(ref[3 * j], ref[3 * j + 1], ref[3 * j + 2], 0.f);
        }
        __syncthreads();
        if (cnt == NN_BLOCK) {
#pragma unroll 16
            for (int k = 0; k < NN_BLOCK; k++) {
                const float4 r = tile[k];
                const float dx = qx - r.x, dy = qy - r.y, dz = qz - r.z;
                const float d2 = dx * dx + dy * dy + dz * dz;
                if (d2 < best) { best = d2; bi = t0 + k; }   // strict: ascending k keeps the lowest index of equals
            }
        } else {
            for (int k = 0; k < cnt; k++) {
                const float4 r = tile[k];
                const float dx = qx - r.x, dy = qy - r.y, dz = qz - r.z;
                const float d2 = dx * dx + dy * dy + dz * dz;
                if (d2 < best) { best = d2; bi = t0 + k; }
            }
        }
        __syncthreads();
    }
    if (live && r0 < r1) {
        const unsigned long long key = ((unsigned long long)__float_as_uint(best) << 32) | (unsigned int)bi;
        atomicMin(&keys[i], key);
    }
}

__global__ void __launch_bounds__(NN_BLOCK) k_nn1_finish(int n, const unsigned long long* __restrict__ keys,
                                                        float* __restrict__ dist, int* __restrict__ index) {
    const int i = blockIdx.x * NN_BLOCK + threadIdx.x;
    if (i >= n) return;
    const unsigned long long key = keys[i];
    dist[i] = sqrtf(__uint_as_float((unsigned int)(key >> 32)));
    index[i] = (int)(unsigned int)key;
}

size_t nn1_workspace_bytes(int n_query) {
    return 128 + (size_t)(n_query > 0 ? n_query : 1) * sizeof(unsigned long long);
}

// Reference points per split: whole LDS tiles, enough splits to bring the grid to ~NN_TARGET_WGS workgroups.
static int nn1_per_split(int n_query, int n_ref) {
    const int qblocks = (n_query + NN_BLOCK - 1) / NN_BLOCK;
    const int tiles = (n_ref + NN_BLOCK - 1) / NN_BLOCK;
    int splits = (NN_TARGET_WGS + qblocks - 1) / qblocks;
    splits = max(1, min(splits, tiles));
    const int tiles_per_split = (tiles + splits - 1) / splits;
    return tiles_per_split * NN_BLOCK;
}

void launch_nn1(hipStream_t s, int n_query, const float* query, int n_ref, const float* ref, float* dist, int* index,
                void* workspace) {
    char* c = (char*)workspace;
    unsigned long long* keys;
    carve(c, keys, (size_t)n_query);
    const int qblocks = (n_query + NN_BLOCK - 1) / NN_BLOCK;
    const int per = nn1_per_split(n_query, n_ref);
    const int splits = (int)(((long long)n_ref + per - 1) / per);
    { ProfScope p("nn1_init", s); hipLaunchKernelGGL(k_nn1_init, dim3(qblocks), dim3(NN_BLOCK), 0, s, n_query, keys); }
    { ProfScope p("nn1_partial", s);
      hipLaunchKernelGGL(k_nn1_partial, dim3(qblocks, splits), dim3(NN_BLOCK), 0, s, n_query, query, n_ref, ref, per, keys); }
    { ProfScope p("nn1_finish", s);
      hipLaunchKernelGGL(k_nn1_finish, dim3(qblocks), dim3(NN_BLOCK), 0, s, n_query, (const unsigned long long*)keys, dist, index); }
}

}  // namespace cgs
