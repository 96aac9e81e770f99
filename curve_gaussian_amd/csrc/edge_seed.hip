// Multi-view voxel vote: where do the edge maps of a scan say the edges are?  (include/curvegs.h, cgs_pack_near_bits /
// cgs_voxel_votes / cgs_voxel_moments / cgs_ray_claims / cgs_ray_wins and the three _depth siblings.)  Every voxel centre
// of a regular grid is projected into every view and counts the views that see it and the views in which it lands within a tolerance of a detected edge
// pixel; the kept voxels around a seed then give the seed's direction through their integer second moments; on request the
// kept voxels first claim the pixels they land on and only those that win their claims stay.  Five kernels:
//   k_pack_near_bits   one thread per pixel of the PADDED row (32 * stride pixels, stride = ceil(W / 32) words): the bit is
//                      dist2 <= tol2 inside the image and 0 in the padding, one wave ballot gives two words, lanes 0 and 32
//                      store them.  A padded plane is a whole number of words, so the linear pixel index / 32 is the word
//                      index and a wave may straddle two rows.  Every word is written, padding included: no memset.
//   seed_walk          the walk that the three kernels below share, written once: the centre of a voxel is
//                      lo + (i + 0.5) * step in float64 without contraction, rounded to float32 (seed_centre): the point
//                      that is projected, by nv_project_xyz (point_projection.h), the device function of
//                      cgs_project_points / cgs_point_mask.  The thread loops over the views; the camera index is
//                      wave-uniform, so the 16 doubles of a camera are scalar loads, as in visibility.hip.  For every view
//                      that keeps the centre, seed_pixel gives its pixel and the pixel's near bit, and the kernel's own
//                      lambda gets (v, px, py, near).  A pixel that differed between the vote and the claim would be a bug
//                      that no tolerance hides: there is one walk for it to differ in.  A template over GATED: false is the
//                      walk as it always was (nv_verdict<false> is nv_project_xyz and nothing else; the gate is not read);
//                      true is the walk of the _depth entries -- nv_verdict<true> holds the centre's camera depth against
//                      the view's float32 depth plane (nv_hidden, the one occlusion rule), a view that hides the centre is
//                      not seen by the lambda and its near bit is not gathered: one float32 gather more per kept pair, one
//                      gather of a word less per hidden pair.  The walk returns the number of views that hid the centre.
//   k_voxel_votes      one thread per voxel, linear index with x fastest, so the lanes of a wave are neighbours along x and
//                      gather neighbouring pixels.  The walk counts the views that keep the centre and those whose bit is
//                      set.  Both counts stay in registers; one plain 16-bit store each at the end (a read-add-store of the
//                      thread's own voxel with `accumulate`).  No atomics, no LDS: the result does not depend on the launch
//                      geometry.  The packed masks are the only gathered data: 1600x1200 is 240 KB a view, 24 MB for 100
//                      views.
//   k_voxel_moments    one wave per seed, four seeds per block.  The lanes walk the (dy, dz) rows of the seed's window, at
//                      most 31 x 31 of them; a row inside the grid whose half span h = isqrt(r^2 - dy^2 - dz^2) exists
//                      covers x = cx - h .. cx + h clipped to the grid, at most 31 voxels in at most two words: plain
//                      loads, a 64-bit shift and a mask leave the row's kept voxels, and the ten integers are summed from
//                      the set bits in registers.  One shuffle reduction per wave, lane 0 stores the ten values: every
//                      output word is written, no memset.  Integers only, no atomics, no LDS, no barrier (a wave without a
//                      seed leaves at once): the result does not depend on the launch geometry.
//   k_ray_claims       one thread per LISTED voxel (the kept voxels, ascending linear indices), the same walk.  Where the
//                      voxel hits, its support goes into best[v][y][x] by atomicMax on unsigned int: the one atomic of
//                      this file, and an integer maximum does not depend on the order, so the result still does not depend
//                      on the launch geometry.
//   k_ray_wins         one thread per listed voxel, the same walk.  Where the voxel hits, the maximum of best over the
//                      (2 w + 1)^2 window around its pixel, clipped to the image, by plain loads; the view is won when
//                      support + margin (32 bits) reaches it.  The count stays in a register; one plain 16-bit store at the
//                      end (a read-add-store of the thread's own word with `accumulate`).  No atomics, no LDS, no barrier.
//                      An index outside the grid (the caller's error) reads nothing, claims nothing and wins nothing.
//   The three kernels are templates over the same GATED; the gated k_voxel_votes stores the walk's hidden count as a third
//   uint16 per voxel when asked (NULL allowed), under the rule of `accumulate`: seen + hidden of the gated vote is seen of
//   the ungated one, voxel for voxel.  No atomic is added: the atomicMax of k_ray_claims stays the only one.
// Voxel, map, keep-bit, depth and pixel offsets are 64-bit.
#include <algorithm>

#include "kernels.h"
#include "point_projection.h"
#include "seed_centre.h"   // seed_centre: the lattice, shared with tsdf.hip

namespace cgs {

constexpr int SEED_THREADS = 256;        // 4 waves
constexpr int SEED_MAX_VIEWS = 65535;    // grid.y of the packing launch
constexpr int MOMENT_WAVES = SEED_THREADS / 64;   // seeds per block of k_voxel_moments
constexpr int MOMENT_VALUES = 10;        // m, the three first and the six second moments

__global__ void __launch_bounds__(SEED_THREADS) k_pack_near_bits(int height, int width, int stride,
                                                                const int* __restrict__ dist2, int tol2,
                                                                unsigned int* __restrict__ bits) {
    const long long padded = (long long)height * stride * 32;   // <= 16384 * 16384: a multiple of 32
    const long long p = (long long)blockIdx.x * SEED_THREADS + threadIdx.x;
    const int view = blockIdx.y;
    bool near = false;
    if (p < padded) {
        const int y = (int)(p / (32 * stride)), x = (int)(p - (long long)y * (32 * stride));
        if (x < width) near = dist2[((size_t)view * (size_t)height + (size_t)y) * (size_t)width + (size_t)x] <= tol2;
    }
    const unsigned long long b = __ballot(near);   // every lane of the wave arrives here
    const int lane = threadIdx.x & 63;
    if ((lane & 31) == 0 && p < padded)            // p is a multiple of 32 here: p / 32 is this half wave's word
        bits[(size_t)view * (size_t)height * (size_t)stride + (size_t)(p >> 5)] = (unsigned int)(lane ? b >> 32 : b);
}

// True if view `c` keeps the centre and, when GATED, does not hide it (nv_verdict, point_projection.h); then (px, py) is its
// pixel and `near` the pixel's bit in the view's packed mask.  `hid`, written only when GATED: the view keeps the centre and
// hides it -- no word of the mask is gathered for it.
template <bool GATED>
__device__ inline bool seed_pixel(const NvCam& c, double X, double Y, double Z, double wd, double hd,
                                  const unsigned int* __restrict__ view_bits, int stride,
                                  const float* __restrict__ depth_plane, int width, double slack, unsigned int& px,
                                  unsigned int& py, bool& near, bool& hid) {
#pragma clang fp contract(off)
    double pu, pv;
    const NvVerdict verdict = nv_verdict<GATED>(c, X, Y, Z, wd, hd, depth_plane, width, slack, pu, pv);
    if (GATED) hid = verdict == NV_HIDDEN;
    if (verdict != NV_VISIBLE) return false;
    // 0 <= pu < W and 0 <= pv < H: the pixel is inside the view, its word inside the view's plane
    px = (unsigned int)floor(pu);
    py = (unsigned int)floor(pv);
    const unsigned int w = view_bits[(size_t)py * (size_t)stride + (size_t)(px >> 5)];
    near = ((w >> (px & 31u)) & 1u) != 0u;
    return true;
}

// The walk of the file header: f(v, px, py, near) for every view v that keeps the centre of the voxel with linear index `id`
// and, when GATED, does not hide it.  Returns the number of views that keep the centre and hide it (0 when not GATED).
template <bool GATED, class F>
__device__ inline int seed_walk(const SeedGrid& g, const SeedViews& s, const SeedGate& gate, long long id, F&& f) {
#pragma clang fp contract(off)
    double X, Y, Z;
    seed_centre(g, id, X, Y, Z);
    const double wd = (double)s.width, hd = (double)s.height;
    const size_t plane = (size_t)s.height * (size_t)s.stride;
    const size_t image = (size_t)s.height * (size_t)s.width;
    int n_hidden = 0;
    for (int v = 0; v < s.V; v++) {   // v is uniform: scalar loads of the camera
        NvCam c;
        nv_load_cam(c, s.intr, s.w2c, v);
        unsigned int px, py;
        bool near, hid = false;
        const float* __restrict__ dplane = GATED ? gate.depth + (size_t)v * image : nullptr;
        if (seed_pixel<GATED>(c, X, Y, Z, wd, hd, s.bits + (size_t)v * plane, s.stride, dplane, s.width, gate.slack, px, py, near,
                              hid))
            f(v, px, py, near);
        if (GATED) n_hidden += (int)hid;
    }
    return n_hidden;
}

template <bool GATED>
__global__ void __launch_bounds__(SEED_THREADS) k_voxel_votes(const SeedGrid g, const SeedViews s, int accumulate,
                                                             unsigned short* __restrict__ seen,
                                                             unsigned short* __restrict__ hit, const SeedGate gate,
                                                             unsigned short* __restrict__ hidden) {
    const long long n = (long long)g.nx * g.ny * g.nz;   // <= 2^31 - 1
    const long long id = (long long)blockIdx.x * SEED_THREADS + threadIdx.x;
    if (id >= n) return;
    int n_seen = 0, n_hit = 0;
    int n_hidden = seed_walk<GATED>(g, s, gate, id, [&](int, unsigned int, unsigned int, bool near) {
        n_seen++;
        n_hit += (int)near;
    });
    if (accumulate) {
        n_seen += seen[id];
        n_hit += hit[id];
    }
    seen[id] = (unsigned short)n_seen;
    hit[id] = (unsigned short)n_hit;
    if (GATED && hidden) {   // the third count, under the same rule
        if (accumulate) n_hidden += hidden[id];
        hidden[id] = (unsigned short)n_hidden;
    }
}

__global__ void __launch_bounds__(SEED_THREADS) k_voxel_moments(int nx, int ny, int nz, int stride,
                                                               const unsigned int* __restrict__ keep, int N,
                                                               const int* __restrict__ centres, int radius,
                                                               int* __restrict__ moments) {
    const int lane = threadIdx.x & 63;
    const long long seed = (long long)blockIdx.x * MOMENT_WAVES + (threadIdx.x >> 6);
    if (seed >= N) return;   // wave-uniform; the kernel has no barrier
    const int cx = centres[3 * seed], cy = centres[3 * seed + 1], cz = centres[3 * seed + 2];
    const int side = 2 * radius + 1, r2 = radius * radius;
    int acc[MOMENT_VALUES];
#pragma unroll
    for (int k = 0; k < MOMENT_VALUES; k++) acc[k] = 0;
    // a centre outside the grid (the caller's error) reads nothing and gives a zero row
    const bool inside = cx >= 0 && cx < nx && cy >= 0 && cy < ny && cz >= 0 && cz < nz;
    for (int row = lane; inside && row < side * side; row += 64) {
        const int dz = row / side - radius, dy = row % side - radius;
        const int y = cy + dy, z = cz + dz;
        const int rem = r2 - dy * dy - dz * dz;
        if (y < 0 || y >= ny || z < 0 || z >= nz || rem < 0) continue;
        int h = 0;   // isqrt(rem), at most 15
        while ((h + 1) * (h + 1) <= rem) h++;
        const int x0 = max(cx - h, 0), x1 = min(cx + h, nx - 1);   // x0 <= cx <= x1, x1 - x0 <= 30
        const unsigned int* line = keep + ((size_t)z * (size_t)ny + (size_t)y) * (size_t)stride;
        const int w0 = x0 >> 5, w1 = x1 >> 5;                      // w1 - w0 <= 1, w1 < stride
        unsigned long long span = line[w0];
        if (w1 != w0) span |= (unsigned long long)line[w1] << 32;
        // bit b of `bitsx` = voxel x0 + b; (x0 & 31) + (x1 - x0 + 1) <= 62 bits of `span` are in use
        unsigned int bitsx = (unsigned int)(span >> (x0 & 31)) & ((1u << (x1 - x0 + 1)) - 1u);
        while (bitsx) {
            const int dx = x0 + (__ffs(bitsx) - 1) - cx;
            bitsx &= bitsx - 1u;
            acc[0] += 1;
            acc[1] += dx; acc[2] += dy; acc[3] += dz;
            acc[4] += dx * dx; acc[5] += dy * dy; acc[6] += dz * dz;
            acc[7] += dx * dy; acc[8] += dx * dz; acc[9] += dy * dz;
        }
    }
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int k = 0; k < MOMENT_VALUES; k++) acc[k] += __shfl_xor(acc[k], off, 64);
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < MOMENT_VALUES; k++) moments[(size_t)seed * MOMENT_VALUES + k] = acc[k];
    }
}

template <bool GATED>
__global__ void __launch_bounds__(SEED_THREADS) k_ray_claims(const SeedGrid g, const SeedViews s, int M,
                                                            const int* __restrict__ index,
                                                            const unsigned short* __restrict__ support,
                                                            unsigned int* __restrict__ best, const SeedGate gate) {
    const long long n = (long long)g.nx * g.ny * g.nz;   // <= 2^31 - 1
    const long long m = (long long)blockIdx.x * SEED_THREADS + threadIdx.x;
    if (m >= M) return;
    const long long id = index[m];
    if (id < 0 || id >= n) return;   // the caller's error: claims nothing
    const unsigned int sup = support[m];
    const size_t image = (size_t)s.height * (size_t)s.width;
    seed_walk<GATED>(g, s, gate, id, [&](int v, unsigned int px, unsigned int py, bool near) {
        if (!near) return;
        unsigned int* p = best + (size_t)v * image + (size_t)py * (size_t)s.width + (size_t)px;
        // no look before the atomic: a plain load that skips it where best already holds as much measured slower
        // (profiles/edge_seed_exclusive.md)
        atomicMax(p, sup);
    });
}

template <bool GATED>
__global__ void __launch_bounds__(SEED_THREADS) k_ray_wins(const SeedGrid g, const SeedViews s, int M,
                                                          const int* __restrict__ index,
                                                          const unsigned short* __restrict__ support,
                                                          const unsigned int* __restrict__ best, int window, int margin,
                                                          int accumulate, unsigned short* __restrict__ wins,
                                                          const SeedGate gate) {
    const long long n = (long long)g.nx * g.ny * g.nz;   // <= 2^31 - 1
    const long long m = (long long)blockIdx.x * SEED_THREADS + threadIdx.x;
    if (m >= M) return;
    const long long id = index[m];
    int n_wins = 0;
    if (id >= 0 && id < n) {   // an index outside the grid is the caller's error: it wins nothing
        const unsigned int sup = (unsigned int)support[m] + (unsigned int)margin;   // <= 131070: 32 bits do not wrap
        const size_t image = (size_t)s.height * (size_t)s.width;
        seed_walk<GATED>(g, s, gate, id, [&](int v, unsigned int px, unsigned int py, bool near) {
            if (!near) return;
            const int x0 = max((int)px - window, 0), x1 = min((int)px + window, s.width - 1);
            const int y0 = max((int)py - window, 0), y1 = min((int)py + window, s.height - 1);
            const unsigned int* view = best + (size_t)v * image;
            unsigned int top = 0;
            for (int y = y0; y <= y1; y++)
                for (int x = x0; x <= x1; x++) top = max(top, view[(size_t)y * (size_t)s.width + (size_t)x]);
            n_wins += (int)(sup >= top);
        });
    }
    if (accumulate) n_wins += wins[m];
    wins[m] = (unsigned short)n_wins;
}

void launch_pack_near_bits(hipStream_t s, int V, int height, int width, const int* dist2, int tol2, unsigned int* bits) {
    const int stride = (width + 31) / 32;
    const long long padded = (long long)height * stride * 32;
    const unsigned blocks = (unsigned)((padded + SEED_THREADS - 1) / SEED_THREADS);   // <= 2^28 / 256 + 1
    const size_t plane = (size_t)height * (size_t)width;
    ProfScope p("pack_near_bits", s);
    for (int v0 = 0; v0 < V; v0 += SEED_MAX_VIEWS) {
        const int nv = std::min(SEED_MAX_VIEWS, V - v0);
        hipLaunchKernelGGL(k_pack_near_bits, dim3(blocks, nv), dim3(SEED_THREADS), 0, s, height, width, stride,
                           dist2 + (size_t)v0 * plane, tol2, bits + (size_t)v0 * (size_t)height * (size_t)stride);
    }
}

template <bool GATED>
static void voxel_votes_launch(hipStream_t s, SeedGrid g, SeedViews views, DepthGate gate, int accumulate, unsigned short* seen,
                               unsigned short* hit, unsigned short* hidden) {
    const long long n = (long long)g.nx * g.ny * g.nz;
    const unsigned blocks = (unsigned)((n + SEED_THREADS - 1) / SEED_THREADS);   // <= 2^23
    ProfScope p(GATED ? "voxel_votes_depth" : "voxel_votes", s);
    hipLaunchKernelGGL(k_voxel_votes<GATED>, dim3(blocks), dim3(SEED_THREADS), 0, s, g, views, accumulate, seen, hit, gate,
                       hidden);
}

void launch_voxel_votes(hipStream_t s, SeedGrid g, SeedViews views, const DepthGate* gate, int accumulate,
                        unsigned short* seen, unsigned short* hit, unsigned short* hidden) {
    if (gate) voxel_votes_launch<true>(s, g, views, *gate, accumulate, seen, hit, hidden);
    else voxel_votes_launch<false>(s, g, views, DepthGate{nullptr, 0.0}, accumulate, seen, hit, nullptr);
}

void launch_voxel_moments(hipStream_t s, int nx, int ny, int nz, const unsigned int* keep, int N, const int* centres,
                          int radius, int* moments) {
    const unsigned blocks = (unsigned)(((long long)N + MOMENT_WAVES - 1) / MOMENT_WAVES);
    ProfScope p("voxel_moments", s);
    hipLaunchKernelGGL(k_voxel_moments, dim3(blocks), dim3(SEED_THREADS), 0, s, nx, ny, nz, (nx + 31) / 32, keep, N, centres,
                       radius, moments);
}

template <bool GATED>
static hipError_t ray_claims_launch(hipStream_t s, SeedGrid g, SeedViews views, DepthGate gate, int M, const int* index,
                                    const unsigned short* support, int clear, unsigned int* best) {
    if (clear && views.V > 0) {
        const size_t bytes = (size_t)views.V * (size_t)views.height * (size_t)views.width * sizeof(unsigned int);
        const hipError_t e = hipMemsetAsync(best, 0, bytes, s);
        if (e != hipSuccess) return e;
    }
    if (M == 0 || views.V == 0) return hipSuccess;
    const unsigned blocks = (unsigned)(((long long)M + SEED_THREADS - 1) / SEED_THREADS);   // <= 2^23
    ProfScope p(GATED ? "ray_claims_depth" : "ray_claims", s);
    hipLaunchKernelGGL(k_ray_claims<GATED>, dim3(blocks), dim3(SEED_THREADS), 0, s, g, views, M, index, support, best, gate);
    return hipSuccess;
}

hipError_t launch_ray_claims(hipStream_t s, SeedGrid g, SeedViews views, const DepthGate* gate, int M, const int* index,
                             const unsigned short* support, int clear, unsigned int* best) {
    return gate ? ray_claims_launch<true>(s, g, views, *gate, M, index, support, clear, best)
                : ray_claims_launch<false>(s, g, views, DepthGate{nullptr, 0.0}, M, index, support, clear, best);
}

template <bool GATED>
static void ray_wins_launch(hipStream_t s, SeedGrid g, SeedViews views, DepthGate gate, int M, const int* index,
                            const unsigned short* support, const unsigned int* best, int window, int margin, int accumulate,
                            unsigned short* wins) {
    const unsigned blocks = (unsigned)(((long long)M + SEED_THREADS - 1) / SEED_THREADS);   // <= 2^23
    ProfScope p(GATED ? "ray_wins_depth" : "ray_wins", s);
    hipLaunchKernelGGL(k_ray_wins<GATED>, dim3(blocks), dim3(SEED_THREADS), 0, s, g, views, M, index, support, best, window,
                       margin, accumulate, wins, gate);
}

void launch_ray_wins(hipStream_t s, SeedGrid g, SeedViews views, const DepthGate* gate, int M, const int* index,
                     const unsigned short* support, const unsigned int* best, int window, int margin, int accumulate,
                     unsigned short* wins) {
    if (gate)
        ray_wins_launch<true>(s, g, views, *gate, M, index, support, best, window, margin, accumulate, wins);
    else
        ray_wins_launch<false>(s, g, views, DepthGate{nullptr, 0.0}, M, index, support, best, window, margin, accumulate,
                               wins);
}

}  // namespace cgs
