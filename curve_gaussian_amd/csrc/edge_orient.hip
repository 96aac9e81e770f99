// Orientation-aware 2D support (include/curvegs.h: cgs_mask_orientation, cgs_oriented_near, cgs_sample_support_oriented): an
// orientation code for every detected pixel, the codes gathered over the tolerance disk, and the per-sample tally of
// edge_trim.hip with the direction of the sample's edge held against them.  The rule is frozen in the header; integers
// (and, for the tally, float64 without contraction) only, so the numpy back end of ops/edge_orient.py agrees bit for bit.
//   k_mask_orientation   one workgroup of 256 threads per tile of ORIENT_TW x ORIENT_TH = 64 x 32 pixels of a view.  The
//                        tile and its halo of ORIENT_R = 3 pixels are staged in LDS once, as bytes 0 / 1 (0 outside the
//                        image).  The six window sums are separable: a first pass forms, per staged row and tile column, the
//                        row's N, Sx and Sxx over dx in [-3, 3] and packs them into one word (N <= 7, |Sx| <= 6, Sxx <= 28);
//                        after one barrier a thread sums seven words of its column per pixel -- N, Sx, Sxx directly, Sy, Syy
//                        and Sxy with the row's dy -- 14 LDS reads per pixel where the plain window takes 49.  A lane owns
//                        one column, a wave every fourth row: a wave's store is 64 consecutive bytes.  Every output byte
//                        of the tile is written; no atomics.
//   k_oriented_near      the same tile; the halo is ORIENT_MAX_R = 4 -- one word -- whatever the tolerance, and the disk
//                        arrives as the half width of each of its nine rows (-1: the row is not part of the disk), formed
//                        on the host from tol2: the kernel knows no square root.  A thread owns four pixels of a row, one
//                        word: per disk row it reads the three words around them and a tap is a 64-bit shift and an OR
//                        for all four pixels, where a byte per pixel and tap took ten times as long at 49 taps.  The word
//                        is stored whole where the plane's rows are word-aligned, byte by byte otherwise.
//   k_sample_support_oriented   the shape of k_sample_support (edge_trim.hip): one thread per sample, the view loop inside,
//                        so the 16 doubles of a camera are wave-uniform loads.  The sample's and its partner's points are
//                        read once before the loop; both are projected with nv_project_xyz in every view.  Two sums in
//                        registers, one read-modify-write of the thread's own row: no atomics, no LDS, no barrier.
//                        A template over GATED: false is cgs_sample_support_oriented as it always was; true is
//                        cgs_sample_support_oriented_depth -- nv_verdict (point_projection.h) gates the SAMPLE; the partner
//                        gives a direction only and is projected with nv_project_xyz, never held against the depth.
// Nothing here depends on the launch geometry: one owner per output byte or row, integer sums, no order of arrival.
#include <algorithm>

#include "kernels.h"
#include "point_projection.h"

namespace cgs {

constexpr int ORIENT_R = CGS_ORIENT_RADIUS;
constexpr int ORIENT_MAX_R = 4;   // isqrt(CGS_ORIENT_MAX_TOL2)
constexpr int ORIENT_TW = CGS_ORIENT_TILE_WIDTH;
constexpr int ORIENT_TH = CGS_ORIENT_TILE_HEIGHT;
constexpr int ORIENT_THREADS = 256;
constexpr int ORIENT_MAX_VIEWS = 65535;   // views per launch: grid.z
constexpr int ORIENT_PITCH = ORIENT_TW + 2 * ORIENT_MAX_R;   // bytes per staged row, both kernels
static_assert(ORIENT_R == 3, "the packed row sums below are sized for a window of 7");
static_assert(ORIENT_MAX_R * ORIENT_MAX_R == CGS_ORIENT_MAX_TOL2, "the halo of k_oriented_near");
static_assert(ORIENT_TW == 64 && ORIENT_THREADS % 64 == 0 && ORIENT_TH % (ORIENT_THREADS / 64) == 0,
              "a lane owns a column, a wave every (ORIENT_THREADS / 64)-th row");

// The half-open octant of the doubled angle of (a, b) != (0, 0), by signs and one comparison of magnitudes (the table of
// the header).  T is int for the moments of a window and double for the step between two projected samples.
template <typename T>
__device__ __forceinline__ int orient_octant(T a, T b) {
    const T ma = a < 0 ? -a : a, mb = b < 0 ? -b : b;
    if (a > 0 && b >= 0) return mb < ma ? 0 : 1;
    if (a <= 0 && b > 0) return mb > ma ? 2 : 3;
    if (a < 0 && b <= 0) return mb < ma ? 4 : 5;
    return mb > ma ? 6 : 7;   // a >= 0, b < 0
}

// Stages rows [y0 - halo, y0 + TH + halo) x columns [x0 - halo, x0 + TW + halo) of a view's plane; `set` maps a byte
template <int HALO, typename F>
__device__ __forceinline__ void orient_stage(uint8_t (*tile)[ORIENT_PITCH], const uint8_t* __restrict__ src, int height,
                                             int width, int x0, int y0, F set) {
    constexpr int RW = ORIENT_TW + 2 * HALO, RH = ORIENT_TH + 2 * HALO;
    for (int k = threadIdx.x; k < RW * RH; k += ORIENT_THREADS) {
        const int r = k / RW, c = k - r * RW;
        const int y = y0 - HALO + r, x = x0 - HALO + c;
        uint8_t b = 0;
        if (y >= 0 && y < height && x >= 0 && x < width) b = set(src[(size_t)y * (size_t)width + (size_t)x]);
        tile[r][c] = b;
    }
}

__global__ void __launch_bounds__(ORIENT_THREADS) k_mask_orientation(int height, int width,
                                                                     const uint8_t* __restrict__ mask,
                                                                     uint8_t* __restrict__ code) {
    constexpr int R = ORIENT_R, RH = ORIENT_TH + 2 * R;
    __shared__ uint8_t m[RH][ORIENT_PITCH];      // the staged pixels, 0 / 1
    __shared__ uint32_t rs[RH][ORIENT_TW];       // per staged row and tile column: N | (Sx + 6) << 8 | Sxx << 16
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x0 = (int)blockIdx.x * ORIENT_TW, y0 = (int)blockIdx.y * ORIENT_TH;
    const size_t plane = (size_t)height * (size_t)width;
    orient_stage<R>(m, mask + (size_t)blockIdx.z * plane, height, width, x0, y0,
                    [](uint8_t b) { return (uint8_t)(b != 0); });
    __syncthreads();
    for (int r = wave; r < RH; r += ORIENT_THREADS / 64) {
        int n = 0, sx = 0, sxx = 0;
#pragma unroll
        for (int dx = -R; dx <= R; dx++) {
            const int b = m[r][lane + R + dx];
            n += b;
            sx += dx * b;
            sxx += dx * dx * b;
        }
        rs[r][lane] = (uint32_t)n | (uint32_t)(sx + 6) << 8 | (uint32_t)sxx << 16;
    }
    __syncthreads();
    const int x = x0 + lane;
    uint8_t* __restrict__ dst = code + (size_t)blockIdx.z * plane;
    for (int ty = wave; ty < ORIENT_TH; ty += ORIENT_THREADS / 64) {
        const int y = y0 + ty;   // wave-uniform
        if (y >= height || x >= width) continue;   // no barrier below
        uint8_t out = 0;
        if (m[ty + R][lane + R]) {
            int N = 0, Sx = 0, Sy = 0, Sxx = 0, Syy = 0, Sxy = 0;
#pragma unroll
            for (int dy = -R; dy <= R; dy++) {
                const uint32_t w = rs[ty + R + dy][lane];
                const int n = (int)(w & 0xFFu), sx = (int)((w >> 8) & 0xFFu) - 6, sxx = (int)(w >> 16);
                N += n;
                Sx += sx;
                Sxx += sxx;
                Sy += dy * n;
                Syy += dy * dy * n;
                Sxy += dy * sx;
            }
            // 32 bits hold everything: N <= 49 and Sxx, Syy <= 196, so 0 <= A, C and A + C <= 49 * 392 = 19208;
            // B^2 <= A C (Cauchy-Schwarz), so a^2 + b^2 = (A - C)^2 + 4 B^2 <= (A + C)^2 and 4 * 19208^2 < 2^31
            const int A = N * Sxx - Sx * Sx, B = N * Sxy - Sx * Sy, C = N * Syy - Sy * Sy;
            const int a = A - C, b = 2 * B;
            const bool oriented = N >= 3 && (a != 0 || b != 0) && 4 * (a * a + b * b) >= (A + C) * (A + C);
            out = oriented ? (uint8_t)(1u << orient_octant(a, b)) : (uint8_t)0xFF;
        }
        dst[(size_t)y * (size_t)width + (size_t)x] = out;
    }
}

struct OrientDisk {   // the half width of row dy = k - ORIENT_MAX_R of the disk dx^2 + dy^2 <= tol2; -1: no pixel; by value
    int half[2 * ORIENT_MAX_R + 1];
};

__global__ void __launch_bounds__(ORIENT_THREADS) k_oriented_near(int height, int width, const uint8_t* __restrict__ code,
                                                                  OrientDisk disk, uint8_t* __restrict__ near) {
    constexpr int R = ORIENT_MAX_R, RH = ORIENT_TH + 2 * R, WORDS = ORIENT_PITCH / 4, GROUPS = ORIENT_TW / 4;
    static_assert(R == 4 && ORIENT_PITCH % 4 == 0, "the halo is one word: pixel group g of the tile is staged word g + 1");
    __shared__ uint32_t mw[RH][WORDS];   // the staged codes, four pixels per word (byte j = pixel j); written as bytes
    const int x0 = (int)blockIdx.x * ORIENT_TW, y0 = (int)blockIdx.y * ORIENT_TH;
    const size_t plane = (size_t)height * (size_t)width;
    orient_stage<R>(reinterpret_cast<uint8_t(*)[ORIENT_PITCH]>(mw), code + (size_t)blockIdx.z * plane, height, width, x0, y0,
                    [](uint8_t b) { return b; });
    __syncthreads();
    // A thread owns four pixels in a row: a tap is one 64-bit shift of the three words around them where it would be four
    // byte reads.  Group g = threadIdx.x % 16 of the row, every (ORIENT_THREADS / 16)-th row.
    const int g = threadIdx.x % GROUPS, x = x0 + 4 * g;
    uint8_t* __restrict__ dst = near + (size_t)blockIdx.z * plane;
    const bool words = (width & 3) == 0 && (reinterpret_cast<uintptr_t>(near) & 3) == 0;   // then every group is aligned
    for (int ty = threadIdx.x / GROUPS; ty < ORIENT_TH; ty += ORIENT_THREADS / GROUPS) {
        const int y = y0 + ty;
        if (y >= height || x >= width) continue;   // no barrier below
        uint32_t acc = 0;
#pragma unroll 1
        for (int k = 0; k <= 2 * R; k++) {   // kept a loop: unrolled, its nine inner loops spilled 22 SGPRs
            const int h = disk.half[k];      // uniform; at most R = 4, one word to either side
            if (h < 0) continue;
            const uint32_t w0 = mw[ty + k][g], w1 = mw[ty + k][g + 1], w2 = mw[ty + k][g + 2];
            const uint64_t lo = (uint64_t)w0 | (uint64_t)w1 << 32;   // pixels x - 4 .. x + 3
            const uint64_t hi = (uint64_t)w1 | (uint64_t)w2 << 32;   // pixels x .. x + 7
            acc |= w1;
            for (int dx = 1; dx <= h; dx++) acc |= (uint32_t)(hi >> (8 * dx)) | (uint32_t)(lo >> (8 * (4 - dx)));
        }
        uint8_t* __restrict__ p = dst + (size_t)y * (size_t)width + (size_t)x;
        if (words) {   // width % 4 == 0: the group lies inside the row
            *reinterpret_cast<uint32_t*>(p) = acc;
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (x + j < width) p[j] = (uint8_t)(acc >> (8 * j));
        }
    }
}

static dim3 orient_grid(int height, int width, int views) {
    return dim3((unsigned)((width + ORIENT_TW - 1) / ORIENT_TW), (unsigned)((height + ORIENT_TH - 1) / ORIENT_TH),
                (unsigned)views);
}

void launch_mask_orientation(hipStream_t s, int V, int height, int width, const uint8_t* mask, uint8_t* code) {
    const size_t plane = (size_t)height * (size_t)width;
    ProfScope p("mask_orientation", s);
    for (int v0 = 0; v0 < V; v0 += ORIENT_MAX_VIEWS) {
        const int nv = std::min(ORIENT_MAX_VIEWS, V - v0);
        hipLaunchKernelGGL(k_mask_orientation, orient_grid(height, width, nv), dim3(ORIENT_THREADS), 0, s, height, width,
                           mask + (size_t)v0 * plane, code + (size_t)v0 * plane);
    }
}

void launch_oriented_near(hipStream_t s, int V, int height, int width, const uint8_t* code, int tol2, uint8_t* near) {
    OrientDisk disk;
    for (int k = 0; k <= 2 * ORIENT_MAX_R; k++) {
        const int dy = k - ORIENT_MAX_R, rest = tol2 - dy * dy;
        int h = -1;
        while (h + 1 <= ORIENT_MAX_R && (h + 1) * (h + 1) <= rest) h++;   // the largest h with h^2 <= rest; -1 when rest < 0
        disk.half[k] = h;
    }
    const size_t plane = (size_t)height * (size_t)width;
    ProfScope p("oriented_near", s);
    for (int v0 = 0; v0 < V; v0 += ORIENT_MAX_VIEWS) {
        const int nv = std::min(ORIENT_MAX_VIEWS, V - v0);
        hipLaunchKernelGGL(k_oriented_near, orient_grid(height, width, nv), dim3(ORIENT_THREADS), 0, s, height, width,
                           code + (size_t)v0 * plane, disk, near + (size_t)v0 * plane);
    }
}

constexpr int ORIENT_TALLY_THREADS = 256;

template <bool GATED>
__global__ void __launch_bounds__(ORIENT_TALLY_THREADS)
k_sample_support_oriented(int P, const float* __restrict__ pts, const int* __restrict__ partner, int V,
                          const double* __restrict__ intr, const double* __restrict__ w2c, int height, int width,
                          const uint8_t* __restrict__ near, int spread, int* __restrict__ tally,
                          const float* __restrict__ depth, double slack, int* __restrict__ hidden) {
    const long long i = (long long)blockIdx.x * ORIENT_TALLY_THREADS + threadIdx.x;
    if (i >= P) return;   // the kernel has no barrier
    const double X = (double)pts[3 * i + 0], Y = (double)pts[3 * i + 1], Z = (double)pts[3 * i + 2];
    const long long j = (long long)partner[i];
    const bool paired = j != i && j >= 0 && j < P;   // anything else is "no partner": nothing is read out of bounds
    const long long jj = paired ? j : i;
    const double Xp = (double)pts[3 * jj + 0], Yp = (double)pts[3 * jj + 1], Zp = (double)pts[3 * jj + 2];
    // the bits (o - spread) .. (o + spread) mod 8 are `band` rotated left by (o - spread) mod 8 within a byte
    const unsigned band = spread >= 4 ? 0xFFu : (1u << (2 * spread + 1)) - 1u;
    const double wd = (double)width, hd = (double)height;
    const size_t plane = (size_t)height * (size_t)width;
    int seen = 0, hit = 0, hid = 0;
    for (int view = 0; view < V; view++) {   // wave-uniform
        NvCam c;
        nv_load_cam(c, intr, w2c, view);
        double u, v, up, vp;
        const NvVerdict verdict = nv_verdict<GATED>(c, X, Y, Z, wd, hd, GATED ? depth + (size_t)view * plane : nullptr, width,
                                                    slack, u, v);
        if (verdict == NV_OUT) continue;
        if (GATED && verdict == NV_HIDDEN) {
            hid++;
            continue;
        }
        seen++;
        unsigned acc = 0xFFu;
        if (paired && nv_project_xyz(c, Xp, Yp, Zp, wd, hd, up, vp)) {
#pragma clang fp contract(off)
            const double dx = up - u, dy = vp - v;
            const double xx = dx * dx, yy = dy * dy, xy = dx * dy;
            const double a = xx - yy, b = 2.0 * xy;
            if (a != 0.0 || b != 0.0) {
                const int sh = (orient_octant(a, b) - spread) & 7;
                acc = ((band << sh) | (band >> (8 - sh))) & 0xFFu;
            }
        }
        // 0 <= u < W, so 0 <= floor(u) <= W - 1 (likewise v): the pixel is inside the view's plane
        const unsigned n = near[(size_t)view * plane + (size_t)floor(v) * (size_t)width + (size_t)floor(u)];
        hit += (n & acc) != 0u ? 1 : 0;
    }
    int* __restrict__ out = tally + 2 * (size_t)i;   // the thread's own row: a plain read-modify-write
    out[0] += seen;
    out[1] += hit;
    if (GATED && hidden) hidden[i] += hid;   // added, like the tally: the thread's own word
}

template <bool GATED>
static void sample_support_oriented_launch(hipStream_t s, int P, const float* points, const int* partner, int V,
                                           const double* intr, const double* w2c, int height, int width, const uint8_t* near,
                                           int spread, int* tally, DepthGate gate, int* hidden) {
    const unsigned blocks = (unsigned)(((long long)P + ORIENT_TALLY_THREADS - 1) / ORIENT_TALLY_THREADS);   // at most 2^23
    ProfScope p(GATED ? "sample_support_oriented_depth" : "sample_support_oriented", s);
    hipLaunchKernelGGL(k_sample_support_oriented<GATED>, dim3(blocks), dim3(ORIENT_TALLY_THREADS), 0, s, P, points, partner, V,
                       intr, w2c, height, width, near, spread, tally, gate.depth, gate.slack, hidden);
}

void launch_sample_support_oriented(hipStream_t s, int P, const float* points, const int* partner, int V, const double* intr,
                                    const double* w2c, int height, int width, const uint8_t* near, int spread,
                                    const DepthGate* gate, int* tally, int* hidden) {
    if (gate)
        sample_support_oriented_launch<true>(s, P, points, partner, V, intr, w2c, height, width, near, spread, tally, *gate,
                                             hidden);
    else
        sample_support_oriented_launch<false>(s, P, points, partner, V, intr, w2c, height, width, near, spread, tally,
                                              DepthGate{nullptr, 0.0}, nullptr);
}

}  // namespace cgs
