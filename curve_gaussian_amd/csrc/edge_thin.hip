// Parallel binary thinning of detected edge masks (include/curvegs.h, cgs_thin_masks): Guo-Hall two-subiteration thinning,
// THIN_K iterations per launch on a tile held bit-packed in LDS.
//   k_thin_pass   one workgroup of THIN_RH threads per tile.  The workgroup's REGION is THIN_RW = 64 columns by THIN_RH = 256
//                 rows: the tile (THIN_TW x THIN_TH = 48 x 240) and a halo of 2 THIN_K = 8 pixels on every side, 0 outside
//                 the image.  A row of the region is ONE 64-bit word (bit b = column b) and belongs to one thread.
//                 Load: a wave reads a row as 64 consecutive bytes, one per lane, and __ballot(byte != 0) IS the row's word
//                 (this also normalises non-0/1 bytes); the loads are unconditional at clamped addresses, eight rows in
//                 flight, and masked afterwards.  A sub-iteration: the thread reads the rows above and below from
//                 LDS (8 bytes per lane, consecutive: no bank conflict), forms the eight neighbour planes by shifts
//                 (P4 = w >> 1, P8 = w << 1, ...) and evaluates the rule for 64 pixels at once with bit-sliced sums; the
//                 state is double-buffered in LDS, so a sub-iteration costs one barrier.  A sub-iteration reads radius 1, so
//                 after s sub-iterations only the pixels within s of the region's rim can be wrong: the tile, 2 THIN_K
//                 from the rim, is exact after every one of the 2 THIN_K sub-iterations.  Where the rim lies on or outside
//                 the image's border the zeros are the true values.  Only the tile is stored (bytes 0/1, to the other
//                 buffer).  A region in which an iteration changed nothing is at a fixed point: the workgroup stops there.
//                 The flag: every thread remembers the last iteration (1-based, of this launch) in which a TILE pixel of its
//                 row changed; a shuffle maximum per wave and one integer atomicMax per wave that saw a change.  A maximum
//                 does not depend on the order, so the flag -- and the iteration count the host derives from it -- is
//                 deterministic.  The flag carries the iteration and not a plain 1 because the caller is told the exact
//                 number of iterations, and because a last change before the launch's last iteration proves that the state
//                 has settled: the confirming launch is saved.
// Integers and booleans only: the result cannot depend on THIN_K, the tile or the launch geometry.
#include <algorithm>

#include "kernels.h"

namespace cgs {

constexpr int THIN_K = CGS_THIN_PASS_ITERATIONS;
constexpr int THIN_HALO = 2 * THIN_K;
constexpr int THIN_RW = 64;    // region width: the bits of one word
constexpr int THIN_RH = 256;   // region height: one thread per row
constexpr int THIN_TW = THIN_RW - 2 * THIN_HALO;
constexpr int THIN_TH = THIN_RH - 2 * THIN_HALO;
constexpr int THIN_THREADS = THIN_RH;
constexpr int THIN_MAX_VIEWS = 65535;   // views per launch: grid.z
constexpr int THIN_LOAD_ROWS = 8;       // rows a wave has in flight while it loads its 64
static_assert(THIN_TW == CGS_THIN_TILE_WIDTH && THIN_TH == CGS_THIN_TILE_HEIGHT, "the header states the tile");
static_assert(THIN_TW > 0 && THIN_RH % 64 == 0, "a wave loads and stores 64 whole rows");

typedef unsigned long long thin_word;

// The number of set bits among a, b, c, d in every bit position, as three planes: n = ones + 2 twos + 4 fours
__device__ __forceinline__ void thin_count4(thin_word a, thin_word b, thin_word c, thin_word d, thin_word& ones,
                                            thin_word& twos, thin_word& fours) {
    const thin_word s1 = a ^ b, c1 = a & b, s2 = c ^ d, c2 = c & d;
    ones = s1 ^ s2;
    twos = c1 ^ c2 ^ (s1 & s2);
    fours = c1 & c2;
}

// One sub-iteration for the 64 pixels of row `mid`, `up` and `down` being the rows y - 1 and y + 1
__device__ __forceinline__ thin_word thin_sub(thin_word up, thin_word mid, thin_word down, int sub) {
    const thin_word P2 = up, P3 = up >> 1, P9 = up << 1, P4 = mid >> 1, P8 = mid << 1, P6 = down, P5 = down >> 1,
                    P7 = down << 1;
    thin_word ones, twos, fours;
    thin_count4(~P2 & (P3 | P4), ~P4 & (P5 | P6), ~P6 & (P7 | P8), ~P8 & (P9 | P2), ones, twos, fours);
    const thin_word c_is_1 = ones & ~twos;   // 1 or 3 have the ones bit; 3 has the twos bit too
    thin_word twos1, fours1, twos2, fours2;
    thin_count4(P9 | P2, P3 | P4, P5 | P6, P7 | P8, ones, twos1, fours1);
    thin_count4(P2 | P3, P4 | P5, P6 | P7, P8 | P9, ones, twos2, fours2);
    // 2 <= min(N1, N2) <= 3: both are at least 2 and not both are 4
    const thin_word n_ok = (twos1 | fours1) & (twos2 | fours2) & ~(fours1 & fours2);
    const thin_word m = sub == 0 ? (P6 | P7 | ~P9) & P8 : (P2 | P3 | ~P5) & P4;
    return mid & ~(c_is_1 & n_ok & ~m);
}

__global__ void __launch_bounds__(THIN_THREADS) k_thin_pass(int height, int width, const uint8_t* __restrict__ in,
                                                            uint8_t* __restrict__ out, int iterations,
                                                            int* __restrict__ changed_flag) {
    __shared__ thin_word rows[2][THIN_RH + 2];   // [buffer][1 + region row]; entries 0 and THIN_RH + 1 stay 0
    const int t = threadIdx.x, lane = t & 63;
    const int wave_row0 = __builtin_amdgcn_readfirstlane(t & ~63);   // the wave's first region row
    const int x0 = (int)blockIdx.x * THIN_TW - THIN_HALO, y0 = (int)blockIdx.y * THIN_TH - THIN_HALO;
    const size_t plane = (size_t)height * (size_t)width;
    const uint8_t* __restrict__ src = in + (size_t)blockIdx.z * plane;
    uint8_t* __restrict__ dst = out + (size_t)blockIdx.z * plane;
    const int x = x0 + lane;
    const bool x_in = x >= 0 && x < width;

    // Eight rows' loads are issued before the first is used: every load is unconditional, at an address clamped into
    // the view, and what it returned is discarded where the pixel lies outside the image
    const size_t xc = (size_t)min(max(x, 0), width - 1);
    thin_word cur = 0;
    for (int r0 = 0; r0 < 64; r0 += THIN_LOAD_ROWS) {
        uint8_t b[THIN_LOAD_ROWS];
#pragma unroll
        for (int j = 0; j < THIN_LOAD_ROWS; j++) {
            const int y = y0 + wave_row0 + r0 + j;   // wave-uniform
            b[j] = src[(size_t)min(max(y, 0), height - 1) * (size_t)width + xc];
        }
#pragma unroll
        for (int j = 0; j < THIN_LOAD_ROWS; j++) {
            const int y = y0 + wave_row0 + r0 + j;
            const thin_word w = __ballot(x_in && y >= 0 && y < height && b[j] != 0);
            if (lane == r0 + j) cur = w;
        }
    }
    if (t == 0) rows[0][0] = rows[1][0] = rows[0][THIN_RH + 1] = rows[1][THIN_RH + 1] = 0;
    rows[0][t + 1] = cur;
    __syncthreads();

    const bool tile_row = t >= THIN_HALO && t < THIN_RH - THIN_HALO;
    constexpr thin_word TILE_COLUMNS = ((1ull << THIN_TW) - 1) << THIN_HALO;
    int last = 0;   // the last iteration in which a tile pixel of this row changed
    for (int it = 1; it <= iterations; it++) {
        const thin_word before = cur;
        cur = thin_sub(rows[0][t], cur, rows[0][t + 2], 0);
        rows[1][t + 1] = cur;
        __syncthreads();
        cur = thin_sub(rows[1][t], cur, rows[1][t + 2], 1);
        rows[0][t + 1] = cur;   // every read of rows[0] lies before the barrier above
        const thin_word diff = cur ^ before;   // pixels are only ever cleared: no change means none in either half
        if (tile_row && (diff & TILE_COLUMNS)) last = it;
        if (!__syncthreads_or(diff != 0)) break;   // the region is at a fixed point
    }

    for (int r = 0; r < 64; r++) {
        const int row = wave_row0 + r, y = y0 + row;   // wave-uniform; a tile row has y >= 0, a tile column x >= 0
        if (row < THIN_HALO || row >= THIN_RH - THIN_HALO || y >= height) continue;
        const thin_word w = rows[0][row + 1];
        if (lane >= THIN_HALO && lane < THIN_RW - THIN_HALO && x < width)
            dst[(size_t)y * (size_t)width + (size_t)x] = (uint8_t)((w >> lane) & 1);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) last = max(last, __shfl_xor(last, off, 64));
    if (lane == 0 && last > 0) atomicMax(changed_flag, last);
}

// The number of launches (passes), or -1 when a HIP call failed (*err holds it).  *iterations: the iterations the rule ran.
int launch_thin_masks(hipStream_t s, int V, int height, int width, uint8_t* masks, uint8_t* scratch, int* changed_flag,
                      int max_iterations, int* iterations, hipError_t* err) {
    const size_t plane = (size_t)height * (size_t)width;
    const dim3 tiles((unsigned)((width + THIN_TW - 1) / THIN_TW), (unsigned)((height + THIN_TH - 1) / THIN_TH));
    uint8_t *src = masks, *dst = scratch;
    int passes = 0, done = 0, last_change = 0, changed = 0;
    for (;;) {
        const int k = max_iterations > 0 ? std::min(THIN_K, max_iterations - done) : THIN_K;
        if ((*err = hipMemsetAsync(changed_flag, 0, sizeof(int), s)) != hipSuccess) return -1;
        {
            ProfScope p("thin_pass", s);
            for (int v0 = 0; v0 < V; v0 += THIN_MAX_VIEWS) {
                const int nv = std::min(THIN_MAX_VIEWS, V - v0);
                hipLaunchKernelGGL(k_thin_pass, dim3(tiles.x, tiles.y, nv), dim3(THIN_THREADS), 0, s, height, width,
                                   src + (size_t)v0 * plane, dst + (size_t)v0 * plane, k, changed_flag);
            }
        }
        passes++;
        if ((*err = hipMemcpyAsync(&changed, changed_flag, sizeof(int), hipMemcpyDeviceToHost, s)) != hipSuccess) return -1;
        if ((*err = hipStreamSynchronize(s)) != hipSuccess) return -1;
        std::swap(src, dst);   // src holds the newest state
        if (changed > 0) last_change = done + changed;
        done += k;
        if (changed < k) break;   // an iteration of this pass changed nothing anywhere: settled
        if (max_iterations > 0 && done >= max_iterations) break;
    }
    // The newest state lies in scratch after an odd number of passes.  When the last of several passes changed nothing,
    // masks (written by the pass before it) already equals it; the first pass also normalises the bytes, so it is copied
    if (src != masks && (passes == 1 || changed > 0)) {
        if ((*err = hipMemcpyAsync(masks, scratch, (size_t)V * plane, hipMemcpyDeviceToDevice, s)) != hipSuccess) return -1;
    }
    *iterations = max_iterations > 0 ? std::min(max_iterations, last_change + 1) : last_change + 1;
    return passes;
}

}  // namespace cgs
