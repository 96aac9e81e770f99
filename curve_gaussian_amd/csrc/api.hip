// C ABI of libcurvegs.so (see include/curvegs.h): host-side sequencing of the HIP kernels on the caller's stream.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <stdlib.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "kernels.h"

namespace cgs {

static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
// An entry's rejection of its arguments: the thread's error text and the status in one return statement
__attribute__((format(printf, 1, 2))) static int reject(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return CGS_ERR_INVALID_ARGUMENT;
}

// ---------------------------------------------------------------- per-kernel timing (bench.py roofline leg)
static bool g_prof_on = false;
struct ProfRec { hipEvent_t e0, e1; const char* name; };
static std::vector<ProfRec> g_pending;
static std::map<std::string, std::pair<double, int64_t>> g_totals;
static std::vector<std::string> g_names_storage;
static std::mutex g_prof_mu;

ProfScope::ProfScope(const char* n, hipStream_t s) : name(n), stream(s), on(g_prof_on) {
    if (on) {
        (void)hipEventCreate(&e0);
        (void)hipEventCreate(&e1);
        (void)hipEventRecord(e0, stream);
    }
}
ProfScope::~ProfScope() {
    if (on) {
        (void)hipEventRecord(e1, stream);
        std::lock_guard<std::mutex> lk(g_prof_mu);
        g_pending.push_back({e0, e1, name});
    }
}

bool check_launch(const char* what, bool debug, hipStream_t s) {
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && debug) e = hipStreamSynchronize(s);  // reference CHECK_CUDA semantics, auxiliary.h:178-185
    if (e != hipSuccess) {
        set_error("%s failed: %s", what, hipGetErrorString(e));
        return false;
    }
    return true;
}
// The tail of an entry whose launches are queued: the launch check on the entry's stream.
static int finish(const char* what, void* stream_) {
    return check_launch(what, false, (hipStream_t)stream_) ? CGS_OK : CGS_ERR_HIP;
}

// ---- the entries with a depth-gated (_depth) or near-clipped (_clipped) sibling (include/curvegs.h).  Each pair has one
// <op>_entry that holds the checks once: `name` is the entry that was called, `gate` is NULL for the ungated entry and `near`
// is NULL for the unclipped one.  The gate's own checks are cgs_point_mask_depth's: a finite slack >= 0 and a depth pointer.
static bool slack_ok(double slack) { return slack >= 0.0 && !std::isinf(slack); }   // a NaN fails the comparison
static bool near_ok(double near) { return near > 0.0 && !std::isinf(near); }        // a NaN fails the comparison
static bool slack_bad(const DepthGate* gate) { return gate && !slack_ok(gate->slack); }
static bool depth_missing(const DepthGate* gate) { return gate && !gate->depth; }
static int reject_slack(const char* name, const DepthGate* gate) {
    return reject("%s: invalid argument (slack=%g; the slack is finite and >= 0)", name, gate->slack);
}

// Binning capacity hints, one set per workload shape (P, width, height): a process that alternates train and test cameras,
// two resolutions or two models keeps a separate history for each instead of thrashing one (each mismatch used to cost a
// bucket overflow and an exact-path redo).  Small LRU table behind a mutex; the three numbers of an entry:
//   R     num_rendered of the previous forward of this shape (speculative binning capacity of the exact path)
//   max   longest tile list seen recently (decaying maximum): sizes the fixed-capacity buckets of the single-pass binning
//   big   splats with oversized tile rects seen by the previous blocking forward: non-zero switches their deferral to
//         k_scatter_big on (one more launch, only worth it when there are any -- room-scale scenes with near-camera splats)
struct BinHints { int64_t R = 0, max = 0, big = 0; };
// bucket scatter: splats per wave from the instance count the shape binned last time (profiles/r04_experiments.md #19: 12 wins
// at cfg3 / cfg5 -- 1.6 M / 8 M instances --, 8 at cfg2 / cfg4 -- 0.4 M / 0.17 M)
static inline int scatter_spw(const BinHints& h) { return (h.R > 0 && h.R < 800000) ? 8 : 12; }
struct HintEntry { int dev = -1, P = -1, W = 0, H = 0; uint64_t stamp = 0; BinHints h; };   // dev: the HIP device the shape was seen on
static std::mutex g_hint_mu;
static HintEntry g_hint_tab[32];
static uint64_t g_hint_clock = 0;
// Exact match, or nullptr.  (A pure lookup never inserts: cgs_view_forward / cgs_rasterize_forward_static only ask.)
static int current_device() {
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess) d = 0;
    return d;
}
static HintEntry* hint_find_locked(int dev, int P, int W, int H) {
    for (auto& e : g_hint_tab)
        if (e.dev == dev && e.P == P && e.W == W && e.H == H) { e.stamp = ++g_hint_clock; return &e; }
    return nullptr;
}
// Most recently used entry of the same resolution but another splat count: a topology edit (densify / prune / split) changes
// P by a few curves, and the new cloud bins almost like the old one -- its history seeds the new shape (R scaled by the
// splat ratio) instead of sending the next forward of every resolution through the exact path again.
static const HintEntry* hint_neighbour_locked(int dev, int W, int H) {
    const HintEntry* best = nullptr;
    for (auto& e : g_hint_tab)
        if (e.dev == dev && e.P > 0 && e.W == W && e.H == H && (!best || e.stamp > best->stamp)) best = &e;
    return best;
}
static BinHints hint_seed_locked(int dev, int P, int W, int H) {
    BinHints h;
    if (const HintEntry* nb = hint_neighbour_locked(dev, W, H)) {
        h = nb->h;
        h.R = (int64_t)((double)nb->h.R * (double)P / (double)nb->P);
    }
    return h;
}
static HintEntry* hint_entry_locked(int dev, int P, int W, int H) {   // find or insert (LRU eviction)
    if (HintEntry* e = hint_find_locked(dev, P, W, H)) return e;
    const BinHints seed = hint_seed_locked(dev, P, W, H);
    HintEntry* lru = &g_hint_tab[0];
    for (auto& e : g_hint_tab)
        if (e.stamp < lru->stamp) lru = &e;
    *lru = HintEntry{};
    lru->dev = dev; lru->P = P; lru->W = W; lru->H = H; lru->stamp = ++g_hint_clock; lru->h = seed;
    return lru;
}
// (the shape's history belongs to the CURRENT device: two ranks' or two models' views on different GPUs of one process do not
// share bucket capacities; `dev` < 0 = ask the runtime)
static BinHints hints_load(int P, int W, int H, int dev = -1) {
    if (dev < 0) dev = current_device();
    std::lock_guard<std::mutex> lk(g_hint_mu);
    if (HintEntry* e = hint_find_locked(dev, P, W, H)) return e->h;
    return hint_seed_locked(dev, P, W, H);
}
// R < 0 / big < 0: leave that field; longest: folded into the decaying maximum
static void hints_update(int P, int W, int H, int64_t R, uint32_t longest, int64_t big, int dev = -1) {
    if (dev < 0) dev = current_device();
    std::lock_guard<std::mutex> lk(g_hint_mu);
    BinHints& h = hint_entry_locked(dev, P, W, H)->h;
    if (R >= 0) h.R = R;
    if (big >= 0) h.big = big;
    // Slowly decaying maximum.  A bucket overflow costs a whole second forward through the exact path, spare capacity only
    // memory (12 bytes per slot and tile), and a training loop cycles through dozens of views whose longest lists differ by
    // tens of per cent: at the round-4 rate of 1/16 per call seven sparser views in a row shrank the capacity by a third
    // and the next dense view overflowed (the general route's eager time was bimodal, 0.40 / 0.53 ms at cfg3).  1/1024 per
    // call (at least one entry: below 1 024 the shift alone would never decay) keeps 94 % after 64 calls -- inside the 25 %
    // margin -- and still follows a cloud that thins out for good.
    h.max = std::max<int64_t>((int64_t)longest, h.max - std::max<int64_t>(1, h.max >> 10));
}
static thread_local int64_t g_last_visible = -1;   // radii > 0 count of the last cgs_view_forward_checked
static thread_local int64_t g_last_stats[3] = {0, 0, 0};  // num_rendered, longest tile list, binning path (0 exact, 1 bucket)

// Device-side zero fill.  hipMemsetAsync is NOT used by the entries that are captured into graphs (the rasterizer, the view
// route, the losses, the regularizers and Adam): captured into a hipGraph (ROCm 7.0 runtime under PyTorch 2.10) its memset
// node cleared the buffer on the first replay only -- later replays ran on stale histograms / partial sums.  A plain kernel
// node replays correctly, and hipMemsetAsync is a fill kernel anyway.  The edge-map launchers do use it and are not captured:
// launch_point_mask and launch_edge_score_reduce (edge_score.hip), launch_edge_trace (edge_detect.hip), launch_thin_masks
// (edge_thin.hip), launch_ray_claims (edge_seed.hip), launch_mesh_depth and launch_point_mask_depth (edge_occlusion.hip), launch_mesh_contours (mesh_contours.hip), launch_surfel_depth (surfel_depth.hip); so does cgs_segment_merge_labels below for an empty input.
__global__ void __launch_bounds__(256) k_zero_words(uint32_t* __restrict__ p, size_t words) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += stride) p[i] = 0u;
}
__global__ void __launch_bounds__(256) k_zero_vec(uint4* __restrict__ p, size_t n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) p[i] = make_uint4(0u, 0u, 0u, 0u);
}
static hipError_t zero_async(void* p, size_t bytes, hipStream_t s) {
    if (bytes == 0) return hipSuccess;
    if (!(bytes & 15u) && !(reinterpret_cast<uintptr_t>(p) & 15u)) {
        const size_t n = bytes / 16;
        const int blocks = (int)std::min<size_t>((n + 255) / 256, 8192);
        hipLaunchKernelGGL(k_zero_vec, dim3(blocks), dim3(256), 0, s, reinterpret_cast<uint4*>(p), n);
        return hipGetLastError();
    }
    if ((bytes & 3u) || (reinterpret_cast<uintptr_t>(p) & 3u)) return hipMemsetAsync(p, 0, bytes, s);  // never the case here
    const size_t words = bytes / 4;
    const int blocks = (int)std::min<size_t>((words + 255) / 256, 4096);
    hipLaunchKernelGGL(k_zero_words, dim3(blocks), dim3(256), 0, s, reinterpret_cast<uint32_t*>(p), words);
    return hipGetLastError();
}
// ... for an entry: a failure leaves `what` as the error text, and the entry returns CGS_ERR_HIP
static bool zeroed(void* p, size_t bytes, hipStream_t s, const char* what) {
    if (zero_async(p, bytes, s) == hipSuccess) return true;
    set_error("%s", what);
    return false;
}

// Operator API (cgs_rasterize_forward / _backward): the forward tags its tile lists and lets the scatter raise a device word
// when some visible splat's colour or all_map[3] is not exactly 1; a backward that needs neither colour nor depth / all_map
// gradients then launches the pair-major unit-colour kernel AND the general training instance, and that word decides on the
// device which of the two runs (no host sync).  CGS_OPT_GENERAL_BACKWARD in that call's `debug` bits keeps the general instance only (A/B, tests).
static inline bool list_tags_fit(int P) { return (long long)P < (1ll << LIST_TAG_SHIFT); }
constexpr int NONUNIT_WORD = 8;            // index into ImageState::work (cleared with the tile histogram)
// tile sort inside the forward compositor; CGS_FUSED_TILE_SORT=0 (read once) selects the separate sort launch for A/B runs
static inline bool fuse_sort() {
    static const bool on = [] { const char* e = getenv("CGS_FUSED_TILE_SORT"); return !(e && e[0] == '0'); }();
    return on;
}
// Shared curve sampling for several views of ONE parameter state (cgs_view_forward_shared, CGS_VIEW_SHARED in
// cgs_view_backward's flags): the grid-wide norm pass of the forward and the last pass of the sampling backward run once per
// view BATCH (cgs_view_shared_begin / _end) instead of once per view -- the parameters do not change inside a batch and that
// backward pass is linear in the per-splat gradients.  A per-call choice: nothing process-wide changes what another caller's
// cgs_view_forward / cgs_view_backward does.
constexpr int VIEW_MODE_MASK = 3, VIEW_MODE_SHARED = 4;
static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace cgs

using namespace cgs;

// Longest tile list of a finished scatter, for the checked (blocking) view forward: one small launch between the scatter
// and the compositor, so the host's wait ends when the BINNING is done and the compositor is still running.
constexpr int STAT_BLOCKS = 64;            // blocks of k_count_stats = chunks of k_visible_compact
constexpr int VIS_COUNT_WORD = 16;         // work[16 .. 16 + STAT_BLOCKS): splats with radii > 0 per chunk of ceil(P / STAT_BLOCKS)
__global__ void __launch_bounds__(256) k_count_stats(const uint32_t* __restrict__ tile_count, int tiles, const int* __restrict__ radii,
                                                     int P, const uint32_t* __restrict__ big, uint32_t* __restrict__ out4,
                                                     uint32_t* __restrict__ vis_counts) {
    // (same-address atomics serialise at ~15 ns each: one per wave -- 768 of them -- made this reduction take 12.7 us of the
    // host's critical path, profiles/r05_kernel_stats.csv; one per BLOCK after an LDS step: 64 blocks x 3)
    __shared__ uint32_t s_part[3][4];
    uint32_t mx = 0, sum = 0, vis = 0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < tiles; i += gridDim.x * 256) {
        const uint32_t c = tile_count[i];
        mx = max(mx, c);
        sum += c;
    }
    // visible splats of this block's CONTIGUOUS chunk: the per-chunk counts are what k_visible_compact needs to write
    // (radii > 0).nonzero() in order without a scan of its own
    const int chunk = (P + (int)gridDim.x - 1) / (int)gridDim.x;
    const int lo = blockIdx.x * chunk, hi = min(P, lo + chunk);
    for (int i = lo + threadIdx.x; i < hi; i += 256) vis += radii[i] > 0 ? 1u : 0u;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        mx = max(mx, (uint32_t)__shfl_xor((int)mx, off, 64));
        sum += (uint32_t)__shfl_xor((int)sum, off, 64);
        vis += (uint32_t)__shfl_xor((int)vis, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        s_part[0][threadIdx.x >> 6] = sum;
        s_part[1][threadIdx.x >> 6] = mx;
        s_part[2][threadIdx.x >> 6] = vis;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t bvis = s_part[2][0] + s_part[2][1] + s_part[2][2] + s_part[2][3];
        vis_counts[blockIdx.x] = bvis;
        atomicAdd(&out4[0], s_part[0][0] + s_part[0][1] + s_part[0][2] + s_part[0][3]);                  // num_rendered
        atomicMax(&out4[1], max(max(s_part[1][0], s_part[1][1]), max(s_part[1][2], s_part[1][3])));      // longest tile list
        atomicAdd(&out4[2], bvis);   // splats with radii > 0 (sizes render()'s visibility_filter without a host sync)
        if (blockIdx.x == 0) out4[3] = *big;   // splats with oversized tile rects (final after the scatter)
    }
}
// (radii > 0).nonzero() (gaussian_renderer/__init__.py:150) in one launch: block b writes the indices of its chunk's
// visible splats, in order, behind those of the chunks before it (their counts come from k_count_stats).
__global__ void __launch_bounds__(256) k_visible_compact(const int* __restrict__ radii, int P, const uint32_t* __restrict__ vis_counts,
                                                         long long* __restrict__ out) {
    __shared__ uint32_t s_wave[4];
    uint32_t base = 0;
    for (int b = 0; b < (int)blockIdx.x; b++) base += vis_counts[b];   // (<= 63 uniform loads)
    const int chunk = (P + (int)gridDim.x - 1) / (int)gridDim.x;
    const int lo = blockIdx.x * chunk, hi = min(P, lo + chunk);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i0 = lo; i0 < hi; i0 += 256) {
        const int i = i0 + (int)threadIdx.x;
        const bool v = i < hi && radii[i] > 0;
        const uint64_t bal = __ballot(v);
        if (lane == 0) s_wave[wave] = (uint32_t)__builtin_popcountll(bal);
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < 4; w++) {
            const uint32_t c = s_wave[w];
            before += w < wave ? c : 0u;
            all += c;
        }
        if (v) out[base + before + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u))] = (long long)i;
        base += all;
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------- render() epilogue
// gaussian_renderer/__init__.py:138-145 for the fused view route in ONE launch: the clamp of the image and the view -> world
// transform of the direction map (the reference runs a clamp kernel and a [H*W,3] x [3,3] matmul on a 1600^2 image), and the
// clamp's gradient mask for the way back.
__global__ void __launch_bounds__(256) k_render_epilogue(size_t npix, const float* __restrict__ color_raw, const float* __restrict__ all_map,
                                                         const float* __restrict__ wv, int clamp, float* __restrict__ color_out,
                                                         float* __restrict__ dir_out) {
    float w00 = 0.f, w01 = 0.f, w02 = 0.f, w10 = 0.f, w11 = 0.f, w12 = 0.f, w20 = 0.f, w21 = 0.f, w22 = 0.f;
    if (dir_out) {   // (viewmatrix may be NULL for a clamp-only call)
        w00 = wv[0]; w01 = wv[1]; w02 = wv[2]; w10 = wv[4]; w11 = wv[5]; w12 = wv[6]; w20 = wv[8]; w21 = wv[9]; w22 = wv[10];
    }
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (size_t)gridDim.x * 256) {
        if (color_out) {
            const float c = color_raw[i];
            color_out[i] = clamp ? fminf(fmaxf(c, 0.f), 1.f) : c;
        }
        if (dir_out) {   // out_i = sum_k d_k wv[i][k]   (rendered_dir.permute(1, 2, 0) @ world_view_transform[:3, :3].T)
            const float d0 = all_map[i], d1 = all_map[npix + i], d2 = all_map[2 * npix + i];
            dir_out[i] = d0 * w00 + d1 * w01 + d2 * w02;
            dir_out[npix + i] = d0 * w10 + d1 * w11 + d2 * w12;
            dir_out[2 * npix + i] = d0 * w20 + d1 * w21 + d2 * w22;
        }
    }
}
__global__ void __launch_bounds__(256) k_clamp_backward(size_t n, const float* __restrict__ raw, const float* __restrict__ g_in,
                                                        float* __restrict__ g_out) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const float x = raw[i];
        g_out[i] = (x >= 0.f && x <= 1.f) ? g_in[i] : 0.f;   // torch.clamp's backward: the gradient passes where min <= x <= max
    }
}

static void launch_render_epilogue(hipStream_t s, size_t npix, const float* color_raw, const float* all_map, const float* wv,
                                   int clamp, float* color_out, float* dir_out) {
    hipLaunchKernelGGL(k_render_epilogue, dim3((unsigned)std::min<size_t>((npix + 255) / 256, 4096)), dim3(256), 0, s, npix,
                       color_raw, all_map, wv, clamp, color_out, dir_out);
}

// ---------------------------------------------------------------------------------------------- shared sequencing
// Tile grid and focal lengths of one W x H frame (rasterizer_impl.cu:227-228)
struct Frame {
    int W, H, gx, gy, tiles;
    size_t npix;
    float focal_x, focal_y;
    Frame(int width, int height, float tan_fovx = 1.f, float tan_fovy = 1.f)
        : W(width), H(height), gx((width + TILE - 1) / TILE), gy((height + TILE - 1) / TILE), tiles(gx * gy),
          npix((size_t)width * height), focal_x(width / (2.0f * tan_fovx)), focal_y(height / (2.0f * tan_fovy)) {}
};
// The states carved from the three buffers (a NULL binning buffer is skipped: the operator forward sizes it later).
// clear_bytes: tile_count, tile_cursor and the status words are adjacent 128B-aligned carve-outs, cleared by one launch.
struct States { GeomState geom; BinState bin; ImageState img; size_t clear_bytes; };
static States carve_states(const Frame& f, int P, const void* geometry, const void* binning, size_t bin_slots, const void* image) {
    char *gchunk = (char*)geometry, *bchunk = (char*)binning, *ichunk = (char*)image;
    States b{};
    b.geom = geom_from_chunk(gchunk, (size_t)P);
    if (bchunk) b.bin = bin_from_chunk(bchunk, bin_slots);
    b.img = image_from_chunk(ichunk, f.npix, (size_t)f.tiles);
    b.clear_bytes = (size_t)((char*)(b.img.total + TOTAL_WORDS) - (char*)b.img.tile_count);
    return b;
}

// Splat inputs of the two operator forwards: exactly one of shs / colors_precomp and one of (scales, rotations) /
// cov3D_precomp, all_map with render_geo, cam_pos with shs, rotations and all_map 16-byte aligned
static bool splat_inputs_ok(const char* fn, int M, const float* means3D, const float* shs, const float* colors_precomp,
                            const float* opacities, const float* scales, const float* rotations, const float* cov3D_precomp,
                            const float* all_map, const float* cam_pos, int render_geo, const int* radii) {
    if (!means3D || !opacities || !radii || (!shs == !colors_precomp) ||
        (cov3D_precomp ? (scales || rotations) : (!scales || !rotations)) || (render_geo && !all_map) ||
        (shs && (!cam_pos || M <= 0))) {
        set_error("%s: inconsistent inputs (need exactly one of shs/colors_precomp and one of "
                  "(scales,rotations)/cov3D_precomp; all_map is required with render_geo)", fn);
        return false;
    }
    if (!aligned16(rotations) || !aligned16(all_map)) {
        set_error("%s: rotations/all_map must be 16-byte aligned", fn);
        return false;
    }
    return true;
}
// A caller-chosen bucket capacity and the binning buffer it needs
static bool bucket_cap_ok(const char* fn, uint32_t bucket_capacity, int tiles, size_t binning_bytes) {
    const uint64_t slots = (uint64_t)bucket_capacity * (uint64_t)tiles;
    if (bucket_capacity > bucket_cap_limit() || slots >= (1ull << 31) || binning_bytes < cgs_binning_bytes((int64_t)slots)) {
        set_error("%s: bucket capacity %u needs %zu binning bytes (got %zu; limit %u per tile)", fn, bucket_capacity,
                  cgs_binning_bytes((int64_t)slots), binning_bytes, bucket_cap_limit());
        return false;
    }
    return true;
}
// Bucket capacity for the longest tile list seen recently: 1.25 x + 64, rounded up to 64
static inline uint64_t bucket_cap_for(int64_t longest) { return (((uint64_t)longest * 5 / 4 + 64) + 63) & ~63ull; }

// Status readback of the forwards that wait for one: a pool of slots (pinned 16-byte buffer + event, created on first use).
// cgs_rasterize_forward holds a slot for the length of its call; a checked view forward hands its slot out as the HANDLE that
// cgs_view_forward_wait releases, so forwards of different threads, devices, streams or models are independent (a handle
// dropped between begin and wait holds its slot until cgs_view_forward_abandon).  An event records only on streams of the
// device it was created on: a forward takes an idle slot of the current device, else a fresh one, else an idle slot of
// another device, whose event it re-creates.
struct StatSlot {
    uint32_t* h = nullptr;
    hipEvent_t ev = nullptr;
    int dev = -1, P = 0, W = 0, H = 0;
    uint64_t cap = 0;
    bool busy = false, in_flight = false;   // in_flight: a copy queued and not yet waited for
};
constexpr int STAT_SLOTS = 64;
static StatSlot g_slots[STAT_SLOTS];
static std::mutex g_slot_mu;
static int slot_acquire() {   // -> slot index, or a negative status
    const int dev = current_device();
    std::lock_guard<std::mutex> lk(g_slot_mu);
    int fresh = -1, other = -1;
    for (int i = 0; i < STAT_SLOTS; i++) {
        StatSlot& v = g_slots[i];
        if (v.busy) continue;
        if (v.dev == dev) { v.busy = true; return i; }
        if (!v.h && fresh < 0) fresh = i;
        if (v.h && other < 0) other = i;
    }
    const int i = fresh >= 0 ? fresh : other;
    if (i < 0) {
        set_error("cgs_view_forward_begin: no free status slot for device %d (%d slots; every begin needs its cgs_view_forward_wait)",
                  dev, STAT_SLOTS);
        return CGS_ERR_INVALID_ARGUMENT;
    }
    StatSlot& v = g_slots[i];
    if (v.ev) (void)hipEventDestroy(v.ev);
    v.ev = nullptr;
    v.dev = -1;
    hipError_t e = v.h ? hipSuccess : hipHostMalloc((void**)&v.h, 4 * sizeof(uint32_t), hipHostMallocDefault);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&v.ev, hipEventDisableTiming);
    if (e != hipSuccess) {
        set_error("pinned readback buffer / event creation failed");
        return CGS_ERR_HIP;
    }
    v.dev = dev;
    v.busy = true;
    return i;
}
static bool slot_held(int i) {   // (a handle of an outstanding forward)
    std::lock_guard<std::mutex> lk(g_slot_mu);
    return i >= 0 && i < STAT_SLOTS && g_slots[i].busy;
}
static void slot_release(int i) {
    std::lock_guard<std::mutex> lk(g_slot_mu);
    g_slots[i].busy = false;
}
// a copy still in flight lands before the pinned words can go to another forward
static void slot_abandon(int i) {
    if (g_slots[i].in_flight) (void)hipEventSynchronize(g_slots[i].ev);
    g_slots[i].in_flight = false;
    slot_release(i);
}
static bool slot_read(int i, const uint32_t* words, hipStream_t s, const char* what) {   // 4 status words + the event behind them
    hipError_t e = hipMemcpyAsync(g_slots[i].h, words, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipEventRecord(g_slots[i].ev, s);
    g_slots[i].in_flight = true;
    if (e != hipSuccess) set_error("%s: status readback failed: %s", what, hipGetErrorString(e));
    return e == hipSuccess;
}
static bool slot_sync(int i, const char* what) {
    const hipError_t e = hipEventSynchronize(g_slots[i].ev);
    g_slots[i].in_flight = e != hipSuccess;
    if (e != hipSuccess) set_error("%s: status readback failed: %s", what, hipGetErrorString(e));
    return e == hipSuccess;
}
// A bucket forward's readback (num_rendered, longest list, visible splats, oversized rects) taken in: the shape's binning
// hints (num_rendered only when no bucket overflowed), cgs_last_forward_stats and cgs_last_forward_visible
static bool slot_wait(int i, const char* what) {
    if (!slot_sync(i, what)) return false;
    const StatSlot& v = g_slots[i];
    const uint32_t longest = v.h[1];
    hints_update(v.P, v.W, v.H, (uint64_t)longest <= v.cap ? (int64_t)v.h[0] : -1, longest, (int64_t)v.h[3], v.dev);
    g_last_stats[0] = (int64_t)v.h[0]; g_last_stats[1] = (int64_t)longest; g_last_stats[2] = 1;
    g_last_visible = (int64_t)v.h[2];
    return true;
}

// Bucket binning and compositing behind the preprocess of every bucket forward: scatter into buckets of `cap` slots per tile;
// with a readback slot (>= 0), the status words reduced and copied to it right behind the SCATTER, so that the host's wait
// overlaps the compositor; the tile sort (inside the compositor when `cap` allows) and the compositor.  `tag` matters only
// without `unit` (the unit-colour compositors always tag).  The epilogue outputs (either may be NULL) are written by the
// sorting compositor, else by one launch behind the other one.
static bool bucket_tail(hipStream_t s, const char* what, const Frame& f, const States& b, uint64_t cap, int P, const int* radii,
                        const BinHints& hints, int cull, uint32_t* nonunit, bool geo, bool unit, bool tag,
                        const float* background, float* out_color, float* out_invdepth, float* out_all_map,
                        float* color_clamped, float* dir_out, const float* wv, int slot) {
    launch_scatter_bucket(s, P, radii, b.geom.rec, f.gx, f.gy, b.img.tile_count, b.bin.keys, (uint32_t)cap, cull, b.img.total + 3,
                          hints.big > 0 ? b.img.tile_cursor : nullptr, (uint32_t)f.tiles, nonunit, scatter_spw(hints));
    if (slot >= 0) {
        uint32_t* const stat = b.img.work + 4;   // four words of the (cleared) work block
        hipLaunchKernelGGL(k_count_stats, dim3(STAT_BLOCKS), dim3(256), 0, s, b.img.tile_count, f.tiles, radii, P, b.img.total + 3,
                           stat, b.img.work + VIS_COUNT_WORD);
        if (!slot_read(slot, stat, s, what)) return false;
        StatSlot& v = g_slots[slot];
        v.P = P; v.W = f.W; v.H = f.H; v.cap = cap;
    }
    if (render_fwd_can_sort((uint32_t)cap) && fuse_sort()) {
        launch_render_fwd_sorting(s, geo, f.tiles, b.img.tile_count, b.bin.keys, (uint32_t)cap, b.img.ranges, b.img.total,
                                  b.bin.point_list, f.W, f.H, f.gx, b.geom.rec, b.img.final_T, b.img.n_contrib, background,
                                  out_color, out_invdepth, out_all_map, unit, tag, color_clamped, dir_out, wv);
    } else {
        launch_tile_sort_bucket(s, f.tiles, b.img.tile_count, b.img.ranges, b.img.total, b.bin.keys, b.bin.point_list,
                                (uint32_t)cap);
        launch_render_fwd(s, geo, f.tiles, b.img.ranges, b.bin.point_list, f.W, f.H, f.gx, b.geom.rec, b.img.final_T,
                          b.img.n_contrib, background, out_color, out_invdepth, out_all_map, unit, tag);
        if (color_clamped || dir_out)   // (long-list buckets: the non-sorting forward has no epilogue of its own)
            launch_render_epilogue(s, f.npix, out_color, out_all_map, wv, 1, color_clamped, dir_out);
    }
    return check_launch(what, false, s);
}

// The body of cgs_view_backward and cgs_view_backward_render (clamp_raw: the forward's unclamped image, or NULL)
static int view_backward_impl(int B, int m, const float* curve_points, const float* width, const uint8_t* is_bezier, const float* coef,
                      float eps, double* norms, const float* opacity_logit, const float* mask_logit, float mask_thr,
                      const float* colors_precomp, void* geometry_buffer, const void* binning_buffer, const void* image_buffer, const float* background,
                      int width_px, int height_px, const float* viewmatrix, const float* projmatrix, const float* cam_pos,
                      float tan_fovx, float tan_fovy, const int* radii, const float* dL_dout_color,
                      const float* dL_drotation_extra, float* dL_dmeans2D, float* dL_dcurve_points, float* dL_dwidth,
                      float* dL_dopacity_logit, float* dL_dmask_logit, float* scratch, int flags, void* stream_,
                      const float* clamp_raw) {
    hipStream_t s = (hipStream_t)stream_;
    if (clamp_raw && colors_precomp)
        return reject("cgs_view_backward_render: the folded clamp mask is part of the unit-colour path (no colors_precomp)");
    const int P = B * m;
    if (B <= 0 || m <= 0 || m > 32 || width_px <= 0 || height_px <= 0 || !curve_points || !width || !coef || !norms ||
        !opacity_logit || !geometry_buffer || !binning_buffer || !image_buffer || !background || !viewmatrix || !projmatrix ||
        !cam_pos || !radii || !dL_dout_color || !dL_dmeans2D || !dL_dcurve_points || !dL_dwidth || !dL_dopacity_logit ||
        !scratch || (mask_logit && !dL_dmask_logit) || !aligned16(curve_points) || !aligned16(coef) ||
        !aligned16(dL_drotation_extra) || !aligned16(dL_dcurve_points))
        return reject("cgs_view_backward: invalid argument");
    const Frame f(width_px, height_px, tan_fovx, tan_fovy);
    const States b = carve_states(f, P, geometry_buffer, binning_buffer, 1, image_buffer);
    // scratch: [B,13] per-curve partials of dL/d{curve_points, width} (k_view_bwd -> k_sample_bwd_close; curve_math.h,
    // sample_backward_tail).  Rounds 2-5 sent 15 floats per SPLAT through here.
    // training configuration: only dL/dcolour flows in, the colours themselves need no gradient; the forward wrote unit
    // colours unless it was given colors_precomp (same argument here): closed-form dL/dalpha, no recurrences (render.hip, UNIT)
    if (colors_precomp == nullptr)
        launch_render_bwd_unit(s, f.tiles, b.img.ranges, b.bin.point_list, width_px, height_px, f.gx, background, b.geom.rec,
                               b.img.final_T, b.img.n_contrib, dL_dout_color, b.geom.grad_acc, ACC_STRIDE_VIEW, nullptr, clamp_raw);
    else   // arbitrary colours: the general training instance (the forward did not tag the lists)
        launch_render_bwd(s, false, false, false, f.tiles, b.img.ranges, b.bin.point_list, width_px, height_px, f.gx, background,
                          b.geom.rec, b.img.final_T, b.img.n_contrib, dL_dout_color, nullptr, nullptr, b.geom.grad_acc,
                          ACC_STRIDE_VIEW);
    launch_view_backward(s, B, m, curve_points, width, is_bezier, coef, eps, norms, opacity_logit, mask_logit, mask_thr,
                         cam_pos, viewmatrix, projmatrix, tan_fovx, tan_fovy, f.focal_x, f.focal_y, width_px, height_px, radii,
                         b.geom.rec, b.geom.grad_acc, dL_drotation_extra, dL_dmeans2D, dL_dopacity_logit, dL_dmask_logit, scratch,
                         ((flags & CGS_VIEW_ACCUMULATE) ? 1 : 0) | ((flags & CGS_VIEW_SHARED) ? 2 : 0));
    if (!(flags & CGS_VIEW_SHARED))
        launch_sample_backward_close(s, B, m, curve_points, width, is_bezier, coef, eps, norms, scratch, dL_dcurve_points,
                                     dL_dwidth, (flags & CGS_VIEW_ACCUMULATE) ? 1 : 0);
    return finish("view_backward", s);
}

extern "C" {

const char* cgs_last_error(void) { return g_err; }
int cgs_version(void) { return 100; }
const char* cgs_target_arch(void) { return "gfx950"; }

size_t cgs_geometry_bytes(int P) {
    char* c = nullptr;
    geom_from_chunk(c, (size_t)(P > 0 ? P : 1));
    return (size_t)c + 128;
}
size_t cgs_image_bytes(int width, int height) {
    char* c = nullptr;
    const Frame f(width, height);
    image_from_chunk(c, f.npix, (size_t)f.tiles);
    return (size_t)c + 128;
}
size_t cgs_binning_bytes(int64_t R) {
    char* c = nullptr;
    bin_from_chunk(c, (size_t)(R > 0 ? R : 1));
    return (size_t)c + 128;
}

void cgs_reset_binning_hints(void) {
    std::lock_guard<std::mutex> lk(g_hint_mu);
    for (auto& e : g_hint_tab) e = HintEntry{};
}
void cgs_prof_enable(int on) { g_prof_on = on != 0; }
void cgs_prof_reset(void) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    for (auto& r : g_pending) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
    g_pending.clear();
    g_totals.clear();
}
int cgs_prof_collect(const char** names, double* total_ms, int64_t* launches, int cap) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    for (auto& r : g_pending) {
        (void)hipEventSynchronize(r.e1);
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.e0, r.e1) == hipSuccess) {
            auto& t = g_totals[r.name];
            t.first += ms;
            t.second += 1;
        }
        (void)hipEventDestroy(r.e0);
        (void)hipEventDestroy(r.e1);
    }
    g_pending.clear();
    g_names_storage.clear();
    for (auto& kv : g_totals) g_names_storage.push_back(kv.first);
    int n = 0;
    for (auto& kv : g_totals) {
        if (n < cap) {
            names[n] = g_names_storage[n].c_str();
            total_ms[n] = kv.second.first;
            launches[n] = kv.second.second;
        }
        n++;
    }
    return n;
}

int64_t cgs_rasterize_forward(cgs_alloc_fn geometry_alloc, void* geometry_user, cgs_alloc_fn binning_alloc,
                              void* binning_user, cgs_alloc_fn image_alloc, void* image_user, int P, int D, int M,
                              const float* background, int width, int height, const float* means3D, const float* shs,
                              const float* colors_precomp, const float* opacities, const float* scales,
                              float scale_modifier, const float* rotations, const float* cov3D_precomp,
                              const float* all_map, const float* viewmatrix, const float* projmatrix,
                              const float* cam_pos, float tan_fovx, float tan_fovy, int prefiltered, float* out_color,
                              float* out_invdepth, float* out_all_map, int antialiasing, int render_geo, int* radii,
                              int debug, void* stream_) {
    (void)prefiltered;
    hipStream_t s = (hipStream_t)stream_;
    g_last_visible = -1;   // (set again by the bucket path, whose status readback carries the count)
    if (P < 0 || width <= 0 || height <= 0 || !out_color || !out_invdepth || !out_all_map || !background ||
        !viewmatrix || !projmatrix)
        return reject("cgs_rasterize_forward: invalid argument (P=%d W=%d H=%d or NULL output/camera pointer)", P, width,
                      height);
    const Frame f(width, height, tan_fovx, tan_fovy);
    if (P == 0) {  // rasterize_points.cu:91: outputs stay zero-filled, nothing is rendered (not even background)
        if (!zeroed(out_color, f.npix * 4, s, "zero_async failed") || !zeroed(out_invdepth, f.npix * 4, s, "zero_async failed") ||
            !zeroed(out_all_map, f.npix * 16, s, "zero_async failed"))
            return CGS_ERR_HIP;
        return 0;
    }
    if (!splat_inputs_ok("cgs_rasterize_forward", M, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                         all_map, cam_pos, render_geo, radii))
        return CGS_ERR_INVALID_ARGUMENT;
    char* gchunk = (char*)geometry_alloc(geometry_user, cgs_geometry_bytes(P));
    char* ichunk = (char*)image_alloc(image_user, cgs_image_bytes(width, height));
    if (!gchunk || !ichunk) {
        set_error("cgs_rasterize_forward: geometry/image allocation callback returned NULL");
        return CGS_ERR_ALLOC;
    }
    States b = carve_states(f, P, gchunk, nullptr, 0, ichunk);
    const int cull = (debug & CGS_OPT_NO_TILE_CULLING) ? 0 : 1;   // per call (include/curvegs.h)
    debug &= CGS_OPT_DEBUG;
    // the status readback of this (blocking) call: a slot of the pool, given back (after its copy landed) when the call returns
    struct Lease { int i; ~Lease() { slot_abandon(i); } };
    const int slot = slot_acquire();
    if (slot < 0) return slot;
    const Lease lease{slot};
    const uint32_t* const h_tot = g_slots[slot].h;
    // tile_count == NULL (bucket binning): the kernel does not count, so it can clear the histogram/cursors/status words
    // itself; with counting, they are cleared by a separate launch first.  Either way it zeroes the gradient accumulators.
    auto preprocess = [&](uint32_t* tile_count) -> bool {
        launch_preprocess_fwd(s, P, D, M, means3D, scales, scale_modifier, rotations, opacities, shs, b.geom.clamped,
                              cov3D_precomp, colors_precomp, render_geo ? all_map : nullptr, viewmatrix, projmatrix,
                              cam_pos, width, height, tan_fovx, tan_fovy, f.focal_x, f.focal_y, radii, b.geom.rec, b.geom.rgb,
                              f.gx, f.gy, tile_count, antialiasing, cull, b.geom.grad_acc, b.img.tile_count,
                              tile_count ? 0 : b.clear_bytes / sizeof(uint32_t));
        return check_launch("preprocess_fwd", debug, s);
    };
    const bool tag = list_tags_fit(P);
    uint32_t* const nonunit = b.img.work + NONUNIT_WORD;

    // ---- path B: single-pass bucket binning (default once a previous forward has told us how long tile lists get).
    // The whole forward is enqueued back to back and the host only waits for the 16-byte readback (num_rendered is part of
    // the reference's API) while the compositor is already running.  A tile that outgrows its bucket raises the overflow
    // flag and the call falls through to the exact path below.
    const BinHints hints = hints_load(P, width, height);
    if (cull && !debug && hints.max > 0) {
        const uint64_t cap = bucket_cap_for(hints.max);
        if (cap <= bucket_cap_limit() && cap * (uint64_t)f.tiles < (1ull << 31)) {
            if (!preprocess(nullptr)) return CGS_ERR_HIP;
            char* bchunk = (char*)binning_alloc(binning_user, cgs_binning_bytes((int64_t)(cap * f.tiles)));
            if (!bchunk) {
                set_error("cgs_rasterize_forward: binning allocation callback returned NULL");
                return CGS_ERR_ALLOC;
            }
            b.bin = bin_from_chunk(bchunk, (size_t)(cap * f.tiles));
            if (!bucket_tail(s, "render_fwd", f, b, cap, P, radii, hints, cull, nonunit, render_geo != 0, false, tag, background,
                             out_color, out_invdepth, out_all_map, nullptr, nullptr, nullptr, slot) ||
                !slot_wait(slot, "cgs_rasterize_forward"))
                return CGS_ERR_HIP;
            if ((uint64_t)h_tot[1] <= cap) return (int64_t)h_tot[0];
            // overflow: the image just rendered is incomplete -- redo the binning with exact sizes
        }
    }

    // ---- path A: exact layout (count -> scan -> scatter -> sort); bit-identical to the reference's binning when
    // tile culling is off.  Used for the first forward, in debug mode, with culling off and after a bucket overflow.
    if (!zeroed(b.img.tile_count, b.clear_bytes, s, "zero_async(tile histogram) failed")) return CGS_ERR_HIP;
    if (!preprocess(b.img.tile_count)) return CGS_ERR_HIP;
    launch_scan_tiles(s, f.tiles, b.img.tile_count, b.img.ranges, b.img.total);
    if (!check_launch("scan_tiles", debug, s)) return CGS_ERR_HIP;

    // num_rendered has to reach the host (it sizes the binning buffer and is part of the reference's API).  Instead of
    // idling the GPU during that round trip (the reference blocks on a 4-byte cudaMemcpy, rasterizer_impl.cu:287), the
    // binning kernels are launched SPECULATIVELY into a buffer sized from the previous call's R (+25 %) while an event
    // marks the readback; the host then waits on the event only.  If the guess was too small (scene changed a lot)
    // the kernels skipped every tile that would not fit and are re-run on an exact-size buffer.
    if (!slot_read(slot, b.img.total, s, "cgs_rasterize_forward")) return CGS_ERR_HIP;
    const int64_t hint = hints.R;
    int64_t cap = 0;
    char* bchunk = nullptr;
    BinState bin{};
    if (hint > 0 && !debug) {
        cap = hint + hint / 4 + 4096;
        bchunk = (char*)binning_alloc(binning_user, cgs_binning_bytes(cap));
        if (!bchunk) {
            set_error("cgs_rasterize_forward: binning allocation callback returned NULL");
            return CGS_ERR_ALLOC;
        }
        bin = bin_from_chunk(bchunk, (size_t)cap);
        launch_scatter(s, P, radii, b.geom.rec, f.gx, f.gy, b.img.ranges, b.img.tile_cursor, bin.keys, (uint32_t)cap, cull, nonunit);
        launch_tile_sort_small(s, f.tiles, b.img.ranges, bin.keys, bin.point_list, (uint32_t)cap);
    }
    if (!slot_sync(slot, "cgs_rasterize_forward")) return CGS_ERR_HIP;
    const int64_t R = (int64_t)h_tot[0];
    const uint32_t max_count = h_tot[1];
    hints_update(P, width, height, R, max_count, -1);
    if (!bchunk || R > cap) {  // first call, debug mode, or the speculative buffer was too small: exact-size (re)run
        if (cap > 0 && !zeroed(b.img.tile_cursor, (size_t)f.tiles * sizeof(uint32_t), s, "zero_async(tile cursors) failed"))
            return CGS_ERR_HIP;
        cap = R;
        bchunk = (char*)binning_alloc(binning_user, cgs_binning_bytes(R));
        if (!bchunk) {
            set_error("cgs_rasterize_forward: binning allocation callback returned NULL");
            return CGS_ERR_ALLOC;
        }
        bin = bin_from_chunk(bchunk, (size_t)(R > 0 ? R : 1));
        if (R > 0) {
            launch_scatter(s, P, radii, b.geom.rec, f.gx, f.gy, b.img.ranges, b.img.tile_cursor, bin.keys, (uint32_t)cap, cull,
                           nonunit);
            if (!check_launch("scatter", debug, s)) return CGS_ERR_HIP;
            launch_tile_sort_small(s, f.tiles, b.img.ranges, bin.keys, bin.point_list, (uint32_t)cap);
            if (!check_launch("tile_sort", debug, s)) return CGS_ERR_HIP;
        }
    }
    if (R > 0) {
        launch_tile_sort_big(s, f.tiles, b.img.ranges, bin.keys, bin.point_list, max_count);  // no-op unless a list > 1024
        if (!check_launch("tile_sort", debug, s)) return CGS_ERR_HIP;
    }
    launch_render_fwd(s, render_geo != 0, f.tiles, b.img.ranges, bin.point_list, width, height, f.gx, b.geom.rec, b.img.final_T,
                      b.img.n_contrib, background, out_color, out_invdepth, out_all_map, false, tag);
    if (!check_launch("render_fwd", debug, s)) return CGS_ERR_HIP;
    g_last_stats[0] = R; g_last_stats[1] = (int64_t)max_count; g_last_stats[2] = 0;
    return R;
}

// Sync-free forward for stream-ordered / hipGraph-captured pipelines: caller-owned buffers, caller-chosen bucket
// capacity, single-pass bucket binning only, nothing read back.  Status lives in the image buffer (see header).
int cgs_rasterize_forward_static(void* geometry_buffer, void* binning_buffer, size_t binning_bytes, void* image_buffer,
                                 uint32_t bucket_capacity, int P, int D, int M, const float* background, int width,
                                 int height, const float* means3D, const float* shs, const float* colors_precomp,
                                 const float* opacities, const float* scales, float scale_modifier,
                                 const float* rotations, const float* cov3D_precomp, const float* all_map,
                                 const float* viewmatrix, const float* projmatrix, const float* cam_pos, float tan_fovx,
                                 float tan_fovy, float* out_color, float* out_invdepth, float* out_all_map,
                                 int antialiasing, int render_geo, int* radii, void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    if (P <= 0 || width <= 0 || height <= 0 || !out_color || !out_invdepth || !out_all_map || !background ||
        !viewmatrix || !projmatrix || !geometry_buffer || !binning_buffer || !image_buffer || bucket_capacity == 0)
        return reject("cgs_rasterize_forward_static: invalid argument (P=%d W=%d H=%d, NULL pointer or zero capacity)", P,
                      width, height);
    const Frame f(width, height, tan_fovx, tan_fovy);
    if (!splat_inputs_ok("cgs_rasterize_forward_static", M, means3D, shs, colors_precomp, opacities, scales, rotations,
                         cov3D_precomp, all_map, cam_pos, render_geo, radii) ||
        !bucket_cap_ok("cgs_rasterize_forward_static", bucket_capacity, f.tiles, binning_bytes))
        return CGS_ERR_INVALID_ARGUMENT;
    const uint64_t cap = bucket_capacity;
    const States b = carve_states(f, P, geometry_buffer, binning_buffer, (size_t)(cap * f.tiles), image_buffer);
    launch_preprocess_fwd(s, P, D, M, means3D, scales, scale_modifier, rotations, opacities, shs, b.geom.clamped,
                          cov3D_precomp, colors_precomp, render_geo ? all_map : nullptr, viewmatrix, projmatrix, cam_pos,
                          width, height, tan_fovx, tan_fovy, f.focal_x, f.focal_y, radii, b.geom.rec, b.geom.rgb, f.gx, f.gy,
                          nullptr, antialiasing, 1, b.geom.grad_acc, b.img.tile_count, b.clear_bytes / sizeof(uint32_t));
    const BinHints hints = hints_load(P, width, height);   // (from the caller's probing forwards of this shape)
    if (!bucket_tail(s, "rasterize_forward_static", f, b, cap, P, radii, hints, 1, b.img.work + NONUNIT_WORD, render_geo != 0,
                     false, list_tags_fit(P), background, out_color, out_invdepth, out_all_map, nullptr, nullptr, nullptr, -1))
        return CGS_ERR_HIP;
    return CGS_OK;
}

size_t cgs_image_status_offset(int width, int height) {
    char* c = nullptr;
    const Frame f(width, height);
    ImageState img = image_from_chunk(c, f.npix, (size_t)f.tiles);
    return (size_t)((char*)img.total - (char*)nullptr);
}
int cgs_status_words(void) { return TOTAL_WORDS; }
uint32_t cgs_bucket_capacity_limit(void) { return bucket_cap_limit(); }

void cgs_last_forward_stats(int64_t* num_rendered, int64_t* longest_tile_list, int* binning_path) {
    if (num_rendered) *num_rendered = g_last_stats[0];
    if (longest_tile_list) *longest_tile_list = g_last_stats[1];
    if (binning_path) *binning_path = (int)g_last_stats[2];
}

int cgs_rasterize_backward(int P, int D, int M, int64_t R, const float* background, int width, int height,
                           const float* means3D, const float* shs, const float* colors_precomp, const float* all_map,
                           const float* opacities, const float* scales, float scale_modifier, const float* rotations,
                           const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                           const float* cam_pos, float tan_fovx, float tan_fovy, const int* radii,
                           void* geometry_buffer, const void* binning_buffer, const void* image_buffer,
                           const float* dL_dout_color, const float* dL_dout_invdepth, const float* dL_dout_all_map,
                           float* dL_dmean2D, float* dL_dconic, float* dL_dopacity, float* dL_dcolor,
                           float* dL_dinvdepth, float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscale,
                           float* dL_drot, float* dL_dall_map, int antialiasing, int render_geo, int debug,
                           void* stream_) {
    (void)colors_precomp;
    (void)all_map;
    hipStream_t s = (hipStream_t)stream_;
    const bool general_only = (debug & CGS_OPT_GENERAL_BACKWARD) != 0;   // per call (include/curvegs.h)
    debug &= CGS_OPT_DEBUG;
    if (P == 0) return CGS_OK;
    if (P < 0 || width <= 0 || height <= 0 || !geometry_buffer || !binning_buffer || !image_buffer || !radii ||
        !dL_dout_color || !dL_dmean2D || !dL_dopacity || (shs && !dL_dcolor) || !dL_dmean3D || !dL_dcov3D ||
        !dL_dall_map || (!dL_dout_invdepth != !dL_dinvdepth) || (scales && (!dL_dscale || !dL_drot)) ||
        (shs && !dL_dsh))
        return reject("cgs_rasterize_backward: invalid argument");
    if (!dL_dcolor && ((render_geo && dL_dout_all_map) || dL_dout_invdepth))
        return reject("cgs_rasterize_backward: dL_dcolor may only be NULL when no depth / all_map gradients flow in");
    if (!aligned16(rotations) || !aligned16(dL_dconic) || !aligned16(dL_drot) || !aligned16(dL_dall_map))
        return reject("cgs_rasterize_backward: rotations/dL_dconic/dL_drot must be 16-byte aligned");
    const Frame f(width, height, tan_fovx, tan_fovy);
    const States b = carve_states(f, P, geometry_buffer, binning_buffer, (size_t)(R > 0 ? R : 1), image_buffer);

    // geom.grad_acc is zero here: the forward's preprocess kernel cleared it and k_preprocess_bwd clears it after use
    if (R > 0) {
        const bool geo = render_geo && dL_dout_all_map;
        const bool invd = dL_dout_invdepth != nullptr, colg = dL_dcolor != nullptr;
        const bool tagged = list_tags_fit(P);   // (the forward's own condition: both sides derive it from P)
        const uint32_t id_mask = tagged ? LIST_ID_MASK : 0xffffffffu;
        // Training instance (only dL/dcolour upstream, the colours themselves need no gradient): the reference's own call
        // (gaussian_renderer/__init__.py:96-129) passes all-ones colours and all_map[:, 3] == 1, for which dL/dalpha has the
        // closed form of render_unit_bwd.hip.  The ABI receives tensors and cannot know that on the host; the scatter of the
        // forward raised img.work[NONUNIT_WORD] if any visible splat deviates, and the two kernels test that word on entry.
        const uint32_t* gate = nullptr;
        if (tagged && !geo && !invd && !colg && !general_only) {
            gate = b.img.work + NONUNIT_WORD;
            launch_render_bwd_unit(s, f.tiles, b.img.ranges, b.bin.point_list, width, height, f.gx, background, b.geom.rec,
                                   b.img.final_T, b.img.n_contrib, dL_dout_color, b.geom.grad_acc, ACC_STRIDE, gate);
        }
        launch_render_bwd(s, geo, invd, colg, f.tiles, b.img.ranges, b.bin.point_list, width, height, f.gx, background,
                          b.geom.rec, b.img.final_T, b.img.n_contrib, dL_dout_color, dL_dout_invdepth, dL_dout_all_map,
                          b.geom.grad_acc, ACC_STRIDE, id_mask, gate);
        if (!check_launch("render_bwd", debug, s)) return CGS_ERR_HIP;
    }
    launch_preprocess_bwd(s, P, D, M, means3D, radii, shs, b.geom.clamped, opacities, scales, rotations, scale_modifier,
                          cov3D_precomp, viewmatrix, projmatrix, cam_pos, f.focal_x, f.focal_y, tan_fovx, tan_fovy, width,
                          height, b.geom.rec, b.geom.grad_acc, dL_dmean2D, dL_dconic, dL_dinvdepth, dL_dopacity, dL_dmean3D,
                          dL_dcolor, dL_dall_map, dL_dcov3D, dL_dsh, dL_dscale, dL_drot, antialiasing);
    if (!check_launch("preprocess_bwd", debug, s)) return CGS_ERR_HIP;
    return CGS_OK;
}

int cgs_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix, uint8_t* present,
                     void* stream_) {
    (void)projmatrix;
    if (P == 0) return CGS_OK;
    if (P < 0 || !means3D || !viewmatrix || !present) return reject("cgs_mark_visible: invalid argument");
    launch_mark_visible((hipStream_t)stream_, P, means3D, viewmatrix, present);
    return finish("mark_visible", stream_);
}


int cgs_sample_curves_forward(int B, int m, const float* curve_points, const float* width, const uint8_t* is_bezier,
                              const float* coef, float eps, double* norms, float* xyz, float* rotation,
                              float* scaling, void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    if (B == 0) return CGS_OK;
    if (B < 0 || m <= 0 || m > 32 || !curve_points || !width || !coef || !norms || !xyz || !rotation || !scaling ||
        !aligned16(curve_points) || !aligned16(rotation) || !aligned16(coef))
        return reject("cgs_sample_curves_forward: invalid argument (NULL or misaligned pointer, B=%d m=%d)", B, m);
    // (no zero fill of norms: k_sample_f12 writes the forward sums and clears the backward's, csrc/curve_math.h)
    launch_sample_forward(s, B, m, curve_points, width, is_bezier, coef, eps, norms, xyz, rotation, scaling);
    return finish("sample_curves_forward", s);
}

// ---------------------------------------------------------------------------------------------- fused per-view path
// One view of the training configuration, curve parameters in, image out (and back): the per-splat chains are fused
// (view.hip), the rasterizer is the sync-free single-pass bucket pipeline of cgs_rasterize_forward_static.
static int64_t view_forward_wait(int handle, int64_t* n_visible) {
    if (!slot_held(handle)) return reject("cgs_view_forward_wait: handle %d is not an outstanding checked forward", handle);
    const bool ok = slot_wait(handle, "cgs_view_forward_wait");
    const int64_t longest = (int64_t)g_slots[handle].h[1];
    if (ok && n_visible) *n_visible = g_last_visible;
    slot_release(handle);
    return ok ? longest : CGS_ERR_HIP;
}

// The gate of the two _depth forwards, checked after the sibling's own arguments and before the bucket capacity, under the
// name of the entry that was called: a gate, its three pointers, V >= 1, a host view inside [0, V) (a device view index is
// the kernel's to read), a slack >= 0 (+inf is allowed: it hides nothing; NaN fails the comparison) and planes of the
// image's size.  Nothing is launched before all of it holds.
static int view_gate_check(const char* name, const cgs_view_gate* gate, int width_px, int height_px, ViewGate& out) {
    if (!gate) return reject("%s: invalid argument (NULL gate)", name);
    if (!gate->planes || !gate->intr || !gate->w2c) return reject("%s: invalid argument (NULL plane or camera pointer)", name);
    if (gate->V < 1) return reject("%s: invalid argument (V=%d; the stack holds at least one view)", name, gate->V);
    if (!gate->view_index && (gate->view < 0 || gate->view >= gate->V))
        return reject("%s: invalid argument (view=%d outside [0, %d))", name, gate->view, gate->V);
    if (!(gate->slack >= 0.0)) return reject("%s: invalid argument (slack=%g; the slack is >= 0)", name, gate->slack);
    if (gate->height != height_px || gate->width != width_px)
        return reject("%s: invalid argument (planes %dx%d, image %dx%d; the planes have the image's size)", name, gate->width,
                      gate->height, width_px, height_px);
    out = ViewGate{gate->planes, gate->intr, gate->w2c, gate->view_index, gate->slack, gate->V, gate->view};
    return 0;
}

static int64_t view_forward_impl(int mode, int B, int m, const float* curve_points, const float* width, const uint8_t* is_bezier, const float* coef,
                     float eps, double* norms, const float* opacity_logit, const float* mask_logit, float mask_thr,
                     const float* colors_precomp, void* geometry_buffer, void* binning_buffer, size_t binning_bytes,
                     void* image_buffer, uint32_t bucket_capacity, const float* background, int width_px, int height_px,
                     const float* viewmatrix, const float* projmatrix, const float* cam_pos, float tan_fovx, float tan_fovy,
                     float* out_color, float* out_invdepth, float* out_all_map, int* radii, float* xyz, float* rotation,
                     float* scaling, void* stream_, float* out_color_clamped = nullptr, float* out_rend_dir = nullptr,
                     const char* gated_name = nullptr, const cgs_view_gate* gate = nullptr) {
    // gated_name: the _depth entry that was called (NULL: one of the five forwards as they always were, `gate` is not looked at)
    hipStream_t s = (hipStream_t)stream_;
    const int P = B * m;
    if (out_rend_dir && !out_all_map) return reject("cgs_view_forward: the direction map needs the all_map output");
    if (B <= 0 || m <= 0 || m > 32 || (long long)B * m >= (1ll << 28) || width_px <= 0 || height_px <= 0 || !curve_points ||
        !width || !coef || !norms ||
        !opacity_logit || !geometry_buffer || !binning_buffer || !image_buffer || bucket_capacity == 0 || !background ||
        !viewmatrix || !projmatrix || !cam_pos || !out_color || (!out_invdepth != !out_all_map) ||
        (!out_all_map && colors_precomp) || !radii || (xyz && (!rotation || !scaling)) || !aligned16(curve_points) || !aligned16(coef) || !aligned16(rotation))
        return reject("cgs_view_forward: invalid argument (B=%d m=%d W=%d H=%d, NULL / misaligned pointer or zero capacity)", B,
                      m, width_px, height_px);
    ViewGate vg{};
    if (gated_name) {
        if (const int rc = view_gate_check(gated_name, gate, width_px, height_px, vg)) return rc;
    }
    const Frame f(width_px, height_px, tan_fovx, tan_fovy);
    if (!bucket_cap_ok("cgs_view_forward", bucket_capacity, f.tiles, binning_bytes)) return CGS_ERR_INVALID_ARGUMENT;
    const uint64_t cap = bucket_capacity;
    const States b = carve_states(f, P, geometry_buffer, binning_buffer, (size_t)(cap * f.tiles), image_buffer);
    const bool shared = (mode & VIEW_MODE_SHARED) != 0;
    mode &= VIEW_MODE_MASK;
    // checked: the longest tile list (and the instance count, oversized-rect count) travel to the host right behind the
    // scatter; the compositor is queued before the host waits, so the wait overlaps it
    const bool checked = mode != 0;
    const int slot = checked ? slot_acquire() : -1;
    if (checked && slot < 0) return slot;
    // the norm pass writes the three forward sums and clears the backward's two: no zero-fill launch
    if (!shared) launch_sample_norms(s, B, m, curve_points, is_bezier, coef, norms);
    launch_view_forward(s, B, m, curve_points, width, is_bezier, coef, eps, norms, opacity_logit, mask_logit, mask_thr,
                        colors_precomp, cam_pos, viewmatrix, projmatrix, tan_fovx, tan_fovy, f.focal_x, f.focal_y, width_px,
                        height_px, f.gx, f.gy, xyz, rotation, scaling, radii, b.geom.rec, b.geom.grad_acc, b.img.tile_count,
                        b.clear_bytes / sizeof(uint32_t), gated_name ? &vg : nullptr);
    // k_view_fwd writes unit colours (no colors_precomp) and all_map[3] = 1 itself: the compositor derives both sums from T.
    // Image-only forward (unit colours required) when the caller passes neither map.
    const bool unit = colors_precomp == nullptr;
    if (!bucket_tail(s, "view_forward", f, b, cap, P, radii, hints_load(P, width_px, height_px), 1, nullptr, out_all_map != nullptr,
                     unit, unit, background, out_color, out_invdepth, out_all_map, out_color_clamped, out_rend_dir, viewmatrix,
                     slot)) {
        if (checked) slot_abandon(slot);
        return CGS_ERR_HIP;
    }
    if (checked) return mode == 1 ? view_forward_wait(slot, nullptr) : (int64_t)slot;
    return CGS_OK;
}

int cgs_view_forward(int B, int m, const float* curve_points, const float* width, const uint8_t* is_bezier, const float* coef,
                     float eps, double* norms, const float* opacity_logit, const float* mask_logit, float mask_thr,
                     const float* colors_precomp, void* geometry_buffer, void* binning_buffer, size_t binning_bytes,
                     void* image_buffer, uint32_t bucket_capacity, const float* background, int width_px, int height_px,
                     const float* viewmatrix, const float* projmatrix, const float* cam_pos, float tan_fovx, float tan_fovy,
                     float* out_color, float* out_invdepth, float* out_all_map, int* radii, float* xyz, float* rotation,
                     float* scaling, void* stream_) {
    return (int)view_forward_impl(0, B, m, curve_points, width, is_bezier, coef, eps, norms, opacity_logit, mask_logit,
                                  mask_thr, colors_precomp, geometry_buffer, binning_buffer, binning_bytes, image_buffer,
                                  bucket_capacity, background, width_px, height_px, viewmatrix, projmatrix, cam_pos, tan_fovx,
                                  tan_fovy, out_color, out_invdepth, out_all_map, radii, xyz, rotation, scaling, stream_);
}
int64_t cgs_view_forward_checked(int B, int m, const float* curve_points, const float* width, const uint8_t* is_bezier,
                                 const float* coef, float eps, double* norms, const float* opacity_logit,
                                 const float* mask_logit, float mask_thr, const float* colors_precomp, void* geometry_buffer,
                                 void* binning_buffer, size_t binning_bytes, void* image_buffer, uint32_t bucket_capacity,
                                 const float* background, int width_px, int height_px, const float* viewmatrix,
                                 const float* projmatrix, const float* cam_pos, float tan_fovx, float tan_fovy,
                                 float* out_color, float* out_invdepth, float* out_all_map, int* radii, float* xyz,
                                 float* rotation, float* scaling, void* stream_) {
    return view_forward_impl(1, B, m, curve_points, width, is_bezier, coef, eps, norms, opacity_logit, mask_logit, mask_thr,
                             colors_precomp, geometry_buffer, binning_buffer, binning_bytes, image_buffer, bucket_capacity,
                             background, width_px, height_px, viewmatrix, projmatrix, cam_pos, tan_fovx, tan_fovy, out_color,
                             out_invdepth, out_all_map, radii, xyz, rotation, scaling, stream_);
}
int cgs_view_forward_begin(int B, int m, const float* curve_points, const float* width, const uint8_t* is_bezier,
                                 const float* coef, float eps, double* norms, const float* opacity_logit,
                                 const float* mask_logit, float mask_thr, const float* colors_precomp, void* geometry_buffer,
                                 void* binning_buffer, size_t binning_bytes, void* image_buffer, uint32_t bucket_capacity,
                                 const float* background, int width_px, int height_px, const float* viewmatrix,
                                 const float* projmatrix, const float* cam_pos, float tan_fovx, float tan_fovy,
                                 float* out_color, float* out_invdepth, float* out_all_map, int* radii, float* xyz,
                                 float* rotation, float* scaling, void* stream_) {
    return (int)view_forward_impl(2, B, m, curve_points, width, is_bezier, coef, eps, norms, opacity_logit, mask_logit, mask_thr,
                             colors_precomp, geometry_buffer, binning_buffer, binning_bytes, image_buffer, bucket_capacity,
                             background, width_px, height_px, viewmatrix, projmatrix, cam_pos, tan_fovx, tan_fovy, out_color,
                             out_invdepth, out_all_map, radii, xyz, rotation, scaling, stream_);
}
// ... with render()'s epilogue written by the compositor itself (out_color_clamped [H*W], out_rend_dir [3,H*W]; either may be NULL)
int cgs_view_forward_render(int checked, int B, int m, const float* curve_points, const float* width, const uint8_t* is_bezier,
                            const float* coef, float eps, double* norms, const float* opacity_logit, const float* mask_logit,
                            float mask_thr, void* geometry_buffer, void* binning_buffer, size_t binning_bytes, void* image_buffer,
                            uint32_t bucket_capacity, const float* background, int width_px, int height_px, const float* viewmatrix,
                            const float* projmatrix, const float* cam_pos, float tan_fovx, float tan_fovy, float* out_color,
                            float* out_invdepth, float* out_all_map, int* radii, float* out_color_clamped, float* out_rend_dir,
                            void* stream_) {
    return (int)view_forward_impl(checked ? 2 : 0, B, m, curve_points, width, is_bezier, coef, eps, norms, opacity_logit, mask_logit,
                                  mask_thr, nullptr, geometry_buffer, binning_buffer, binning_bytes, image_buffer, bucket_capacity,
                                  background, width_px, height_px, viewmatrix, projmatrix, cam_pos, tan_fovx, tan_fovy, out_color,
                                  out_invdepth, out_all_map, radii, nullptr, nullptr, nullptr, stream_, out_color_clamped,
                                  out_rend_dir);
}
// The two forwards every training route calls, behind the depth gate (include/curvegs.h): the sibling's arguments and checks,
// then the gate's; the launcher picks k_view_fwd<true>, everything behind it is the sibling's.
int cgs_view_forward_depth(int B, int m, const float* curve_points, const float* width, const uint8_t* is_bezier, const float* coef,
                           float eps, double* norms, const float* opacity_logit, const float* mask_logit, float mask_thr,
                           const float* colors_precomp, void* geometry_buffer, void* binning_buffer, size_t binning_bytes,
                           void* image_buffer, uint32_t bucket_capacity, const float* background, int width_px, int height_px,
                           const float* viewmatrix, const float* projmatrix, const float* cam_pos, float tan_fovx, float tan_fovy,
                           float* out_color, float* out_invdepth, float* out_all_map, int* radii, float* xyz, float* rotation,
                           float* scaling, const cgs_view_gate* gate, void* stream_) {
    return (int)view_forward_impl(0, B, m, curve_points, width, is_bezier, coef, eps, norms, opacity_logit, mask_logit,
                                  mask_thr, colors_precomp, geometry_buffer, binning_buffer, binning_bytes, image_buffer,
                                  bucket_capacity, background, width_px, height_px, viewmatrix, projmatrix, cam_pos, tan_fovx,
                                  tan_fovy, out_color, out_invdepth, out_all_map, radii, xyz, rotation, scaling, stream_, nullptr,
                                  nullptr, "cgs_view_forward_depth", gate);
}
int cgs_view_forward_render_depth(int checked, int B, int m, const float* curve_points, const float* width,
                                  const uint8_t* is_bezier, const float* coef, float eps, double* norms,
                                  const float* opacity_logit, const float* mask_logit, float mask_thr, void* geometry_buffer,
                                  void* binning_buffer, size_t binning_bytes, void* image_buffer, uint32_t bucket_capacity,
                                  const float* background, int width_px, int height_px, const float* viewmatrix,
                                  const float* projmatrix, const float* cam_pos, float tan_fovx, float tan_fovy, float* out_color,
                                  float* out_invdepth, float* out_all_map, int* radii, float* out_color_clamped,
                                  float* out_rend_dir, const cgs_view_gate* gate, void* stream_) {
    return (int)view_forward_impl(checked ? 2 : 0, B, m, curve_points, width, is_bezier, coef, eps, norms, opacity_logit, mask_logit,
                                  mask_thr, nullptr, geometry_buffer, binning_buffer, binning_bytes, image_buffer, bucket_capacity,
                                  background, width_px, height_px, viewmatrix, projmatrix, cam_pos, tan_fovx, tan_fovy, out_color,
                                  out_invdepth, out_all_map, radii, nullptr, nullptr, nullptr, stream_, out_color_clamped,
                                  out_rend_dir, "cgs_view_forward_render_depth", gate);
}
int64_t cgs_view_forward_wait(int handle, int64_t* n_visible) { return view_forward_wait(handle, n_visible); }
void cgs_view_forward_abandon(int handle) {
    if (slot_held(handle)) slot_abandon(handle);
}
int cgs_view_forward_shared(int B, int m, const float* curve_points, const float* width, const uint8_t* is_bezier, const float* coef,
                     float eps, double* norms, const float* opacity_logit, const float* mask_logit, float mask_thr,
                     const float* colors_precomp, void* geometry_buffer, void* binning_buffer, size_t binning_bytes,
                     void* image_buffer, uint32_t bucket_capacity, const float* background, int width_px, int height_px,
                     const float* viewmatrix, const float* projmatrix, const float* cam_pos, float tan_fovx, float tan_fovy,
                     float* out_color, float* out_invdepth, float* out_all_map, int* radii, float* xyz, float* rotation,
                     float* scaling, void* stream_) {
    return (int)view_forward_impl(VIEW_MODE_SHARED, B, m, curve_points, width, is_bezier, coef, eps, norms, opacity_logit, mask_logit,
                                  mask_thr, colors_precomp, geometry_buffer, binning_buffer, binning_bytes, image_buffer,
                                  bucket_capacity, background, width_px, height_px, viewmatrix, projmatrix, cam_pos, tan_fovx,
                                  tan_fovy, out_color, out_invdepth, out_all_map, radii, xyz, rotation, scaling, stream_);
}
int64_t cgs_last_forward_visible(void) { return g_last_visible; }
int cgs_visible_indices(int P, const int* radii, const void* image_buffer, int width, int height, int64_t* out_indices, void* stream_) {
    if (P <= 0 || !radii || !image_buffer || width <= 0 || height <= 0 || !out_indices)
        return reject("cgs_visible_indices: invalid argument");
    const Frame f(width, height);
    char* ichunk = (char*)const_cast<void*>(image_buffer);
    ImageState img = image_from_chunk(ichunk, f.npix, (size_t)f.tiles);
    hipLaunchKernelGGL(k_visible_compact, dim3(STAT_BLOCKS), dim3(256), 0, (hipStream_t)stream_, radii, P, img.work + VIS_COUNT_WORD,
                       (long long*)out_indices);
    return finish("visible_indices", stream_);
}
uint32_t cgs_bucket_capacity_hint(int P, int width, int height) {
    const int64_t mx = hints_load(P, width, height).max;
    if (mx <= 0) return 0u;
    return (uint32_t)std::min<uint64_t>(bucket_cap_for(mx), bucket_cap_limit());
}

int cgs_view_norms_backward_range(int* first, int* count) {
    if (first) *first = sample_norm_fwd_words();
    if (count) *count = sample_norm_words() - sample_norm_fwd_words();
    return 384;
}
// 13 floats per curve are used (16 asked for: the size stays a multiple of 64 bytes); rounds 2-5: 15 per splat
size_t cgs_view_backward_scratch_floats(int B, int m) { (void)m; return (size_t)(B > 0 ? B : 0) * 16; }

int cgs_view_backward(int B, int m, const float* curve_points, const float* width, const uint8_t* is_bezier, const float* coef,
                      float eps, double* norms, const float* opacity_logit, const float* mask_logit, float mask_thr,
                      const float* colors_precomp, void* geometry_buffer, const void* binning_buffer, const void* image_buffer, const float* background,
                      int width_px, int height_px, const float* viewmatrix, const float* projmatrix, const float* cam_pos,
                      float tan_fovx, float tan_fovy, const int* radii, const float* dL_dout_color,
                      const float* dL_drotation_extra, float* dL_dmeans2D, float* dL_dcurve_points, float* dL_dwidth,
                      float* dL_dopacity_logit, float* dL_dmask_logit, float* scratch, int flags, void* stream_) {
    return view_backward_impl(B, m, curve_points, width, is_bezier, coef, eps, norms, opacity_logit, mask_logit, mask_thr, colors_precomp,
                              geometry_buffer, binning_buffer, image_buffer, background, width_px, height_px, viewmatrix, projmatrix,
                              cam_pos, tan_fovx, tan_fovy, radii, dL_dout_color, dL_drotation_extra, dL_dmeans2D, dL_dcurve_points,
                              dL_dwidth, dL_dopacity_logit, dL_dmask_logit, scratch, flags, stream_, nullptr);
}
// ... for an image that went through render()'s clamp: dL_dout_color is the gradient of the CLAMPED image and color_raw the
// forward's unclamped one; torch.clamp's gradient mask is applied where the compositor loads the pixel's upstream gradient
int cgs_view_backward_render(int B, int m, const float* curve_points, const float* width, const uint8_t* is_bezier, const float* coef,
                      float eps, double* norms, const float* opacity_logit, const float* mask_logit, float mask_thr,
                      void* geometry_buffer, const void* binning_buffer, const void* image_buffer, const float* background,
                      int width_px, int height_px, const float* viewmatrix, const float* projmatrix, const float* cam_pos,
                      float tan_fovx, float tan_fovy, const int* radii, const float* dL_dout_color, const float* color_raw,
                      float* dL_dmeans2D, float* dL_dcurve_points, float* dL_dwidth,
                      float* dL_dopacity_logit, float* dL_dmask_logit, float* scratch, int flags, void* stream_) {
    return view_backward_impl(B, m, curve_points, width, is_bezier, coef, eps, norms, opacity_logit, mask_logit, mask_thr, nullptr,
                              geometry_buffer, binning_buffer, image_buffer, background, width_px, height_px, viewmatrix, projmatrix,
                              cam_pos, tan_fovx, tan_fovy, radii, dL_dout_color, nullptr, dL_dmeans2D, dL_dcurve_points,
                              dL_dwidth, dL_dopacity_logit, dL_dmask_logit, scratch, flags, stream_, color_raw);
}

int cgs_view_shared_begin(int B, int m, const float* curve_points, const uint8_t* is_bezier, const float* coef, double* norms,
                          float* scratch, void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    if (B <= 0 || m <= 0 || m > 32 || !curve_points || !coef || !norms || !scratch || !aligned16(curve_points) || !aligned16(coef))
        return reject("cgs_view_shared_begin: invalid argument");
    if (!zeroed(scratch, cgs_view_backward_scratch_floats(B, m) * sizeof(float), s, "zero_async failed")) return CGS_ERR_HIP;
    launch_sample_norms(s, B, m, curve_points, is_bezier, coef, norms);
    return finish("view_shared_begin", s);
}
int cgs_view_shared_end(int B, int m, const float* curve_points, const float* width, const uint8_t* is_bezier, const float* coef,
                        float eps, double* norms, float* scratch, float* dL_dcurve_points, float* dL_dwidth, int accumulate,
                        void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    if (B <= 0 || m <= 0 || m > 32 || !curve_points || !width || !coef || !norms || !scratch || !dL_dcurve_points || !dL_dwidth ||
        !aligned16(curve_points) || !aligned16(coef) || !aligned16(dL_dcurve_points))
        return reject("cgs_view_shared_end: invalid argument");
    launch_sample_backward_close(s, B, m, curve_points, width, is_bezier, coef, eps, norms, scratch, dL_dcurve_points, dL_dwidth,
                                 accumulate);
    return finish("view_shared_end", s);
}

int cgs_sample_curves_backward(int B, int m, const float* curve_points, const float* width, const uint8_t* is_bezier,
                               const float* coef, float eps, double* norms, const float* dL_dxyz,
                               const float* dL_drotation, const float* dL_dscaling, float* dL_dcurve_points,
                               float* dL_dwidth, float* scratch, void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    if (B == 0) return CGS_OK;
    if (B < 0 || m <= 0 || m > 32 || !curve_points || !width || !coef || !norms || !dL_dcurve_points || !dL_dwidth ||
        (dL_drotation && !scratch) ||
        !aligned16(curve_points) || !aligned16(dL_drotation) || !aligned16(dL_dcurve_points) || !aligned16(coef))
        return reject("cgs_sample_curves_backward: invalid argument");
    // (a second backward over the same forward -- retain_graph -- must not see the first one's two sums)
    if (!zeroed(norms + sample_norm_fwd_words(), (size_t)(sample_norm_words() - sample_norm_fwd_words()) * sizeof(double), s,
                "zero_async(norms) failed"))
        return CGS_ERR_HIP;
    launch_sample_backward(s, B, m, curve_points, width, is_bezier, coef, eps, norms, dL_dxyz, dL_drotation, dL_dscaling,
                           dL_dcurve_points, dL_dwidth, scratch);
    return finish("sample_curves_backward", s);
}

int cgs_splat_attrs_forward(int B, int m, const float* rotation_raw, const float* xyz, const float* opacity_logit,
                            const float* mask_logit, float mask_thr, const float* scaling, const float* campos,
                            const float* viewmatrix, float* rotation_n, float* opacity, float* scaling_out,
                            float* all_map, void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    if (B == 0) return CGS_OK;
    if (B < 0 || m <= 0 || !rotation_raw || !xyz || !opacity_logit || !campos || !viewmatrix || !rotation_n || !opacity ||
        !all_map || (scaling_out && !scaling) || !aligned16(rotation_raw) || !aligned16(rotation_n) || !aligned16(all_map))
        return reject("cgs_splat_attrs_forward: invalid argument");
    launch_attrs_forward(s, B, m, rotation_raw, xyz, opacity_logit, mask_logit, mask_thr, scaling, campos, viewmatrix,
                         rotation_n, opacity, scaling_out, all_map);
    return finish("splat_attrs_forward", s);
}

int cgs_splat_attrs_backward(int B, int m, const float* rotation_raw, const float* xyz, const float* opacity_logit,
                             const float* mask_logit, float mask_thr, const float* scaling, const float* campos,
                             const float* viewmatrix, const float* dL_drotation_n, const float* dL_dopacity,
                             const float* dL_dscaling_out, const float* dL_dall_map, float* dL_drotation_raw,
                             float* dL_dopacity_logit, float* dL_dmask_logit, float* dL_dscaling, void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    if (B == 0) return CGS_OK;
    if (B < 0 || m <= 0 || !rotation_raw || !xyz || !opacity_logit || !campos || !viewmatrix || !dL_drotation_raw ||
        !dL_dopacity_logit || !aligned16(rotation_raw) || !aligned16(dL_drotation_n) || !aligned16(dL_dall_map) ||
        !aligned16(dL_drotation_raw))
        return reject("cgs_splat_attrs_backward: invalid argument");
    launch_attrs_backward(s, B, m, rotation_raw, xyz, opacity_logit, mask_logit, mask_thr, scaling, campos, viewmatrix,
                          dL_drotation_n, dL_dopacity, dL_dscaling_out, dL_dall_map, dL_drotation_raw, dL_dopacity_logit,
                          dL_dmask_logit, dL_dscaling);
    return finish("splat_attrs_backward", s);
}


int cgs_ssim_forward(int batch, int channels, int height, int width, float C1, float C2, const float* img1,
                     const float* img2, float* ssim_map, float* dm_dmu1, float* dm_dsigma1_sq, float* dm_dsigma12,
                     void* stream_) {
    if (batch * channels == 0 || height == 0 || width == 0) return CGS_OK;
    if (batch < 0 || channels < 0 || height < 0 || width < 0 || !img1 || !img2 || !ssim_map ||
        (dm_dmu1 && (!dm_dsigma1_sq || !dm_dsigma12)) || (long long)batch * channels > 65535)
        return reject("cgs_ssim_forward: invalid argument");
    launch_ssim_fwd((hipStream_t)stream_, batch * channels, height, width, C1, C2, img1, img2, ssim_map, dm_dmu1,
                    dm_dsigma1_sq, dm_dsigma12);
    return finish("ssim_forward", stream_);
}

int cgs_ssim_backward(int batch, int channels, int height, int width, float C1, float C2, const float* img1,
                      const float* img2, const float* dL_dmap, const float* dm_dmu1, const float* dm_dsigma1_sq,
                      const float* dm_dsigma12, float* dL_dimg1, void* stream_) {
    (void)C1;
    (void)C2;
    if (batch * channels == 0 || height == 0 || width == 0) return CGS_OK;
    if (batch < 0 || channels < 0 || height < 0 || width < 0 || !img1 || !img2 || !dL_dmap || !dm_dmu1 ||
        !dm_dsigma1_sq || !dm_dsigma12 || !dL_dimg1 || (long long)batch * channels > 65535)
        return reject("cgs_ssim_backward: invalid argument");
    launch_ssim_bwd((hipStream_t)stream_, batch * channels, height, width, img1, img2, dL_dmap, dm_dmu1, dm_dsigma1_sq,
                    dm_dsigma12, dL_dimg1);
    return finish("ssim_backward", stream_);
}

int cgs_edge_aware_loss(int channels, int height, int width, const float* image, const float* gt, float threshold,
                        void* scratch16, float* dL_dimage, void* stream_) {
    hipStream_t s = (hipStream_t)stream_;
    if (channels <= 0 || height <= 0 || width <= 0 || !image || !gt || !scratch16)
        return reject("cgs_edge_aware_loss: invalid argument");
    if (!zeroed(scratch16, 16, s, "zero_async failed")) return CGS_ERR_HIP;
    launch_edge_aware_loss(s, channels, height, width, image, gt, threshold, scratch16, dL_dimage);
    return finish("edge_aware_loss", s);
}

size_t cgs_photometric_workspace_bytes(int height, int width) {
    return photometric_workspace_bytes(height > 0 ? height : 1, width > 0 ? width : 1);
}
int cgs_render_epilogue(int height, int width, const float* color_raw, const float* all_map, const float* viewmatrix, int clamp,
                        float* color_out, float* dir_out, void* stream_) {
    if (height <= 0 || width <= 0 || (color_out && !color_raw) || (dir_out && (!all_map || !viewmatrix)))
        return reject("cgs_render_epilogue: invalid argument");
    if (!color_out && !dir_out) return CGS_OK;
    launch_render_epilogue((hipStream_t)stream_, (size_t)height * width, color_raw, all_map, viewmatrix, clamp, color_out, dir_out);
    return finish("render_epilogue", stream_);
}
int cgs_clamp_backward(int64_t n, const float* raw, const float* g_in, float* g_out, void* stream_) {
    if (n < 0 || (n > 0 && (!raw || !g_in || !g_out))) return reject("cgs_clamp_backward: invalid argument");
    if (n == 0) return CGS_OK;
    hipLaunchKernelGGL(k_clamp_backward, dim3((unsigned)std::min<size_t>(((size_t)n + 255) / 256, 4096)), dim3(256), 0, (hipStream_t)stream_,
                       (size_t)n, raw, g_in, g_out);
    return finish("clamp_backward", stream_);
}

int cgs_edge_count(int channels, int height, int width, const float* gt, float threshold, uint32_t* n_pos, void* stream_) {
    if (channels <= 0 || height <= 0 || width <= 0 || !gt || !n_pos) return reject("cgs_edge_count: invalid argument");
    hipStream_t s = (hipStream_t)stream_;
    if (!zeroed(n_pos, sizeof(uint32_t), s, "cgs_edge_count: zero_async failed")) return CGS_ERR_HIP;
    launch_edge_count(s, channels, height * width, gt, threshold, n_pos);
    return finish("edge_count", s);
}
// cgs_photometric_loss (the view's own target and edge count: no view_index) and cgs_photometric_loss_indexed, as `name`
static int photometric_loss(const char* name, int height, int width, const float* image, const float* gt, const int* view_index,
                            float threshold, const uint32_t* n_pos, float lambda_edge, float lambda_ssim, int clamp_input,
                            void* workspace, float* dL_dimage, float* loss, void* stream_) {
    if (height <= 0 || width <= 0 || !image || !gt || !n_pos || !workspace || !dL_dimage || !loss)
        return reject("cgs_%s: invalid argument", name);
    launch_photometric_loss((hipStream_t)stream_, height, width, image, gt, view_index, threshold, n_pos, lambda_edge, lambda_ssim,
                            clamp_input, workspace, dL_dimage, loss);
    return finish(name, stream_);
}
int cgs_photometric_loss(int height, int width, const float* image, const float* gt, float threshold,
                         const uint32_t* n_pos, float lambda_edge, float lambda_ssim, int clamp_input, void* workspace,
                         float* dL_dimage, float* loss, void* stream_) {
    return photometric_loss("photometric_loss", height, width, image, gt, nullptr, threshold, n_pos, lambda_edge, lambda_ssim,
                            clamp_input, workspace, dL_dimage, loss, stream_);
}
int cgs_photometric_loss_indexed(int height, int width, const float* image, const float* gt_stack, const int* view_index,
                                 float threshold, const uint32_t* n_pos_table, float lambda_edge, float lambda_ssim,
                                 int clamp_input, void* workspace, float* dL_dimage, float* loss, void* stream_) {
    if (!view_index) return reject("cgs_photometric_loss_indexed: invalid argument");
    return photometric_loss("photometric_loss_indexed", height, width, image, gt_stack, view_index, threshold, n_pos_table,
                            lambda_edge, lambda_ssim, clamp_input, workspace, dL_dimage, loss, stream_);
}

size_t cgs_curve_regularizers_workspace_bytes(void) { return curve_reg_workspace_bytes(); }
int cgs_curve_regularizers(int B, int m, const float* rotation_raw, const float* opacity_logit, const float* width_log,
                           const int* radii, float w_opacity, const float* opacity_gate, float w_smooth, float w_width,
                           float width_threshold, void* workspace, float* loss, float* dL_drotation_raw,
                           float* dL_dopacity_logit, float* dL_dwidth_log, void* stream_) {
    if (B <= 0 || m < 2 || m > 32 || 256 / m < 1 || !rotation_raw || !opacity_logit || !width_log || !radii || !workspace ||
        !loss || !dL_drotation_raw || !dL_dopacity_logit || !dL_dwidth_log || !aligned16(rotation_raw) ||
        !aligned16(dL_drotation_raw))
        return reject("cgs_curve_regularizers: invalid argument (NULL / misaligned pointer, B=%d m=%d)", B, m);
    hipStream_t s = (hipStream_t)stream_;
    launch_curve_regularizers(s, B, m, rotation_raw, opacity_logit, width_log, radii, w_opacity, opacity_gate, w_smooth,
                              w_width, width_threshold, workspace, loss, dL_drotation_raw, dL_dopacity_logit,
                              dL_dwidth_log);
    return finish("curve_regularizers", s);
}

int cgs_adam_step_flat(int64_t n, float* params, float* grads, float* exp_avg, float* exp_avg_sq,
                       const void* segments, int n_segments, float beta1, float beta2, float eps, int step,
                       int zero_grads, void* stream_) {
    if (n == 0) return CGS_OK;
    if (n < 0 || !params || !grads || !exp_avg || !exp_avg_sq || !segments || n_segments <= 0 ||
        n_segments > adam_max_segments() || step <= 0)
        return reject("cgs_adam_step_flat: invalid argument");
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    launch_adam_flat((hipStream_t)stream_, (long long)n, params, grads, exp_avg, exp_avg_sq, segments, n_segments, beta1,
                     beta2, eps, (float)bc1, (float)sqrt(bc2), zero_grads);
    return finish("adam_step_flat", stream_);
}

// The two device-state Adam entries, as `name` (without a report: NULL, NULL, 0, launch_adam_flat_dev's own defaults)
static int adam_step_flat_dev(const char* name, int64_t n, float* params, float* grads, float* exp_avg, float* exp_avg_sq,
                              const void* device_state, int n_segments, float beta1, float beta2, float eps, int zero_grads,
                              const uint32_t* skip_flag, uint32_t* report_seq, uint32_t* report_ring, int report_len,
                              void* stream_) {
    if (n == 0) return CGS_OK;
    if (n < 0 || !params || !grads || !exp_avg || !exp_avg_sq || !device_state || n_segments <= 0 ||
        n_segments > adam_max_segments())
        return reject("cgs_%s: invalid argument", name);
    launch_adam_flat_dev((hipStream_t)stream_, (long long)n, params, grads, exp_avg, exp_avg_sq, device_state, n_segments,
                         beta1, beta2, eps, zero_grads, skip_flag, report_seq, report_ring, report_len);
    return finish(name, stream_);
}
int cgs_adam_step_flat_dev(int64_t n, float* params, float* grads, float* exp_avg, float* exp_avg_sq,
                           const void* device_state, int n_segments, float beta1, float beta2, float eps, int zero_grads,
                           const uint32_t* skip_flag, void* stream_) {
    return adam_step_flat_dev("adam_step_flat_dev", n, params, grads, exp_avg, exp_avg_sq, device_state, n_segments, beta1, beta2,
                              eps, zero_grads, skip_flag, nullptr, nullptr, 0, stream_);
}
int cgs_adam_step_flat_dev_report(int64_t n, float* params, float* grads, float* exp_avg, float* exp_avg_sq,
                                  const void* device_state, int n_segments, float beta1, float beta2, float eps, int zero_grads,
                                  const uint32_t* skip_flag, uint32_t* report_seq, uint32_t* report_ring, int report_len,
                                  void* stream_) {
    if (n != 0 && (!report_seq || !report_ring || report_len <= 0))   // (an empty step needs no report)
        return reject("cgs_adam_step_flat_dev_report: invalid argument");
    return adam_step_flat_dev("adam_step_flat_dev_report", n, params, grads, exp_avg, exp_avg_sq, device_state, n_segments, beta1,
                              beta2, eps, zero_grads, skip_flag, report_seq, report_ring, report_len, stream_);
}
size_t cgs_endpoint_connection_workspace_bytes(int B) { return endpoint_connection_workspace_bytes(B > 0 ? B : 1); }
int cgs_endpoint_connection_loss(int B, const float* curve_points, float distance_threshold, float weight, void* workspace,
                                 float* loss, float* dL_dcurve_points, int accumulate, void* stream_) {
    if (B <= 0 || !curve_points || !workspace || !loss || !dL_dcurve_points || !(distance_threshold > 0.f))
        return reject("cgs_endpoint_connection_loss: invalid argument (NULL pointer, B=%d or threshold <= 0)", B);
    hipStream_t s = (hipStream_t)stream_;
    launch_endpoint_connection(s, B, curve_points, distance_threshold, weight, workspace, loss, dL_dcurve_points, accumulate);
    return finish("endpoint_connection_loss", s);
}

size_t cgs_adam_state_bytes(void) { return adam_state_bytes(); }

size_t cgs_knn_workspace_bytes(int P) { return knn_workspace_bytes(P); }

int cgs_knn_mean_dist2(int P, const float* points, float* mean_dist2, void* workspace, void* stream_) {
    if (P == 0) return CGS_OK;
    if (P < 0 || !points || !mean_dist2 || !workspace) return reject("cgs_knn_mean_dist2: invalid argument");
    launch_knn((hipStream_t)stream_, P, points, mean_dist2, workspace);
    return finish("knn_mean_dist2", stream_);
}

size_t cgs_nn1_workspace_bytes(int n_query) { return nn1_workspace_bytes(n_query); }

int cgs_nn1(int n_query, const float* query, int n_ref, const float* ref, float* dist, int* index, void* workspace,
            void* stream_) {
    if (n_query < 0 || n_ref < 0 || n_query > (1 << 30) || n_ref > (1 << 30))
        return reject("cgs_nn1: invalid argument (n_query=%d, n_ref=%d)", n_query, n_ref);
    if (n_query == 0) return CGS_OK;
    if (n_ref == 0 || !query || !ref || !dist || !index || !workspace)
        return reject("cgs_nn1: invalid argument (NULL pointer or an empty reference set, n_ref=%d)", n_ref);
    launch_nn1((hipStream_t)stream_, n_query, query, n_ref, ref, dist, index, workspace);
    return finish("nn1", stream_);
}

// The slack comes right after the counts, the depth pointer among the pointers of the frames.
static int edge_visibility_entry(const char* name, int n_curves, const double* curves, int n_lines, const double* lines,
                                 int n_frames, const double* K, const double* w2c, int height, int width,
                                 const unsigned char* maps, int invert, const DepthGate* gate, int* counts, void* stream_) {
    if (n_curves < 0 || n_lines < 0 || n_frames < 0 || (long long)n_curves + n_lines > (1 << 30))
        return reject("%s: invalid argument (n_curves=%d, n_lines=%d, n_frames=%d)", name, n_curves, n_lines, n_frames);
    if (slack_bad(gate)) return reject_slack(name, gate);
    if (n_curves + n_lines == 0) return CGS_OK;
    if (n_frames > 0 && (height <= 0 || width <= 0))
        return reject("%s: invalid argument (height=%d, width=%d)", name, height, width);
    if ((n_curves > 0 && !curves) || (n_lines > 0 && !lines) || !counts ||
        (n_frames > 0 && (!K || !w2c || !maps || depth_missing(gate))))
        return reject("%s: invalid argument (NULL pointer)", name);
    launch_edge_visibility((hipStream_t)stream_, n_curves, curves, n_lines, lines, n_frames, K, w2c, height, width, maps,
                           invert, gate, counts);
    return finish(name + 4, stream_);   // the label is the entry's name without its cgs_
}

int cgs_edge_visibility(int n_curves, const double* curves, int n_lines, const double* lines, int n_frames,
                        const double* K, const double* w2c, int height, int width, const unsigned char* maps,
                        int invert, int* counts, void* stream_) {
    return edge_visibility_entry("cgs_edge_visibility", n_curves, curves, n_lines, lines, n_frames, K, w2c, height, width,
                                 maps, invert, nullptr, counts, stream_);
}

int cgs_edge_visibility_depth(int n_curves, const double* curves, int n_lines, const double* lines, int n_frames,
                              const double* K, const double* w2c, int height, int width, const unsigned char* maps,
                              int invert, const float* depth, double slack, int32_t* counts_out, void* stream_) {
    const DepthGate gate{depth, slack};
    return edge_visibility_entry("cgs_edge_visibility_depth", n_curves, curves, n_lines, lines, n_frames, K, w2c, height,
                                 width, maps, invert, &gate, counts_out, stream_);
}

int cgs_densification_stats(int64_t P, const int* radii, const float* dL_dmeans2D, int64_t grad_stride, float* max_radii2D,
                            float* xyz_gradient_accum, float* denom, const uint32_t* skip_flag, void* stream_) {
    if (P < 0 || grad_stride < 2)
        return reject("cgs_densification_stats: invalid argument (P=%lld, grad_stride=%lld)", (long long)P,
                      (long long)grad_stride);
    if (P == 0) return CGS_OK;
    if (!radii || !dL_dmeans2D || !max_radii2D || !xyz_gradient_accum || !denom)
        return reject("cgs_densification_stats: invalid argument (NULL pointer)");
    launch_densification_stats((hipStream_t)stream_, (long long)P, radii, dL_dmeans2D, (long long)grad_stride, max_radii2D,
                               xyz_gradient_accum, denom, skip_flag);
    return finish("densification_stats", stream_);
}

size_t cgs_view_metrics_workspace_bytes(int n_views) { return view_metrics_workspace_bytes(n_views); }

int cgs_view_metrics(int n_views, const cgs_metric_view* views, void* workspace, double* sums, double* means,
                     void* stream_) {
    if (n_views < 0 || n_views > 65535) return reject("cgs_view_metrics: invalid argument (n_views=%d)", n_views);
    if (n_views == 0) return CGS_OK;
    if (!views || !workspace || !sums) return reject("cgs_view_metrics: invalid argument (NULL pointer)");
    for (int v = 0; v < n_views; v++) {
        const cgs_metric_view& d = views[v];
        if (!d.image || !d.gt) return reject("cgs_view_metrics: invalid argument (view %d: NULL pointer)", v);
        if (d.channels <= 0 || d.height <= 0 || d.width <= 0 || d.x0 < 0 || d.x0 >= d.width)
            return reject("cgs_view_metrics: invalid argument (view %d: channels=%d, height=%d, width=%d, x0=%d)", v,
                          d.channels, d.height, d.width, d.x0);
    }
    if (launch_view_metrics((hipStream_t)stream_, n_views, views, workspace, sums, means) != hipSuccess) {
        set_error("cgs_view_metrics: descriptor copy failed");
        return CGS_ERR_HIP;
    }
    return finish("view_metrics", stream_);
}

size_t cgs_report_panels_workspace_bytes(int n_views) { return report_panels_workspace_bytes(n_views); }

int cgs_report_panels(int n_views, cgs_report_view* views, void* workspace, unsigned char* out, void* stream_) {
    if (n_views < 0 || n_views > CGS_REPORT_MAX_VIEWS)
        return reject("cgs_report_panels: invalid argument (n_views=%d, at most %d per call)", n_views, CGS_REPORT_MAX_VIEWS);
    if (n_views == 0) return CGS_OK;
    if (!views || !workspace || !out) return reject("cgs_report_panels: invalid argument (NULL pointer)");
    for (int v = 0; v < n_views; v++) {
        const cgs_report_view& d = views[v];
        if (d.height <= 0 || d.width <= 0 || (d.gt && d.gt_channels != 1 && d.gt_channels != 3))
            return reject("cgs_report_panels: invalid argument (view %d: gt_channels=%d, height=%d, width=%d)", v,
                          d.gt_channels, d.height, d.width);
        const size_t bytes = (size_t)CGS_REPORT_PANELS * 3 * (size_t)d.height * (size_t)d.width;
        for (int u = 0; u < v; u++) {
            const size_t other = (size_t)CGS_REPORT_PANELS * 3 * (size_t)views[u].height * (size_t)views[u].width;
            if (d.out_offset < views[u].out_offset + other && views[u].out_offset < d.out_offset + bytes)
                return reject("cgs_report_panels: invalid argument (the output ranges of views %d and %d overlap)", u, v);
        }
    }
    for (int v = 0; v < n_views; v++) {
        cgs_report_view& d = views[v];
        d.written = (d.render ? 1u : 0u) | (d.gt ? 2u : 0u) | (d.depth ? 4u : 0u) | (d.rend_dir ? 8u : 0u) |
                    (d.rend_alpha ? 16u : 0u);
    }
    launch_report_panels((hipStream_t)stream_, n_views, views, workspace, out);
    return finish("report_panels", stream_);
}

// The drawn views: the slack comes right after the counts (and the sizes, where they are checked with the counts).
static int project_points_entry(const char* name, int P, const float* points, int V, const double* intr, const double* w2c,
                                int height, int width, const DepthGate* gate, double* uv_out, uint8_t* hidden_out,
                                void* stream_) {
    if (P < 0 || V < 0 || (long long)P * V > (1LL << 40)) return reject("%s: invalid argument (P=%d, V=%d)", name, P, V);
    if (slack_bad(gate)) return reject_slack(name, gate);
    if (P == 0 || V == 0) return CGS_OK;
    if (height <= 0 || width <= 0) return reject("%s: invalid argument (height=%d, width=%d)", name, height, width);
    if (!points || !intr || !w2c || depth_missing(gate) || !uv_out) return reject("%s: invalid argument (NULL pointer)", name);
    launch_project_points((hipStream_t)stream_, P, points, V, intr, w2c, height, width, gate, uv_out, hidden_out);
    return finish(name + 4, stream_);
}

int cgs_project_points(int P, const float* points, int V, const double* intr, const double* w2c, int height, int width,
                       double* uv_out, void* stream_) {
    return project_points_entry("cgs_project_points", P, points, V, intr, w2c, height, width, nullptr, uv_out, nullptr,
                                stream_);
}

int cgs_project_points_depth(int P, const float* points, int V, const double* intr, const double* w2c, int height, int width,
                             const float* depth, double slack, double* uv_out, uint8_t* hidden_out, void* stream_) {
    const DepthGate gate{depth, slack};
    return project_points_entry("cgs_project_points_depth", P, points, V, intr, w2c, height, width, &gate, uv_out, hidden_out,
                                stream_);
}

size_t cgs_render_points_workspace_bytes(int P, int V, int height, int width) {
    return render_points_workspace_bytes(P, V, height, width);
}

static int render_points_entry(const char* name, int P, const float* points, const float* colors, int V, const double* intr,
                               const double* w2c, int height, int width, const DepthGate* gate, double alpha,
                               const double* background, float* out, int* kept, int* hidden, void* workspace,
                               size_t workspace_bytes, void* stream_) {
    if (P < 0 || V < 0 || height <= 0 || width <= 0 || (long long)height * width > (1LL << 31))
        return reject("%s: invalid argument (P=%d, V=%d, height=%d, width=%d)", name, P, V, height, width);
    if (slack_bad(gate)) return reject_slack(name, gate);
    if (!(alpha >= 0.0 && alpha <= 1.0)) return reject("%s: invalid argument (alpha=%g, need 0 <= alpha <= 1)", name, alpha);
    if (V == 0) return CGS_OK;
    if (!intr || !w2c || depth_missing(gate) || !background || !out || !workspace || (P > 0 && (!points || !colors)))
        return reject("%s: invalid argument (NULL pointer)", name);
    const int per = render_points_views_per_chunk(P, V, height, width, workspace_bytes);
    if (per <= 0)
        return reject("%s: invalid argument (workspace of %zu bytes holds no view; one view needs %zu)", name, workspace_bytes,
                      render_points_workspace_bytes(P, 1, height, width));
    launch_render_points((hipStream_t)stream_, P, points, colors, V, intr, w2c, height, width, gate, alpha, background, out,
                         kept, hidden, workspace, per);
    return finish(name + 4, stream_);
}

int cgs_render_points(int P, const float* points, const float* colors, int V, const double* intr, const double* w2c,
                      int height, int width, double alpha, const double* background, float* out, int* kept,
                      void* workspace, size_t workspace_bytes, void* stream_) {
    return render_points_entry("cgs_render_points", P, points, colors, V, intr, w2c, height, width, nullptr, alpha, background,
                               out, kept, nullptr, workspace, workspace_bytes, stream_);
}

int cgs_render_points_depth(int P, const float* points, const float* colors, int V, const double* intr, const double* w2c,
                            int height, int width, const float* depth, double slack, double alpha, const double* background,
                            float* out, int* kept, int* hidden, void* workspace, size_t workspace_bytes, void* stream_) {
    const DepthGate gate{depth, slack};
    return render_points_entry("cgs_render_points_depth", P, points, colors, V, intr, w2c, height, width, &gate, alpha,
                               background, out, kept, hidden, workspace, workspace_bytes, stream_);
}

int64_t cgs_ellipsoid_mesh_body_bytes(int P, int resolution, int64_t* vertex_bytes, int64_t* face_bytes) {
    if (P < 0 || resolution < 2 || resolution > 1024) {
        set_error("cgs_ellipsoid_mesh_body_bytes: invalid argument (P=%d, resolution=%d)", P, resolution);
        return -1;
    }
    const long long V0 = 2 + 2LL * resolution * (resolution - 1), F0 = 4LL * resolution * (resolution - 1);
    if ((long long)P * V0 > (1LL << 31)) {
        set_error("cgs_ellipsoid_mesh_body_bytes: %d splats of %lld vertices: a vertex index would not fit in an int", P,
                  V0);
        return -1;
    }
    const int64_t vb = (int64_t)P * V0 * 27, fb = (int64_t)P * F0 * 13;
    if (vertex_bytes) *vertex_bytes = vb;
    if (face_bytes) *face_bytes = fb;
    return vb + fb;
}

int cgs_ellipsoid_mesh_vertices(int first, int count, const float* xyz, const float* rot, const float* scale,
                                const float* rgb, int V0, const double* unit_vertices, void* out, void* stream_) {
    if (first < 0 || count < 0 || V0 <= 0 || (long long)(first + (long long)count) * V0 > (1LL << 31))
        return reject("cgs_ellipsoid_mesh_vertices: invalid argument (first=%d, count=%d, V0=%d)", first, count, V0);
    if (count == 0) return CGS_OK;
    if (!xyz || !rot || !scale || !rgb || !unit_vertices || !out)
        return reject("cgs_ellipsoid_mesh_vertices: invalid argument (NULL pointer)");
    if ((uintptr_t)out % 16) return reject("cgs_ellipsoid_mesh_vertices: out must be 16-byte aligned");
    launch_ellipsoid_vertices((hipStream_t)stream_, first, count, xyz, rot, scale, rgb, V0, unit_vertices, out);
    return finish("ellipsoid_mesh_vertices", stream_);
}

int cgs_ellipsoid_mesh_faces(int first, int count, int V0, int F0, const int* template_faces, void* out, void* stream_) {
    if (first < 0 || count < 0 || V0 <= 0 || F0 <= 0)
        return reject("cgs_ellipsoid_mesh_faces: invalid argument (first=%d, count=%d, V0=%d, F0=%d)", first, count, V0, F0);
    if ((long long)(first + (long long)count) * V0 > (1LL << 31))
        return reject("cgs_ellipsoid_mesh_faces: splats [%d, %d) of %d vertices: a vertex index would not fit in an int",
                      first, first + count, V0);
    if (count == 0) return CGS_OK;
    if (!template_faces || !out) return reject("cgs_ellipsoid_mesh_faces: invalid argument (NULL pointer)");
    if ((uintptr_t)out % 16) return reject("cgs_ellipsoid_mesh_faces: out must be 16-byte aligned");
    launch_ellipsoid_faces((hipStream_t)stream_, first, count, V0, F0, template_faces, out);
    return finish("ellipsoid_mesh_faces", stream_);
}

int cgs_curve_straightness(int B, const float* curve_points, const uint8_t* is_bezier, int sample_num, double threshold,
                           double threshold_max, double* mean_dist, double* max_dist, uint8_t* straight, void* stream_) {
    if (B < 0 || B > (1 << 24) || sample_num < 2 || sample_num > CGS_CURVE_FIT_MAX_SAMPLES)
        return reject("cgs_curve_straightness: invalid argument (B=%d, sample_num=%d, need 2 <= sample_num <= %d)", B,
                      sample_num, CGS_CURVE_FIT_MAX_SAMPLES);
    if (threshold != threshold || threshold_max != threshold_max)
        return reject("cgs_curve_straightness: invalid argument (a threshold is NaN)");
    if (B == 0) return CGS_OK;
    if (!curve_points || !is_bezier || !mean_dist || !max_dist || !straight)
        return reject("cgs_curve_straightness: invalid argument (NULL pointer)");
    launch_curve_straightness((hipStream_t)stream_, B, curve_points, is_bezier, sample_num, threshold, threshold_max,
                              mean_dist, max_dist, straight);
    return finish("curve_straightness", stream_);
}

size_t cgs_segment_merge_workspace_bytes(int n) { return segment_merge_workspace_bytes(n); }

int cgs_segment_merge_labels(int n, const float* seg, double distance_threshold, double similarity_threshold,
                             void* workspace, int* labels, int* n_components, void* stream_) {
    if (n < 0 || n > CGS_SEGMENT_MERGE_MAX)
        return reject("cgs_segment_merge_labels: invalid argument (n=%d, need 0 <= n <= %d)", n, CGS_SEGMENT_MERGE_MAX);
    if (distance_threshold != distance_threshold || similarity_threshold != similarity_threshold)
        return reject("cgs_segment_merge_labels: invalid argument (a threshold is NaN)");
    if (!n_components || (n > 0 && (!seg || !workspace || !labels)))
        return reject("cgs_segment_merge_labels: invalid argument (NULL pointer)");
    if (n == 0) {
        if (hipMemsetAsync(n_components, 0, sizeof(int), (hipStream_t)stream_) != hipSuccess) {
            set_error("cgs_segment_merge_labels: hipMemsetAsync failed");
            return CGS_ERR_HIP;
        }
        return CGS_OK;
    }
    launch_segment_merge_labels((hipStream_t)stream_, n, seg, distance_threshold, similarity_threshold, workspace, labels,
                                n_components);
    return finish("segment_merge_labels", stream_);
}

int cgs_pair_consensus_fit(int B, const float* curve_points, int K, const int* pairs, int sample_num, double ransac_thresh,
                           double error_threshold, float* ctrl, double* rmse, int* inliers, uint8_t* ok, void* stream_) {
    if (B < 0 || K < 0 || B > (1 << 24) || K > (1 << 24) || sample_num < 2 || sample_num > CGS_CURVE_FIT_MAX_SAMPLES)
        return reject("cgs_pair_consensus_fit: invalid argument (B=%d, K=%d, sample_num=%d, need 2 <= sample_num <= %d)", B, K,
                      sample_num, CGS_CURVE_FIT_MAX_SAMPLES);
    if (ransac_thresh != ransac_thresh || error_threshold != error_threshold)
        return reject("cgs_pair_consensus_fit: invalid argument (a threshold is NaN)");
    if (K == 0) return CGS_OK;
    if (B == 0 || !curve_points || !pairs || !ctrl || !rmse || !inliers || !ok)
        return reject("cgs_pair_consensus_fit: invalid argument (NULL pointer or pairs without curves, B=%d)", B);
    launch_pair_consensus_fit((hipStream_t)stream_, K, curve_points, pairs, sample_num, ransac_thresh, error_threshold, ctrl,
                              rmse, inliers, ok);
    return finish("pair_consensus_fit", stream_);
}

int cgs_undistort_images(int n_views, const cgs_undistort_view* views, float fill, int* blank_counts, void* stream_) {
    if (n_views < 0 || n_views > CGS_UNDISTORT_MAX_VIEWS)
        return reject("cgs_undistort_images: invalid argument (n_views=%d, at most %d per call)", n_views,
                      CGS_UNDISTORT_MAX_VIEWS);
    if (n_views == 0) return CGS_OK;
    if (!views || !blank_counts) return reject("cgs_undistort_images: invalid argument (NULL pointer)");
    if (!std::isfinite(fill)) return reject("cgs_undistort_images: invalid argument (fill is not finite)");
    for (int v = 0; v < n_views; v++) {
        const cgs_undistort_view& d = views[v];
        if (!d.src || !d.dst || d.src == d.dst)
            return reject("cgs_undistort_images: invalid argument (view %d: NULL pointer or dst == src)", v);
        if (d.channels < 1 || d.channels > CGS_UNDISTORT_MAX_CHANNELS || d.height <= 0 || d.width <= 0)
            return reject("cgs_undistort_images: invalid argument (view %d: channels=%d (1..%d), height=%d, width=%d)", v,
                          d.channels, CGS_UNDISTORT_MAX_CHANNELS, d.height, d.width);
        if (d.model != 0 && d.model != 1 && d.model != 2 && d.model != 3 && d.model != 4 && d.model != 6)
            return reject("cgs_undistort_images: invalid argument (view %d: camera model id %d is not supported: SIMPLE_PINHOLE 0, "
                          "PINHOLE 1, SIMPLE_RADIAL 2, RADIAL 3, OPENCV 4 and FULL_OPENCV 6 are)", v, d.model);
        const double focals[4] = {d.fx, d.fy, d.out_fx, d.out_fy};
        for (double f : focals) {
            if (!(f > 0.0) || !std::isfinite(f))
                return reject("cgs_undistort_images: invalid argument (view %d: focal lengths fx=%g, fy=%g, out_fx=%g, out_fy=%g must "
                              "be positive and finite)", v, d.fx, d.fy, d.out_fx, d.out_fy);
        }
        bool finite = std::isfinite(d.cx) && std::isfinite(d.cy);
        for (double k : d.k) finite = finite && std::isfinite(k);
        if (!finite)
            return reject("cgs_undistort_images: invalid argument (view %d: a principal point or coefficient is not finite)",
                          v);
    }
    launch_undistort_images((hipStream_t)stream_, n_views, views, fill, blank_counts);
    return finish("undistort_images", stream_);
}

int cgs_edge_gradients(int n_views, const cgs_edge_gradient_view* views, const float* taps, int radius, void* stream_) {
    if (n_views < 1 || n_views > CGS_EDGE_MAX_VIEWS)
        return reject("cgs_edge_gradients: invalid argument (n_views=%d, 1..%d per call)", n_views, CGS_EDGE_MAX_VIEWS);
    if (!views || !taps) return reject("cgs_edge_gradients: invalid argument (NULL pointer)");
    if (radius < 0 || radius > CGS_EDGE_MAX_RADIUS)
        return reject("cgs_edge_gradients: invalid argument (radius=%d, 0..%d)", radius, CGS_EDGE_MAX_RADIUS);
    for (int v = 0; v < n_views; v++) {
        const cgs_edge_gradient_view& d = views[v];
        if (!d.pixels || !d.gx || !d.gy || !d.m)
            return reject("cgs_edge_gradients: invalid argument (view %d: NULL pointer)", v);
        if (d.height <= 0 || d.width <= 0 || (d.channels != 1 && d.channels != 3 && d.channels != 4))
            return reject("cgs_edge_gradients: invalid argument (view %d: height=%d, width=%d, channels=%d (1, 3 or 4))", v,
                          d.height, d.width, d.channels);
    }
    launch_edge_gradients((hipStream_t)stream_, n_views, views, taps, radius);
    return finish("edge_gradients", stream_);
}

int cgs_edge_trace(int n_views, const cgs_edge_trace_view* views, float low, float high, int thin, int* changed_flag,
                   void* stream_) {
    if (n_views < 1 || n_views > CGS_EDGE_MAX_VIEWS)
        return reject("cgs_edge_trace: invalid argument (n_views=%d, 1..%d per call)", n_views, CGS_EDGE_MAX_VIEWS);
    if (!views || !changed_flag) return reject("cgs_edge_trace: invalid argument (NULL pointer)");
    if (!(low > 0.0f) || !(low <= high) || !std::isfinite(high))   // (a NaN compares false)
        return reject("cgs_edge_trace: invalid argument (low=%g, high=%g: need 0 < low <= high, finite)", low, high);
    for (int v = 0; v < n_views; v++) {
        const cgs_edge_trace_view& d = views[v];
        if (!d.gx || !d.gy || !d.m || !d.e || !d.state)
            return reject("cgs_edge_trace: invalid argument (view %d: NULL pointer)", v);
        if (d.height <= 0 || d.width <= 0)
            return reject("cgs_edge_trace: invalid argument (view %d: height=%d, width=%d)", v, d.height, d.width);
    }
    hipError_t err = hipSuccess;
    const int rounds = launch_edge_trace((hipStream_t)stream_, n_views, views, low, high, thin, changed_flag, &err);
    if (rounds < 0) {
        set_error("edge_trace failed: %s", hipGetErrorString(err));
        return CGS_ERR_HIP;
    }
    if (!check_launch("edge_trace", false, (hipStream_t)stream_)) return CGS_ERR_HIP;
    return rounds;
}

int cgs_point_mask(int P, const float* points, int V, const double* intr, const double* w2c, int height, int width,
                   uint8_t* mask_out, int* kept, void* stream_) {
    if (P < 0 || V < 0) return reject("cgs_point_mask: invalid argument (P=%d, V=%d)", P, V);
    if (V == 0) return CGS_OK;
    if (height <= 0 || width <= 0) return reject("cgs_point_mask: invalid argument (height=%d, width=%d)", height, width);
    if (!intr || !w2c || !mask_out || (P > 0 && !points)) return reject("cgs_point_mask: invalid argument (NULL pointer)");
    if (launch_point_mask((hipStream_t)stream_, P, points, V, intr, w2c, height, width, mask_out, kept) != hipSuccess) {
        set_error("cgs_point_mask: clearing the mask failed");
        return CGS_ERR_HIP;
    }
    return finish("point_mask", stream_);
}

static bool edt_size_ok(int height, int width) {
    return height >= 1 && height <= CGS_EDT_MAX_SIZE && width >= 1 && width <= CGS_EDT_MAX_SIZE;
}

size_t cgs_edt_workspace_bytes(int V, int height, int width) {
    if (V < 0 || !edt_size_ok(height, width)) return 0;
    return edt_workspace_bytes(V, height, width);
}

int cgs_edt_squared(int V, int height, int width, const uint8_t* mask, void* workspace, int32_t* dist2_out, void* stream_) {
    if (V < 0 || !edt_size_ok(height, width))
        return reject("cgs_edt_squared: invalid argument (V=%d, height=%d, width=%d; sizes lie in [1, %d])", V, height, width,
                      CGS_EDT_MAX_SIZE);
    if (V == 0) return CGS_OK;
    if (!mask || !workspace || !dist2_out) return reject("cgs_edt_squared: invalid argument (NULL pointer)");
    launch_edt_squared((hipStream_t)stream_, V, height, width, mask, workspace, dist2_out);
    return finish("edt_squared", stream_);
}

size_t cgs_edge_score_workspace_bytes(int V) { return edge_score_workspace_bytes(V); }

int cgs_edge_score_reduce(int V, int height, int width, const uint8_t* pred_mask, const uint8_t* det_mask,
                          const int32_t* pred_dist2, const int32_t* det_dist2, int n_tol, const int* tol2, void* workspace,
                          int64_t* counts, double* sums, uint8_t* both_nonempty, void* stream_) {
    if (V < 0 || !edt_size_ok(height, width) || n_tol < 0 || n_tol > CGS_EDGE_SCORE_MAX_TOL)
        return reject("cgs_edge_score_reduce: invalid argument (V=%d, height=%d, width=%d, n_tol=%d)", V, height, width, n_tol);
    if (n_tol > 0 && !tol2) return reject("cgs_edge_score_reduce: invalid argument (NULL pointer)");
    for (int t = 0; t < n_tol; t++)
        if (tol2[t] < 0) return reject("cgs_edge_score_reduce: invalid argument (tol2[%d]=%d)", t, tol2[t]);
    if (V == 0) return CGS_OK;
    if (!pred_mask || !det_mask || !pred_dist2 || !det_dist2 || !workspace || !counts || !sums || !both_nonempty)
        return reject("cgs_edge_score_reduce: invalid argument (NULL pointer)");
    if (launch_edge_score_reduce((hipStream_t)stream_, V, height, width, pred_mask, det_mask, pred_dist2, det_dist2, n_tol,
                                 tol2, workspace, counts, sums, both_nonempty) != hipSuccess) {
        set_error("cgs_edge_score_reduce: clearing the counters failed");
        return CGS_ERR_HIP;
    }
    return finish("edge_score_reduce", stream_);
}

int cgs_pack_near_bits(int V, int height, int width, const int32_t* dist2, int tol2, uint32_t* bits_out, void* stream_) {
    if (V < 0 || !edt_size_ok(height, width) || tol2 < 0)
        return reject("cgs_pack_near_bits: invalid argument (V=%d, height=%d, width=%d, tol2=%d; sizes lie in [1, %d])", V,
                      height, width, tol2, CGS_EDT_MAX_SIZE);
    if (V == 0) return CGS_OK;
    if (!dist2 || !bits_out) return reject("cgs_pack_near_bits: invalid argument (NULL pointer)");
    launch_pack_near_bits((hipStream_t)stream_, V, height, width, dist2, tol2, bits_out);
    return finish("pack_near_bits", stream_);
}

// The checks that the seed entries share.  A grid: positive dims, nx ny and nx ny nz at most 2^31 - 1 and, where lo and step
// are given (cgs_voxel_moments has neither; a NULL one is the entry's to report), finite with step > 0.
static bool seed_grid_ok(const char* name, int nx, int ny, int nz, const double* lo, const double* step) {
    if (nx <= 0 || ny <= 0 || nz <= 0) {
        set_error("%s: invalid argument (dims=%dx%dx%d)", name, nx, ny, nz);
        return false;
    }
    if ((long long)nx * ny > INT32_MAX || (long long)nx * ny * nz > INT32_MAX) {   // the first product is below 2^62
        set_error("%s: invalid argument (%dx%dx%d voxels: at most 2^31 - 1)", name, nx, ny, nz);
        return false;
    }
    for (int a = 0; lo && step && a < 3; a++)
        if (!std::isfinite(lo[a]) || !std::isfinite(step[a]) || !(step[a] > 0.0)) {
            set_error("%s: invalid argument (axis %d: lo=%g, step=%g)", name, a, lo[a], step[a]);
            return false;
        }
    return true;
}

// The views of a seed entry: their number and the size of their maps.
static bool seed_views_ok(const char* name, int V, int height, int width) {
    if (V < 0 || V > CGS_SEED_MAX_VIEWS || !edt_size_ok(height, width)) {
        set_error("%s: invalid argument (V=%d, height=%d, width=%d; sizes lie in [1, %d])", name, V, height, width,
                  CGS_EDT_MAX_SIZE);
        return false;
    }
    return true;
}

// The three seed entries that walk the views: the slack comes right after the grid, the depth pointer among the pointers of
// the views.
static int voxel_votes_entry(const char* name, int nx, int ny, int nz, const double* lo, const double* step, int V,
                             const double* intr, const double* w2c, int height, int width, const uint32_t* bits,
                             const DepthGate* gate, int accumulate, uint16_t* seen, uint16_t* hit, uint16_t* hidden,
                             void* stream_) {
    // a NULL pointer is reported after the dims and before a bad lo or step, as it always was
    const bool ptrs = lo && step && seen && hit && (V == 0 || (intr && w2c && bits && !depth_missing(gate)));
    if (!seed_views_ok(name, V, height, width) || !seed_grid_ok(name, nx, ny, nz, ptrs ? lo : nullptr, ptrs ? step : nullptr))
        return CGS_ERR_INVALID_ARGUMENT;
    if (slack_bad(gate)) return reject_slack(name, gate);
    if (!ptrs) return reject("%s: invalid argument (NULL pointer)", name);
    if (V == 0 && accumulate) return CGS_OK;
    launch_voxel_votes((hipStream_t)stream_, SeedGrid{{lo[0], lo[1], lo[2]}, {step[0], step[1], step[2]}, nx, ny, nz},
                       SeedViews{V, height, width, (width + 31) / 32, intr, w2c, bits}, gate, accumulate, seen, hit, hidden);
    return finish(name + 4, stream_);
}

int cgs_voxel_votes(int nx, int ny, int nz, const double* lo, const double* step, int V, const double* intr,
                    const double* w2c, int height, int width, const uint32_t* bits, int accumulate, uint16_t* seen,
                    uint16_t* hit, void* stream_) {
    return voxel_votes_entry("cgs_voxel_votes", nx, ny, nz, lo, step, V, intr, w2c, height, width, bits, nullptr, accumulate,
                             seen, hit, nullptr, stream_);
}

int cgs_voxel_votes_depth(int nx, int ny, int nz, const double* lo, const double* step, int V, const double* intr,
                          const double* w2c, int height, int width, const uint32_t* bits, const float* depth, double slack,
                          int accumulate, uint16_t* seen, uint16_t* hit, uint16_t* hidden, void* stream_) {
    const DepthGate gate{depth, slack};
    return voxel_votes_entry("cgs_voxel_votes_depth", nx, ny, nz, lo, step, V, intr, w2c, height, width, bits, &gate,
                             accumulate, seen, hit, hidden, stream_);
}

int cgs_voxel_moments(int nx, int ny, int nz, const void* keep_bits, int N, const void* centres, int radius, void* moments,
                      void* stream_) {
    if (N < 0 || radius < 1 || radius > CGS_SEED_MAX_RADIUS)
        return reject("cgs_voxel_moments: invalid argument (N=%d, radius=%d; the radius lies in [1, %d])", N, radius,
                      CGS_SEED_MAX_RADIUS);
    if (!seed_grid_ok("cgs_voxel_moments", nx, ny, nz, nullptr, nullptr)) return CGS_ERR_INVALID_ARGUMENT;
    if (!keep_bits || !centres || !moments) return reject("cgs_voxel_moments: invalid argument (NULL pointer)");
    if (N == 0) return CGS_OK;
    launch_voxel_moments((hipStream_t)stream_, nx, ny, nz, (const unsigned int*)keep_bits, N, (const int*)centres, radius,
                         (int*)moments);
    return finish("voxel_moments", stream_);
}

static int ray_claims_entry(const char* name, int nx, int ny, int nz, const double* lo, const double* step, int M,
                            const int32_t* index, const uint16_t* support, int V, const double* intr, const double* w2c,
                            int height, int width, const uint32_t* bits, const DepthGate* gate, int clear, uint32_t* best,
                            void* stream_) {
    if (M < 0) return reject("%s: invalid argument (M=%d)", name, M);
    if (!seed_views_ok(name, V, height, width) || !seed_grid_ok(name, nx, ny, nz, lo, step)) return CGS_ERR_INVALID_ARGUMENT;
    if (slack_bad(gate)) return reject_slack(name, gate);
    if (!lo || !step || (V > 0 && !best) ||
        (M > 0 && V > 0 && (!index || !support || !intr || !w2c || !bits || depth_missing(gate))))
        return reject("%s: invalid argument (NULL pointer)", name);
    const SeedGrid g{{lo[0], lo[1], lo[2]}, {step[0], step[1], step[2]}, nx, ny, nz};
    const SeedViews views{V, height, width, (width + 31) / 32, intr, w2c, bits};
    if (launch_ray_claims((hipStream_t)stream_, g, views, gate, M, index, support, clear, best) != hipSuccess) {
        set_error("%s: clearing the claims failed", name);
        return CGS_ERR_HIP;
    }
    if (M == 0 || V == 0) return CGS_OK;
    return finish(name + 4, stream_);
}

int cgs_ray_claims(int nx, int ny, int nz, const double* lo, const double* step, int M, const int32_t* index,
                   const uint16_t* support, int V, const double* intr, const double* w2c, int height, int width,
                   const uint32_t* bits, int clear, uint32_t* best, void* stream_) {
    return ray_claims_entry("cgs_ray_claims", nx, ny, nz, lo, step, M, index, support, V, intr, w2c, height, width, bits,
                            nullptr, clear, best, stream_);
}

int cgs_ray_claims_depth(int nx, int ny, int nz, const double* lo, const double* step, int M, const int32_t* index,
                         const uint16_t* support, int V, const double* intr, const double* w2c, int height, int width,
                         const uint32_t* bits, const float* depth, double slack, int clear, uint32_t* best, void* stream_) {
    const DepthGate gate{depth, slack};
    return ray_claims_entry("cgs_ray_claims_depth", nx, ny, nz, lo, step, M, index, support, V, intr, w2c, height, width, bits,
                            &gate, clear, best, stream_);
}

// Here the slack comes after lo and step and before the window.
static int ray_wins_entry(const char* name, int nx, int ny, int nz, const double* lo, const double* step, int M,
                          const int32_t* index, const uint16_t* support, int V, const double* intr, const double* w2c,
                          int height, int width, const uint32_t* bits, const uint32_t* best, const DepthGate* gate, int window,
                          int margin, int accumulate, uint16_t* wins, void* stream_) {
    if (M < 0) return reject("%s: invalid argument (M=%d)", name, M);
    if (!seed_views_ok(name, V, height, width) || !seed_grid_ok(name, nx, ny, nz, lo, step)) return CGS_ERR_INVALID_ARGUMENT;
    if (!lo || !step)   // before the slack, the window and the margin, as it always was
        return reject("%s: invalid argument (NULL pointer)", name);
    if (slack_bad(gate)) return reject_slack(name, gate);
    if (window < 0 || window > CGS_SEED_MAX_WINDOW || margin < 0 || margin > 65535)
        return reject("%s: invalid argument (window=%d, margin=%d; the window lies in [0, %d], the margin in [0, 65535])", name,
                      window, margin, CGS_SEED_MAX_WINDOW);
    if (M > 0 && V > 0 && (!index || !support || !intr || !w2c || !bits || !best || depth_missing(gate) || !wins))
        return reject("%s: invalid argument (NULL pointer)", name);
    if (M == 0 || V == 0) return CGS_OK;
    launch_ray_wins((hipStream_t)stream_, SeedGrid{{lo[0], lo[1], lo[2]}, {step[0], step[1], step[2]}, nx, ny, nz},
                    SeedViews{V, height, width, (width + 31) / 32, intr, w2c, bits}, gate, M, index, support, best, window,
                    margin, accumulate, wins);
    return finish(name + 4, stream_);
}

int cgs_ray_wins(int nx, int ny, int nz, const double* lo, const double* step, int M, const int32_t* index,
                 const uint16_t* support, int V, const double* intr, const double* w2c, int height, int width,
                 const uint32_t* bits, const uint32_t* best, int window, int margin, int accumulate, uint16_t* wins,
                 void* stream_) {
    return ray_wins_entry("cgs_ray_wins", nx, ny, nz, lo, step, M, index, support, V, intr, w2c, height, width, bits, best,
                          nullptr, window, margin, accumulate, wins, stream_);
}

int cgs_ray_wins_depth(int nx, int ny, int nz, const double* lo, const double* step, int M, const int32_t* index,
                       const uint16_t* support, int V, const double* intr, const double* w2c, int height, int width,
                       const uint32_t* bits, const uint32_t* best, const float* depth, double slack, int window, int margin,
                       int accumulate, uint16_t* wins, void* stream_) {
    const DepthGate gate{depth, slack};
    return ray_wins_entry("cgs_ray_wins_depth", nx, ny, nz, lo, step, M, index, support, V, intr, w2c, height, width, bits,
                          best, &gate, window, margin, accumulate, wins, stream_);
}

// The slack comes before the no-op return.
static int edge_support_entry(const char* name, int E, int P, const float* points, const int32_t* offsets, int V,
                              const double* intr, const double* w2c, int height, int width, const int32_t* d2, int T,
                              const int32_t* tol2, const DepthGate* gate, int32_t* counts, int32_t* hidden, void* stream_) {
    if (E < 0 || P < 0 || V < 0 || T < 1 || T > CGS_EDGE_SUPPORT_MAX_TOL)
        return reject("%s: invalid argument (E=%d, P=%d, V=%d, T=%d; T lies in [1, %d])", name, E, P, V, T,
                      CGS_EDGE_SUPPORT_MAX_TOL);
    if (slack_bad(gate)) return reject_slack(name, gate);
    if (E == 0 || V == 0) return CGS_OK;
    if (!edt_size_ok(height, width))   // d2 is a cgs_edt_squared transform, depth has its size
        return reject("%s: invalid argument (height=%d, width=%d; sizes lie in [1, %d])", name, height, width,
                      CGS_EDT_MAX_SIZE);
    if (!offsets || !intr || !w2c || !d2 || !tol2 || depth_missing(gate) || !counts || (P > 0 && !points))
        return reject("%s: invalid argument (NULL pointer)", name);
    launch_edge_support((hipStream_t)stream_, E, P, points, offsets, V, intr, w2c, height, width, d2, T, tol2, gate, counts,
                        hidden);
    return finish(name + 4, stream_);
}

int cgs_edge_support(int E, int P, const float* points, const int32_t* offsets, int V, const double* intr,
                     const double* w2c, int height, int width, const int32_t* d2, int T, const int32_t* tol2,
                     int32_t* counts, void* stream_) {
    return edge_support_entry("cgs_edge_support", E, P, points, offsets, V, intr, w2c, height, width, d2, T, tol2, nullptr,
                              counts, nullptr, stream_);
}

int cgs_edge_support_depth(int E, int P, const float* points, const int32_t* offsets, int V, const double* intr,
                           const double* w2c, int height, int width, const int32_t* d2, int T, const int32_t* tol2,
                           const float* depth, double slack, int32_t* counts, int32_t* hidden, void* stream_) {
    const DepthGate gate{depth, slack};
    return edge_support_entry("cgs_edge_support_depth", E, P, points, offsets, V, intr, w2c, height, width, d2, T, tol2, &gate,
                              counts, hidden, stream_);
}

// The three per-sample operators: the slack comes right after the sizes.
static int sample_support_entry(const char* name, int P, const float* points, int V, const double* intr, const double* w2c,
                                int height, int width, const int32_t* d2, int T, const int32_t* tol2, const DepthGate* gate,
                                int32_t* tally, int32_t* hidden, void* stream_) {
    if (P < 0 || V < 0 || T < 1 || T > CGS_EDGE_SUPPORT_MAX_TOL)
        return reject("%s: invalid argument (P=%d, V=%d, T=%d; T lies in [1, %d])", name, P, V, T, CGS_EDGE_SUPPORT_MAX_TOL);
    if (!edt_size_ok(height, width))   // d2 is a cgs_edt_squared transform, depth has its size
        return reject("%s: invalid argument (height=%d, width=%d; sizes lie in [1, %d])", name, height, width,
                      CGS_EDT_MAX_SIZE);
    if (slack_bad(gate)) return reject_slack(name, gate);
    if (!intr || !w2c || !d2 || !tol2 || depth_missing(gate) || (P > 0 && (!points || !tally)))
        return reject("%s: invalid argument (NULL pointer; P=%d, V=%d)", name, P, V);
    if (P == 0 || V == 0) return CGS_OK;   // nothing to add
    launch_sample_support((hipStream_t)stream_, P, points, V, intr, w2c, height, width, d2, T, tol2, gate, tally, hidden);
    return finish(name + 4, stream_);
}

int cgs_sample_support(int P, const float* points, int V, const double* intr, const double* w2c, int height, int width,
                       const int32_t* d2, int T, const int32_t* tol2, int32_t* tally, void* stream_) {
    return sample_support_entry("cgs_sample_support", P, points, V, intr, w2c, height, width, d2, T, tol2, nullptr, tally,
                                nullptr, stream_);
}

int cgs_sample_support_depth(int P, const float* points, int V, const double* intr, const double* w2c, int height, int width,
                             const int32_t* d2, int T, const int32_t* tol2, const float* depth, double slack, int32_t* tally,
                             int32_t* hidden, void* stream_) {
    const DepthGate gate{depth, slack};
    return sample_support_entry("cgs_sample_support_depth", P, points, V, intr, w2c, height, width, d2, T, tol2, &gate, tally,
                                hidden, stream_);
}

size_t cgs_sample_cover_workspace_bytes(int P) { return sample_cover_workspace_bytes(P); }

int cgs_sample_cover(int P, const float* points, int E, const int32_t* offsets, const int32_t* rank, float tol2, float cos2,
                     int32_t* cover, void* workspace, void* stream_) {
    if (P < 0 || E < 0) return reject("cgs_sample_cover: invalid argument (P=%d, E=%d)", P, E);
    if (!(tol2 >= 0.f) || !(cos2 >= 0.f && cos2 <= 1.f))   // a NaN fails either comparison
        return reject("cgs_sample_cover: invalid argument (tol2=%g, cos2=%g; tol2 >= 0 and cos2 lies in [0, 1])",
                      (double)tol2, (double)cos2);
    if (!offsets || !rank || !workspace || (P > 0 && (!points || !cover)))
        return reject("cgs_sample_cover: invalid argument (NULL pointer; P=%d, E=%d)", P, E);
    if (P == 0 || E == 0) return CGS_OK;   // nothing to cover
    launch_sample_cover((hipStream_t)stream_, P, points, E, offsets, rank, tol2, cos2, cover, workspace);
    return finish("sample_cover", stream_);
}

size_t cgs_end_attach_workspace_bytes(int P, int E) { return end_attach_workspace_bytes(P, E); }

int cgs_end_attach(int P, const float* points, int E, const int32_t* offsets, float tol2, float reach2, uint64_t* keys,
                   void* workspace, void* stream_) {
    if (P < 0 || E < 0) return reject("cgs_end_attach: invalid argument (P=%d, E=%d)", P, E);
    if (!(tol2 >= 0.f) || !(reach2 >= 0.f))   // a NaN fails either comparison
        return reject("cgs_end_attach: invalid argument (tol2=%g, reach2=%g; neither may be negative or NaN)", (double)tol2,
                      (double)reach2);
    if (!offsets || !workspace || (P > 0 && !points) || (E > 0 && !keys))
        return reject("cgs_end_attach: invalid argument (NULL pointer; P=%d, E=%d)", P, E);
    if (E == 0) return CGS_OK;   // no end: nothing is written
    launch_end_attach((hipStream_t)stream_, P, points, E, offsets, tol2, reach2, (unsigned long long*)keys, workspace);
    return finish("end_attach", stream_);
}

int cgs_thin_masks(int V, int height, int width, uint8_t* masks, uint8_t* scratch, int* changed_flag, int max_iterations,
                   int* iterations_out, void* stream_) {
    if (V < 0 || !edt_size_ok(height, width) || max_iterations < 0)
        return reject("cgs_thin_masks: invalid argument (V=%d, height=%d, width=%d, max_iterations=%d; sizes lie in [1, %d])",
                      V, height, width, max_iterations, CGS_EDT_MAX_SIZE);
    if (V == 0) {
        if (iterations_out) *iterations_out = 0;
        return CGS_OK;
    }
    if (!masks || !scratch || !changed_flag) return reject("cgs_thin_masks: invalid argument (NULL pointer)");
    hipError_t err = hipSuccess;
    int iterations = 0;
    const int passes = launch_thin_masks((hipStream_t)stream_, V, height, width, masks, scratch, changed_flag, max_iterations,
                                         &iterations, &err);
    if (passes < 0) {
        set_error("thin_masks failed: %s", hipGetErrorString(err));
        return CGS_ERR_HIP;
    }
    if (!check_launch("thin_masks", false, (hipStream_t)stream_)) return CGS_ERR_HIP;
    if (iterations_out) *iterations_out = iterations;
    return passes;
}

int cgs_mask_orientation(int V, int height, int width, const uint8_t* mask, uint8_t* code, void* stream_) {
    if (V < 0 || !edt_size_ok(height, width))
        return reject("cgs_mask_orientation: invalid argument (V=%d, height=%d, width=%d; sizes lie in [1, %d])", V, height,
                      width, CGS_EDT_MAX_SIZE);
    if (!mask || !code) return reject("cgs_mask_orientation: invalid argument (NULL pointer)");
    if (V == 0) return CGS_OK;   // nothing to write
    launch_mask_orientation((hipStream_t)stream_, V, height, width, mask, code);
    return finish("mask_orientation", stream_);
}

int cgs_oriented_near(int V, int height, int width, const uint8_t* code, int tol2, uint8_t* near, void* stream_) {
    if (V < 0 || !edt_size_ok(height, width))
        return reject("cgs_oriented_near: invalid argument (V=%d, height=%d, width=%d; sizes lie in [1, %d])", V, height,
                      width, CGS_EDT_MAX_SIZE);
    if (tol2 < 0 || tol2 > CGS_ORIENT_MAX_TOL2)
        return reject("cgs_oriented_near: invalid argument (tol2=%d; tol2 lies in [0, %d])", tol2, CGS_ORIENT_MAX_TOL2);
    if (!code || !near) return reject("cgs_oriented_near: invalid argument (NULL pointer)");
    const size_t bytes = (size_t)V * (size_t)height * (size_t)width;   // at most 2^31 * 2^28
    const uintptr_t c0 = reinterpret_cast<uintptr_t>(code), n0 = reinterpret_cast<uintptr_t>(near);
    if (c0 < n0 + bytes && n0 < c0 + bytes)   // a tile reads its halo from code while its neighbours write near
        return reject("cgs_oriented_near: invalid argument (code and near overlap)");
    if (V == 0) return CGS_OK;   // nothing to write
    launch_oriented_near((hipStream_t)stream_, V, height, width, code, tol2, near);
    return finish("oriented_near", stream_);
}

static int sample_support_oriented_entry(const char* name, int P, const float* points, const int32_t* partner, int V,
                                         const double* intr, const double* w2c, int height, int width, const uint8_t* near,
                                         int spread, const DepthGate* gate, int32_t* tally, int32_t* hidden, void* stream_) {
    if (P < 0 || V < 0 || spread < 0 || spread > CGS_ORIENT_MAX_SPREAD)
        return reject("%s: invalid argument (P=%d, V=%d, spread=%d; the spread lies in [0, %d])", name, P, V, spread,
                      CGS_ORIENT_MAX_SPREAD);
    if (!edt_size_ok(height, width))
        return reject("%s: invalid argument (height=%d, width=%d; sizes lie in [1, %d])", name, height, width,
                      CGS_EDT_MAX_SIZE);
    if (slack_bad(gate)) return reject_slack(name, gate);
    if (!intr || !w2c || !near || depth_missing(gate) || (P > 0 && (!points || !partner || !tally)))
        return reject("%s: invalid argument (NULL pointer; P=%d, V=%d)", name, P, V);
    if (P == 0 || V == 0) return CGS_OK;   // nothing to add
    launch_sample_support_oriented((hipStream_t)stream_, P, points, partner, V, intr, w2c, height, width, near, spread, gate,
                                   tally, hidden);
    return finish(name + 4, stream_);
}

int cgs_sample_support_oriented(int P, const float* points, const int32_t* partner, int V, const double* intr,
                                const double* w2c, int height, int width, const uint8_t* near, int spread, int32_t* tally,
                                void* stream_) {
    return sample_support_oriented_entry("cgs_sample_support_oriented", P, points, partner, V, intr, w2c, height, width, near,
                                         spread, nullptr, tally, nullptr, stream_);
}

int cgs_sample_support_oriented_depth(int P, const float* points, const int32_t* partner, int V, const double* intr,
                                      const double* w2c, int height, int width, const uint8_t* near, int spread,
                                      const float* depth, double slack, int32_t* tally, int32_t* hidden, void* stream_) {
    const DepthGate gate{depth, slack};
    return sample_support_oriented_entry("cgs_sample_support_oriented_depth", P, points, partner, V, intr, w2c, height, width,
                                         near, spread, &gate, tally, hidden, stream_);
}

static int sample_snap_terms_entry(const char* name, int P, const float* points, int V, const double* intr, const double* w2c,
                                   int height, int width, const int32_t* d2, int cap2, const double* dist_lut,
                                   const DepthGate* gate, double* terms, int32_t* views, int32_t* hidden, void* stream_) {
    if (P < 0 || V < 0 || cap2 < 1 || cap2 > CGS_SNAP_MAX_CAP2)   // the kernel stages cap2 + 1 table entries in LDS
        return reject("%s: invalid argument (P=%d, V=%d, cap2=%d; cap2 lies in [1, %d])", name, P, V, cap2, CGS_SNAP_MAX_CAP2);
    if (!edt_size_ok(height, width))   // d2 is a cgs_edt_squared transform, depth has its size
        return reject("%s: invalid argument (height=%d, width=%d; sizes lie in [1, %d])", name, height, width,
                      CGS_EDT_MAX_SIZE);
    if (slack_bad(gate)) return reject_slack(name, gate);
    if (!intr || !w2c || !d2 || !dist_lut || depth_missing(gate) || (P > 0 && (!points || !terms || !views)))
        return reject("%s: invalid argument (NULL pointer; P=%d, V=%d)", name, P, V);
    if (P == 0 || V == 0) return CGS_OK;   // nothing to add
    launch_sample_snap_terms((hipStream_t)stream_, P, points, V, intr, w2c, height, width, d2, cap2, dist_lut, gate, terms,
                             views, hidden);
    return finish(name + 4, stream_);
}

int cgs_sample_snap_terms(int P, const float* points, int V, const double* intr, const double* w2c, int height, int width,
                          const int32_t* d2, int cap2, const double* dist_lut, double* terms, int32_t* views,
                          void* stream_) {
    return sample_snap_terms_entry("cgs_sample_snap_terms", P, points, V, intr, w2c, height, width, d2, cap2, dist_lut, nullptr,
                                   terms, views, nullptr, stream_);
}

int cgs_sample_snap_terms_depth(int P, const float* points, int V, const double* intr, const double* w2c, int height,
                                int width, const int32_t* d2, int cap2, const double* dist_lut, const float* depth,
                                double slack, double* terms, int32_t* views, int32_t* hidden, void* stream_) {
    const DepthGate gate{depth, slack};
    return sample_snap_terms_entry("cgs_sample_snap_terms_depth", P, points, V, intr, w2c, height, width, d2, cap2, dist_lut,
                                   &gate, terms, views, hidden, stream_);
}

// Near-plane clipping: the plane is checked right after the sizes (and the slack, where there is one).
static int mesh_depth_entry(const char* name, int F, const float* tris, int V, const double* intr, const double* w2c,
                            int height, int width, const double* near, float* depth, void* stream_) {
    if (F < 0 || V < 0) return reject("%s: invalid argument (F=%d, V=%d)", name, F, V);
    if (!edt_size_ok(height, width))
        return reject("%s: invalid argument (height=%d, width=%d; sizes lie in [1, %d])", name, height, width,
                      CGS_EDT_MAX_SIZE);
    if (near && !near_ok(*near)) return reject("%s: invalid argument (near=%g; the plane is finite and > 0)", name, *near);
    if (!intr || !w2c || !depth || (F > 0 && !tris)) return reject("%s: invalid argument (NULL pointer; F=%d)", name, F);
    if (V == 0) return CGS_OK;   // nothing to write
    if (launch_mesh_depth((hipStream_t)stream_, F, tris, V, intr, w2c, height, width, near, depth) != hipSuccess) {
        set_error("%s: filling the depth planes failed", name);
        return CGS_ERR_HIP;
    }
    return finish(name + 4, stream_);
}

int cgs_mesh_depth(int F, const float* tris, int V, const double* intr, const double* w2c, int height, int width,
                   float* depth, void* stream_) {
    return mesh_depth_entry("cgs_mesh_depth", F, tris, V, intr, w2c, height, width, nullptr, depth, stream_);
}

int cgs_mesh_depth_clipped(int F, const float* tris, int V, const double* intr, const double* w2c, int height, int width,
                           double near, float* depth, void* stream_) {
    return mesh_depth_entry("cgs_mesh_depth_clipped", F, tris, V, intr, w2c, height, width, &near, depth, stream_);
}

int cgs_depth_window_max(int V, int height, int width, int radius, const float* depth, float* out, void* stream_) {
    if (V < 0 || !edt_size_ok(height, width))
        return reject("cgs_depth_window_max: invalid argument (V=%d, height=%d, width=%d; sizes lie in [1, %d])", V, height,
                      width, CGS_EDT_MAX_SIZE);
    if (radius < 0 || radius > CGS_DEPTH_MAX_WINDOW)   // the tile's LDS halo
        return reject("cgs_depth_window_max: invalid argument (radius=%d; the radius lies in [0, %d])", radius,
                      CGS_DEPTH_MAX_WINDOW);
    if (!depth || !out) return reject("cgs_depth_window_max: invalid argument (NULL pointer)");
    const size_t bytes = (size_t)V * (size_t)height * (size_t)width * sizeof(float);
    const uintptr_t d0 = reinterpret_cast<uintptr_t>(depth), o0 = reinterpret_cast<uintptr_t>(out);
    if (d0 < o0 + bytes && o0 < d0 + bytes)   // a tile reads its halo from depth while its neighbours write out
        return reject("cgs_depth_window_max: invalid argument (depth and out overlap)");
    if (V == 0) return CGS_OK;   // nothing to write
    launch_depth_window_max((hipStream_t)stream_, V, height, width, radius, depth, out);
    return finish("depth_window_max", stream_);
}

int cgs_point_mask_depth(int P, const float* points, int V, const double* intr, const double* w2c, int height, int width,
                         const float* depth, double slack, uint8_t* mask_out, int* kept, int* hidden, void* stream_) {
    if (P < 0 || V < 0) return reject("cgs_point_mask_depth: invalid argument (P=%d, V=%d)", P, V);
    if (!edt_size_ok(height, width))
        return reject("cgs_point_mask_depth: invalid argument (height=%d, width=%d; sizes lie in [1, %d])", height, width,
                      CGS_EDT_MAX_SIZE);
    if (!(slack >= 0.0) || std::isinf(slack))
        return reject("cgs_point_mask_depth: invalid argument (slack=%g; the slack is finite and >= 0)", slack);
    if (!intr || !w2c || !depth || !mask_out || (P > 0 && !points))
        return reject("cgs_point_mask_depth: invalid argument (NULL pointer; P=%d)", P);
    if (V == 0) return CGS_OK;   // nothing to write
    if (launch_point_mask_depth((hipStream_t)stream_, P, points, V, intr, w2c, height, width, depth, slack, mask_out, kept,
                                hidden) != hipSuccess) {
        set_error("cgs_point_mask_depth: clearing the mask failed");
        return CGS_ERR_HIP;
    }
    return finish("point_mask_depth", stream_);
}

// ---- occluding contours of a mesh (include/curvegs.h).  The slack is checked only with a plane: without one it is not read.
static int mesh_contours_entry(const char* name, int E, const float* edges, int V, const double* intr, const double* w2c,
                               int height, int width, const float* depth, double slack, const double* near, uint8_t* mask_out,
                               void* stream_) {
    if (E < 0 || V < 0) return reject("%s: invalid argument (E=%d, V=%d)", name, E, V);
    if (!edt_size_ok(height, width))
        return reject("%s: invalid argument (height=%d, width=%d; sizes lie in [1, %d])", name, height, width,
                      CGS_EDT_MAX_SIZE);
    if (depth && !slack_ok(slack))
        return reject("%s: invalid argument (slack=%g; with a depth plane the slack is finite and >= 0)", name, slack);
    if (near && !near_ok(*near)) return reject("%s: invalid argument (near=%g; the plane is finite and > 0)", name, *near);
    if (!intr || !w2c || !mask_out || (E > 0 && !edges)) return reject("%s: invalid argument (NULL pointer; E=%d)", name, E);
    if (V == 0) return CGS_OK;   // nothing to clear
    const DepthGate gate{depth, slack};
    if (launch_mesh_contours((hipStream_t)stream_, E, edges, V, intr, w2c, height, width, depth ? &gate : nullptr, near,
                             mask_out) != hipSuccess) {
        set_error("%s: clearing the mask failed", name);
        return CGS_ERR_HIP;
    }
    return finish(name + 4, stream_);
}

int cgs_mesh_contours(int E, const float* edges, int V, const double* intr, const double* w2c, int height, int width,
                      const float* depth, double slack, uint8_t* mask_out, void* stream_) {
    return mesh_contours_entry("cgs_mesh_contours", E, edges, V, intr, w2c, height, width, depth, slack, nullptr, mask_out,
                               stream_);
}

int cgs_mesh_contours_clipped(int E, const float* edges, int V, const double* intr, const double* w2c, int height, int width,
                              const float* depth, double slack, double near, uint8_t* mask_out, void* stream_) {
    return mesh_contours_entry("cgs_mesh_contours_clipped", E, edges, V, intr, w2c, height, width, depth, slack, &near,
                               mask_out, stream_);
}

// ---- the surfel z-buffer (include/curvegs.h): cgs_mesh_depth's checks in their order; normals may always be NULL.
int cgs_surfel_depth(int P, const float* points, const float* normals, const float* radii, int V, const double* intr,
                     const double* w2c, int height, int width, float* depth, void* stream_) {
    if (P < 0 || V < 0) return reject("cgs_surfel_depth: invalid argument (P=%d, V=%d)", P, V);
    if (!edt_size_ok(height, width))
        return reject("cgs_surfel_depth: invalid argument (height=%d, width=%d; sizes lie in [1, %d])", height, width,
                      CGS_EDT_MAX_SIZE);
    if (!intr || !w2c || !depth || (P > 0 && (!points || !radii)))
        return reject("cgs_surfel_depth: invalid argument (NULL pointer; P=%d)", P);
    if (V == 0) return CGS_OK;   // nothing to write
    if (launch_surfel_depth((hipStream_t)stream_, P, points, normals, radii, V, intr, w2c, height, width, depth) != hipSuccess) {
        set_error("cgs_surfel_depth: filling the depth planes failed");
        return CGS_ERR_HIP;
    }
    return finish("surfel_depth", stream_);
}

// ---- plane-sweep stereo (include/curvegs.h).  The arrays are the device's: an entry of src outside [0, V) is no source.
int cgs_stereo_sweep(int V, int height, int width, const uint8_t* gray, const double* intr, int D, const double* inv, int S,
                     const int* src, const double* rel, int radius, double min_var, double max_cost, int min_sources,
                     float* depth, void* stream_) {
    if (V < 0 || !edt_size_ok(height, width))
        return reject("cgs_stereo_sweep: invalid argument (V=%d, height=%d, width=%d; sizes lie in [1, %d])", V, height, width,
                      CGS_EDT_MAX_SIZE);
    if (D < 1 || S < 1 || min_sources < 1)
        return reject("cgs_stereo_sweep: invalid argument (D=%d, S=%d, min_sources=%d; each is at least 1)", D, S, min_sources);
    if (radius < 0 || radius > CGS_STEREO_MAX_RADIUS)   // the tile's LDS halo
        return reject("cgs_stereo_sweep: invalid argument (radius=%d; the radius lies in [0, %d])", radius,
                      CGS_STEREO_MAX_RADIUS);
    if (!(min_var >= 0.0) || max_cost != max_cost)
        return reject("cgs_stereo_sweep: invalid argument (min_var=%g, max_cost=%g; min_var is >= 0, neither is NaN)", min_var,
                      max_cost);
    if (!gray || !intr || !inv || !src || !rel || !depth) return reject("cgs_stereo_sweep: invalid argument (NULL pointer)");
    if (V == 0) return CGS_OK;   // nothing to write
    launch_stereo_sweep((hipStream_t)stream_, V, height, width, gray, intr, D, inv, S, src, rel, radius, min_var, max_cost,
                        min_sources, depth);
    return finish("stereo_sweep", stream_);
}

int cgs_stereo_consistency(int V, int height, int width, const float* depth, const double* intr, int S, const int* src,
                           const double* rel, const double* tol, int min_consistent, float* out, void* stream_) {
    if (V < 0 || !edt_size_ok(height, width))
        return reject("cgs_stereo_consistency: invalid argument (V=%d, height=%d, width=%d; sizes lie in [1, %d])", V, height,
                      width, CGS_EDT_MAX_SIZE);
    if (S < 1 || min_consistent < 0)
        return reject("cgs_stereo_consistency: invalid argument (S=%d, min_consistent=%d; S is at least 1, min_consistent "
                      "at least 0)", S, min_consistent);
    if (!depth || !intr || !src || !rel || !tol || !out) return reject("cgs_stereo_consistency: invalid argument (NULL pointer)");
    const size_t bytes = (size_t)V * (size_t)height * (size_t)width * sizeof(float);
    const uintptr_t d0 = reinterpret_cast<uintptr_t>(depth), o0 = reinterpret_cast<uintptr_t>(out);
    if (d0 < o0 + bytes && o0 < d0 + bytes)   // a pixel reads its sources' planes while their pixels are written
        return reject("cgs_stereo_consistency: invalid argument (depth and out overlap)");
    if (V == 0) return CGS_OK;   // nothing to write
    launch_stereo_consistency((hipStream_t)stream_, V, height, width, depth, intr, S, src, rel, tol, min_consistent, out);
    return finish("stereo_consistency", stream_);
}

// ---- fusing the stereo maps (include/curvegs.h).  The checks the two entries share: the sizes, the range, F.
static bool fuse_shape_ok(int V, int height, int width, int F, int v0, int nv) {
    return V >= 0 && edt_size_ok(height, width) && F >= 1 && F <= CGS_STEREO_MAX_FUSE && v0 >= 0 && nv >= 0 && v0 <= V &&
           nv <= V - v0;
}
static bool ranges_overlap(const void* a, size_t abytes, const void* b, size_t bbytes) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return abytes > 0 && bbytes > 0 && a0 < b0 + bbytes && b0 < a0 + abytes;
}

int cgs_stereo_warp(int V, int height, int width, const float* depth, const double* intr, int F, const int* fsrc,
                    const double* into, int v0, int nv, float* warped, void* stream_) {
    if (!fuse_shape_ok(V, height, width, F, v0, nv))
        return reject("cgs_stereo_warp: invalid argument (V=%d, height=%d, width=%d, F=%d, v0=%d, nv=%d; sizes lie in [1, %d], "
                      "F in [1, %d], the range in [0, V])", V, height, width, F, v0, nv, CGS_EDT_MAX_SIZE, CGS_STEREO_MAX_FUSE);
    if (!depth || !intr || !fsrc || !into || !warped) return reject("cgs_stereo_warp: invalid argument (NULL pointer)");
    const size_t plane = (size_t)height * (size_t)width * sizeof(float);
    if (ranges_overlap(depth, (size_t)V * plane, warped, (size_t)nv * (size_t)F * plane))
        return reject("cgs_stereo_warp: invalid argument (depth and warped overlap)");
    if (nv == 0) return CGS_OK;   // nothing to write
    if (launch_stereo_warp((hipStream_t)stream_, V, height, width, depth, intr, F, fsrc, into, v0, nv, warped) != hipSuccess) {
        set_error("cgs_stereo_warp: filling the warped planes failed");
        return CGS_ERR_HIP;
    }
    return finish("stereo_warp", stream_);
}

int cgs_stereo_fuse(int V, int height, int width, const float* depth, int F, const float* warped, const double* tol,
                    int min_support, int v0, int nv, float* out, uint8_t* support, void* stream_) {
    if (!fuse_shape_ok(V, height, width, F, v0, nv))
        return reject("cgs_stereo_fuse: invalid argument (V=%d, height=%d, width=%d, F=%d, v0=%d, nv=%d; sizes lie in [1, %d], "
                      "F in [1, %d], the range in [0, V])", V, height, width, F, v0, nv, CGS_EDT_MAX_SIZE, CGS_STEREO_MAX_FUSE);
    if (min_support < 1) return reject("cgs_stereo_fuse: invalid argument (min_support=%d; it is at least 1)", min_support);
    if (!depth || !warped || !tol || !out) return reject("cgs_stereo_fuse: invalid argument (NULL pointer)");
    const size_t pixels = (size_t)height * (size_t)width, plane = pixels * sizeof(float);
    const size_t dbytes = (size_t)V * plane, wbytes = (size_t)nv * (size_t)F * plane, obytes = (size_t)nv * plane;
    if (ranges_overlap(out, obytes, depth, dbytes) || ranges_overlap(out, obytes, warped, wbytes) ||
        (support && (ranges_overlap(support, (size_t)nv * pixels, depth, dbytes) ||
                     ranges_overlap(support, (size_t)nv * pixels, warped, wbytes) ||
                     ranges_overlap(support, (size_t)nv * pixels, out, obytes))))
        return reject("cgs_stereo_fuse: invalid argument (the outputs overlap an input or each other)");
    if (nv == 0) return CGS_OK;   // nothing to write
    launch_stereo_fuse((hipStream_t)stream_, height, width, depth, F, warped, tol, min_support, v0, nv, out, support);
    return finish("stereo_fuse", stream_);
}

// ---- the distance field and its surface (include/curvegs.h).  The grid and the views are checked as the seed entries
// check theirs.
static bool tsdf_weight_ok(int min_weight) { return min_weight >= 1 && min_weight <= CGS_TSDF_MAX_WEIGHT; }

int cgs_tsdf_integrate(int nx, int ny, int nz, const double* lo, const double* step, int V, const double* intr,
                       const double* w2c, int height, int width, const float* depth, double trunc, int accumulate, double* sum,
                       uint16_t* weight, void* stream_) {
    const char* name = "cgs_tsdf_integrate";
    const bool ptrs = lo && step && sum && weight && (V == 0 || (intr && w2c && depth));
    if (!seed_views_ok(name, V, height, width) || !seed_grid_ok(name, nx, ny, nz, ptrs ? lo : nullptr, ptrs ? step : nullptr))
        return CGS_ERR_INVALID_ARGUMENT;
    if (!(trunc > 0.0) || std::isinf(trunc))   // a NaN fails the comparison
        return reject("%s: invalid argument (trunc=%g; the truncation distance is finite and > 0)", name, trunc);
    if (!ptrs) return reject("%s: invalid argument (NULL pointer)", name);
    if (V == 0 && accumulate) return CGS_OK;   // nothing to add
    launch_tsdf_integrate((hipStream_t)stream_, SeedGrid{{lo[0], lo[1], lo[2]}, {step[0], step[1], step[2]}, nx, ny, nz},
                          TsdfViews{V, height, width, intr, w2c, depth}, trunc, accumulate, sum, weight);
    return finish("tsdf_integrate", stream_);
}

int cgs_tsdf_mesh_count(int nx, int ny, int nz, const double* sum, const uint16_t* weight, int min_weight, uint8_t* counts,
                        void* stream_) {
    const char* name = "cgs_tsdf_mesh_count";
    if (!seed_grid_ok(name, nx, ny, nz, nullptr, nullptr)) return CGS_ERR_INVALID_ARGUMENT;
    if (!tsdf_weight_ok(min_weight))
        return reject("%s: invalid argument (min_weight=%d; it lies in [1, %d])", name, min_weight, CGS_TSDF_MAX_WEIGHT);
    if (!sum || !weight) return reject("%s: invalid argument (NULL pointer)", name);
    if (nx == 1 || ny == 1 || nz == 1) return CGS_OK;   // no cells: nothing to write
    if (!counts) return reject("%s: invalid argument (NULL pointer)", name);
    launch_tsdf_count((hipStream_t)stream_, SeedGrid{{0.0, 0.0, 0.0}, {1.0, 1.0, 1.0}, nx, ny, nz}, sum, weight, min_weight, counts);
    return finish("tsdf_mesh_count", stream_);
}

int cgs_tsdf_mesh_emit(int nx, int ny, int nz, const double* lo, const double* step, const double* sum, const uint16_t* weight,
                       int min_weight, const int64_t* offsets, int64_t T, float* tris, void* stream_) {
    const char* name = "cgs_tsdf_mesh_emit";
    const bool cells = nx > 1 && ny > 1 && nz > 1;
    const bool ptrs = lo && step && sum && weight && (!cells || T == 0 || (offsets && tris));
    if (!seed_grid_ok(name, nx, ny, nz, ptrs ? lo : nullptr, ptrs ? step : nullptr)) return CGS_ERR_INVALID_ARGUMENT;
    if (!tsdf_weight_ok(min_weight))
        return reject("%s: invalid argument (min_weight=%d; it lies in [1, %d])", name, min_weight, CGS_TSDF_MAX_WEIGHT);
    if (T < 0) return reject("%s: invalid argument (T=%lld; it is at least 0)", name, (long long)T);
    if (!ptrs) return reject("%s: invalid argument (NULL pointer)", name);
    if (!cells || T == 0) return CGS_OK;   // nothing to write
    launch_tsdf_emit((hipStream_t)stream_, SeedGrid{{lo[0], lo[1], lo[2]}, {step[0], step[1], step[2]}, nx, ny, nz}, sum, weight,
                     min_weight, (const long long*)offsets, (long long)T, tris);
    return finish("tsdf_mesh_emit", stream_);
}

}  // extern "C"
