// C ABI around the reference rasterizer (CudaRasterizer::Rasterizer, built from the reference's own cuda_rasterizer/ sources
// by oracle/ref_raster/Makefile).  It plays the role of the reference's rasterize_points.cu without torch: the caller passes
// device pointers, the three scratch buffers live in a context the wrapper owns, and the accessors decode the reference's
// own saved state through GeometryState / BinningState / ImageState::fromChunk.
//
// Conventions follow rasterize_points.cu: nothing runs when P == 0; the inverse depth output is [1,H,W]; dL_dinvdepths is
// only written when an upstream inverse-depth gradient is given; dL_dsh is [P,M,3] (the kernel fills the first P*M floats);
// NUM_CHANNELS = 1, NUM_ALL_MAP = 4.  Every C++ exception is caught here and becomes a non-zero return code.
// The GLM shim's host-only check exports (glm_check.cpp) are linked into the same library.
//
// Test infrastructure only: loaded by oracle/ref_raster.py, never by the product.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <exception>
#include <functional>
#include <string>

#include "config.h"
#include "rasterizer.h"
#include "rasterizer_impl.h"

namespace {

struct Buffer {
    char* ptr = nullptr;
    size_t bytes = 0;
    char* resize(size_t n) {
        if (n > bytes) {
            if (ptr) hipFree(ptr);
            ptr = nullptr;
            bytes = 0;
            if (hipMalloc(&ptr, n) != hipSuccess) throw std::runtime_error("hipMalloc failed");
            bytes = n;
        }
        return ptr;
    }
    ~Buffer() {
        if (ptr) hipFree(ptr);
    }
};

struct Context {
    int P = 0, W = 0, H = 0;
    int num_rendered = 0;
    Buffer geom, binning, image;
};

thread_local std::string g_error;

int fail(const char* what) {
    g_error = what;
    return 1;
}

int copy_out(void* dst, const void* src, size_t bytes) {
    if (bytes == 0) return 0;
    if (hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) != hipSuccess) return fail("hipMemcpy failed");
    return 0;
}

}  // namespace

extern "C" {

const char* ref_last_error() { return g_error.c_str(); }

int ref_num_channels() { return NUM_CHANNELS; }
int ref_num_all_map() { return NUM_ALL_MAP; }

// Forward.  *ctx_out receives a new context (also for P == 0); radii is [P] int32; outputs are zero-initialised by the caller
// like the binding's torch::full(...).
int ref_forward(void** ctx_out, int P, int D, int M, const float* background, int W, int H, const float* means3D,
                const float* shs, const float* colors_precomp, const float* opacities, const float* scales,
                float scale_modifier, const float* rotations, const float* cov3D_precomp, const float* all_map,
                const float* viewmatrix, const float* projmatrix, const float* cam_pos, float tan_fovx, float tan_fovy,
                int prefiltered, float* out_color, float* out_invdepth, float* out_all_map, int antialiasing,
                int render_geo, int* radii) {
    try {
        *ctx_out = nullptr;
        if (prefiltered) return fail("prefiltered == true is not supported (its only effect is a device trap)");
        Context* ctx = new Context();
        ctx->P = P;
        ctx->W = W;
        ctx->H = H;
        *ctx_out = ctx;
        if (P == 0) return 0;
        auto geomFunc = [ctx](size_t n) { return ctx->geom.resize(n); };
        auto binningFunc = [ctx](size_t n) { return ctx->binning.resize(n); };
        auto imgFunc = [ctx](size_t n) { return ctx->image.resize(n); };
        ctx->num_rendered = CudaRasterizer::Rasterizer::forward(
            geomFunc, binningFunc, imgFunc, P, D, M, background, W, H, means3D, shs, colors_precomp, opacities, scales,
            scale_modifier, rotations, cov3D_precomp, all_map, viewmatrix, projmatrix, cam_pos, tan_fovx, tan_fovy, false,
            out_color, out_invdepth, out_all_map, antialiasing != 0, render_geo != 0, radii, false);
        if (hipDeviceSynchronize() != hipSuccess) return fail("reference forward failed on the device");
        return 0;
    } catch (const std::exception& e) {
        return fail(e.what());
    } catch (...) {
        return fail("unknown exception in ref_forward");
    }
}

// Backward over the state of one ref_forward.  all_map_pixels is the forward's out_all_map (the binding saves it);
// dL_dinvdepth_out / dL_invdepths may be null together (no upstream inverse-depth gradient).
int ref_backward(void* handle, int D, int M, const float* background, const float* all_map_pixels, const float* means3D,
                 const float* shs, const float* colors_precomp, const float* all_maps, const float* opacities,
                 const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
                 const float* viewmatrix, const float* projmatrix, const float* campos, float tan_fovx, float tan_fovy,
                 const int* radii, const float* dL_dpix, const float* dL_invdepths, const float* dL_dout_all_map,
                 float* dL_dmean2D, float* dL_dconic, float* dL_dopacity, float* dL_dcolor, float* dL_dinvdepth,
                 float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscale, float* dL_drot, float* dL_dall_map,
                 int antialiasing, int render_geo) {
    try {
        Context* ctx = static_cast<Context*>(handle);
        if (!ctx) return fail("null context");
        if (ctx->P == 0) return 0;
        CudaRasterizer::Rasterizer::backward(
            ctx->P, D, M, ctx->num_rendered, background, all_map_pixels, ctx->W, ctx->H, means3D, shs, colors_precomp,
            all_maps, opacities, scales, scale_modifier, rotations, cov3D_precomp, viewmatrix, projmatrix, campos, tan_fovx,
            tan_fovy, radii, ctx->geom.ptr, ctx->binning.ptr, ctx->image.ptr, dL_dpix, dL_invdepths, dL_dout_all_map,
            dL_dmean2D, dL_dconic, dL_dopacity, dL_dcolor, dL_dinvdepth, dL_dmean3D, dL_dcov3D, dL_dsh, dL_dscale, dL_drot,
            dL_dall_map, antialiasing != 0, render_geo != 0, false);
        if (hipDeviceSynchronize() != hipSuccess) return fail("reference backward failed on the device");
        return 0;
    } catch (const std::exception& e) {
        return fail(e.what());
    } catch (...) {
        return fail("unknown exception in ref_backward");
    }
}

int ref_mark_visible(int P, float* means3D, float* viewmatrix, float* projmatrix, bool* present) {
    try {
        if (P == 0) return 0;
        CudaRasterizer::Rasterizer::markVisible(P, means3D, viewmatrix, projmatrix, present);
        if (hipDeviceSynchronize() != hipSuccess) return fail("reference markVisible failed on the device");
        return 0;
    } catch (const std::exception& e) {
        return fail(e.what());
    } catch (...) {
        return fail("unknown exception in ref_mark_visible");
    }
}

int ref_num_rendered(void* handle) { return handle ? static_cast<Context*>(handle)->num_rendered : 0; }

// State accessors: copy the reference's own saved state to host memory the caller sized.
//   ranges    [tiles, 2] uint32     n_contrib [H*W] uint32     final_T [H*W] float
//   point_list [num_rendered] uint32 (sorted)                  point_keys [num_rendered] uint64 (sorted)
//   means2D [P, 2], depths [P], conic_opacity [P, 4], tiles_touched [P] uint32
int ref_copy_state(void* handle, const char* which, void* dst) {
    try {
        Context* ctx = static_cast<Context*>(handle);
        if (!ctx) return fail("null context");
        if (ctx->P == 0) return 0;
        const size_t P = ctx->P, N = size_t(ctx->W) * ctx->H, R = ctx->num_rendered;
        const size_t tiles = size_t((ctx->W + BLOCK_X - 1) / BLOCK_X) * ((ctx->H + BLOCK_Y - 1) / BLOCK_Y);
        char* g = ctx->geom.ptr;
        char* b = ctx->binning.ptr;
        char* im = ctx->image.ptr;
        CudaRasterizer::GeometryState geom = CudaRasterizer::GeometryState::fromChunk(g, P);
        CudaRasterizer::ImageState img = CudaRasterizer::ImageState::fromChunk(im, N);
        const std::string w(which);
        if (w == "ranges") return copy_out(dst, img.ranges, tiles * sizeof(uint2));
        if (w == "n_contrib") return copy_out(dst, img.n_contrib, N * sizeof(uint32_t));
        if (w == "final_T") return copy_out(dst, img.accum_alpha, N * sizeof(float));
        if (w == "means2D") return copy_out(dst, geom.means2D, P * sizeof(float2));
        if (w == "depths") return copy_out(dst, geom.depths, P * sizeof(float));
        if (w == "conic_opacity") return copy_out(dst, geom.conic_opacity, P * sizeof(float4));
        if (w == "tiles_touched") return copy_out(dst, geom.tiles_touched, P * sizeof(uint32_t));
        if (w == "point_list" || w == "point_keys") {
            CudaRasterizer::BinningState bin = CudaRasterizer::BinningState::fromChunk(b, R);
            if (w == "point_list") return copy_out(dst, bin.point_list, R * sizeof(uint32_t));
            return copy_out(dst, bin.point_list_keys, R * sizeof(uint64_t));
        }
        return fail("unknown state name");
    } catch (const std::exception& e) {
        return fail(e.what());
    } catch (...) {
        return fail("unknown exception in ref_copy_state");
    }
}

void ref_free(void* handle) { delete static_cast<Context*>(handle); }

}  // extern "C"
