/*
 * curvegs.h -- C ABI of libcurvegs.so, the MI355X (gfx950) native curve-Gaussian hot path.
 *
 * Drop-in boundary: these entry points are what the reference's torch extension shims
 * (/root/reference/submodules/diff-cur-rasterization/rasterize_points.cu, submodules/fused-ssim/ssim.cu,
 * submodules/simple-knn/spatial.cu) call into, restated with plain pointers, sizes and a HIP stream.
 * No torch types cross this boundary.  All pointers are DEVICE pointers unless marked "host".
 * Every function returns 0 (CGS_OK) / a non-negative count on success and a negative cgs_status on
 * failure; cgs_last_error() returns a thread-local message for the last failure.
 *
 * Memory is caller-owned.  The rasterizer's scratch state lives in three byte buffers obtained through
 * caller-supplied allocation callbacks, exactly like the reference's std::function<char*(size_t)>
 * resize callbacks (rasterize_points.cu:27-33, cuda_rasterizer/rasterizer.h:24-60); the same three
 * buffers are handed back to cgs_rasterize_backward.
 */
#ifndef CURVEGS_H_INCLUDED
#define CURVEGS_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum cgs_status {
    CGS_OK = 0,
    CGS_ERR_INVALID_ARGUMENT = -1,
    CGS_ERR_HIP = -2,          /* a HIP runtime call or kernel launch failed; see cgs_last_error() */
    CGS_ERR_ALLOC = -3,        /* an allocation callback returned NULL */
    CGS_ERR_NO_DEVICE = -4
} cgs_status;

/* Caller-supplied allocator: must return a device pointer to at least `bytes` bytes (any alignment >= 16;
 * the library aligns its carve-outs to 128 B itself), valid until the matching backward has run. */
typedef void* (*cgs_alloc_fn)(void* user, size_t bytes);

const char* cgs_last_error(void);
int cgs_version(void);
/* Name of the GPU ISA this library was compiled for ("gfx950"). */
const char* cgs_target_arch(void);

/* ------------------------------------------------------------------------------------------------
 * Rasterizer.  Replaces CudaRasterizer::Rasterizer::{forward,backward,markVisible}
 * (cuda_rasterizer/rasterizer.h:24-98; bodies cuda_rasterizer/rasterizer_impl.cu:198-347, :351-466, :141-153)
 * as called from RasterizeGaussiansCUDA / RasterizeGaussiansBackwardCUDA / markVisible
 * (rasterize_points.cu:35-130, :132-239, :241-260).
 *
 * Fixed by the reference's config.h: 1 colour channel, 4 "all_map" channels.
 * NULL for shs / colors_precomp / scales / rotations / cov3D_precomp / all_map plays the role of the
 * reference's empty tensors.  Exactly one of (shs, colors_precomp) and one of ((scales,rotations),
 * cov3D_precomp) must be non-NULL.  SH layout is the reference's single-channel [P, M] float layout
 * (forward.cu:32-33).
 *
 * cgs_rasterize_forward:
 *   out_color [1,H,W], out_invdepth [1,H,W], out_all_map [4,H,W] f32, radii [P] i32 are fully written
 *   (no pre-zeroing required).  Returns num_rendered (#(splat,tile) instances binned) >= 0, which the
 *   caller passes back as R.  Performs one stream synchronisation (to size the binning buffer), like
 *   the reference's blocking 4-byte D2H copy (rasterizer_impl.cu:287).  The readback goes through a slot of the
 *   status-slot pool of the checked view forwards (below), held for the length of the call: the call fails like
 *   cgs_view_forward_begin when all 64 slots are held by outstanding forwards.
 * ------------------------------------------------------------------------------------------------ */
int64_t cgs_rasterize_forward(
    cgs_alloc_fn geometry_alloc, void* geometry_user,
    cgs_alloc_fn binning_alloc, void* binning_user,
    cgs_alloc_fn image_alloc, void* image_user,
    int P, int D, int M,
    const float* background,      /* [3]; only [0] is read (1 channel) */
    int width, int height,
    const float* means3D,         /* [P,3] */
    const float* shs,             /* [P,M] or NULL */
    const float* colors_precomp,  /* [P,1] or NULL */
    const float* opacities,       /* [P,1] */
    const float* scales,          /* [P,3] or NULL */
    float scale_modifier,
    const float* rotations,       /* [P,4] (w,x,y,z), used UN-normalised, or NULL */
    const float* cov3D_precomp,   /* [P,6] or NULL */
    const float* all_map,         /* [P,4] or NULL (required when render_geo) */
    const float* viewmatrix,      /* [16], column-major math matrix = row-major transposed torch tensor */
    const float* projmatrix,      /* [16] */
    const float* cam_pos,         /* [3] */
    float tan_fovx, float tan_fovy,
    int prefiltered,
    float* out_color, float* out_invdepth, float* out_all_map,
    int antialiasing, int render_geo,
    int* radii,
    int debug,
    void* stream /* hipStream_t */);

/* cgs_rasterize_backward:
 *   Every gradient output is fully WRITTEN for all P splats (zeros for culled ones); unlike the reference's shim
 *   (rasterize_points.cu:173-193) the caller does not have to zero-fill anything, except dL_dsh [P,M], which is
 *   written for visible splats only when shs != NULL (zero it on entry).  The per-splat accumulation scratch lives
 *   in the geometry buffer, which is therefore written by the backward: the forward's preprocess kernel zeroes it and
 *   the backward hands it back zeroed, so any number of backward calls may follow one forward (no fill launch); the
 *   buffer must be the one the forward of the same splats wrote.
 *   dL_dmean2D [P,3] (.z = 0, NDC-scaled, quirk 9), dL_dconic [P,4] (.x,.y,.w; scratch in the reference, may be
 *   NULL), dL_dopacity [P], dL_dcolor [P,1], dL_dinvdepth [P] (NULL together with dL_dout_invdepth),
 *   dL_dall_map [P,4], dL_dmean3D [P,3], dL_dcov3D [P,6], dL_dscale [P,3], dL_drot [P,4].
 *   dL_dout_all_map may be NULL (treated as zeros) -- lets the autograd wrapper skip materialising unused grads.
 *   dL_dcolor may be NULL when the caller does not need the colour gradient (legal only with shs == NULL and no
 *   depth / all_map gradients flowing in: the training configuration, where colours are a constant ones tensor).
 */
int cgs_rasterize_backward(
    int P, int D, int M, int64_t R,
    const float* background,
    int width, int height,
    const float* means3D, const float* shs, const float* colors_precomp, const float* all_map,
    const float* opacities, const float* scales, float scale_modifier, const float* rotations,
    const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix, const float* cam_pos,
    float tan_fovx, float tan_fovy,
    const int* radii,
    void* geometry_buffer, const void* binning_buffer, const void* image_buffer,
    const float* dL_dout_color,     /* [1,H,W] */
    const float* dL_dout_invdepth,  /* [1,H,W] or NULL */
    const float* dL_dout_all_map,   /* [4,H,W] or NULL */
    float* dL_dmean2D, float* dL_dconic, float* dL_dopacity, float* dL_dcolor, float* dL_dinvdepth,
    float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscale, float* dL_drot, float* dL_dall_map,
    int antialiasing, int render_geo, int debug,
    void* stream);

/* present[i] = (view-space z of means3D[i] > 0.2); rasterizer_impl.cu:54-66 */
int cgs_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                     uint8_t* present, void* stream);

/* Byte sizes the allocation callbacks will be asked for (exposed for callers that pre-allocate). */
size_t cgs_geometry_bytes(int P);
size_t cgs_image_bytes(int width, int height);
size_t cgs_binning_bytes(int64_t R);

/* ------------------------------------------------------------------------------------------------
 * Fused per-view path of the training configuration (no counterpart in the reference, which runs ~45 PyTorch kernels and
 * three extension calls for the same work): curve parameters in, image out, and back to curve-parameter gradients.
 * Equivalent to  cgs_sample_curves_forward -> cgs_splat_attrs_forward -> cgs_rasterize_forward_static  (and their
 * backwards in reverse) with scales + rotations, precomputed colours (NULL = all ones), scale_modifier 1, no
 * antialiasing, render_geo on -- i.e. gaussian_renderer/__init__.py:18-157 as train.py calls it -- but the per-splat
 * tensors between those calls (xyz, rotation, scaling, opacity, all_map and their gradients) never leave registers:
 * 8 kernel launches per view and direction pair instead of 13.
 *   cgs_view_forward: arguments as the three calls it replaces; xyz / rotation / scaling may be NULL (all three) when the
 *     caller does not need the model's derived splat tensors.  out_invdepth and out_all_map may BOTH be NULL (only without
 *     colors_precomp): image-only forward for a training iteration, which reads `render` alone (train.py:98-107).  Status words as cgs_rasterize_forward_static.
 *     B * m < 2^28 (the tile-list entries of this path carry four tag bits for the matching cgs_view_backward; the binning
 *     buffer and the 32-byte gradient accumulator records it leaves in the geometry buffer are private to that pair of calls).
 *   cgs_view_backward: valid ONCE per cgs_view_forward (it consumes scratch sums the forward zeroed).  Only dL/dcolour
 *     flows in (train.py's loss reads `render` only); colors_precomp as given to the forward (NULL = unit colours: the
 *     compositors then use closed forms, sum w = 1 - T and dC/dalpha = (1 - bg) T_final / (1 - alpha)); dL_drotation_extra [P,4] or NULL is added to the gradient of the
 *     raw splat rotations before it is pulled back to the curves (the curve-smoothness regulariser enters there).
 *     Outputs: dL_dmeans2D [P,3] (NDC-scaled, feeds add_densification_stats), dL_dcurve_points [B,4,3], dL_dwidth [B,1],
 *     dL_dopacity_logit [B,1], dL_dmask_logit [P] (required iff mask_logit) -- overwritten, or added to when `flags`
 *     has CGS_VIEW_ACCUMULATE (several views summed into one gradient buffer without extra kernels).  scratch:
 *     cgs_view_backward_scratch_floats(B, m) floats (13 per curve are used: the part of dL/d{curve_points, width} that does not
 *     depend on the two grid-wide sums of the sampling backward, summed per curve inside the per-splat kernel; the closing
 *     pass adds the rest from the curve alone -- rounds 2-5 sent 15 floats per SPLAT through this buffer and back).
 *   cgs_view_forward_checked: the same forward for eager callers (the drop-in render(): gaussian_renderer/__init__.py:18-157
 *     as train.py:95-97 calls it).  Like the reference's forward it reports how much it binned -- but the host only waits for
 *     a 16-byte readback queued right behind the SCATTER, with the compositor already enqueued behind it (the reference blocks
 *     on num_rendered before it can even size its sort buffers, rasterizer_impl.cu:287).  Returns the longest tile list
 *     (>= 0; cgs_last_forward_stats has num_rendered): when it exceeds bucket_capacity the outputs are INVALID and the call
 *     must be repeated with a larger capacity; negative = cgs_status.  Updates the per-shape binning hints.
 *   cgs_bucket_capacity_hint: bucket capacity recommended for the next forward of this workload shape (1.25 x the longest
 *     list seen recently + 64, rounded up to 64), 0 when nothing is known about it yet.
 * ------------------------------------------------------------------------------------------------ */
int cgs_view_forward(int B, int m, const float* curve_points, const float* width, const uint8_t* is_bezier, const float* coef,
                     float eps, double* norms, const float* opacity_logit, const float* mask_logit, float mask_thr,
                     const float* colors_precomp, void* geometry_buffer, void* binning_buffer, size_t binning_bytes,
                     void* image_buffer, uint32_t bucket_capacity, const float* background, int width_px, int height_px,
                     const float* viewmatrix, const float* projmatrix, const float* cam_pos, float tan_fovx, float tan_fovy,
                     float* out_color, float* out_invdepth, float* out_all_map, int* radii, float* xyz, float* rotation,
                     float* scaling, void* stream);
int64_t cgs_view_forward_checked(int B, int m, const float* curve_points, const float* width, const uint8_t* is_bezier, const float* coef,
                     float eps, double* norms, const float* opacity_logit, const float* mask_logit, float mask_thr,
                     const float* colors_precomp, void* geometry_buffer, void* binning_buffer, size_t binning_bytes,
                     void* image_buffer, uint32_t bucket_capacity, const float* background, int width_px, int height_px,
                     const float* viewmatrix, const float* projmatrix, const float* cam_pos, float tan_fovx, float tan_fovy,
                     float* out_color, float* out_invdepth, float* out_all_map, int* radii, float* xyz, float* rotation,
                     float* scaling, void* stream);
/* The same in two halves, so that the caller can queue MORE work behind the forward before it blocks (render() queues its
 * clamp and direction-map kernels, then waits): cgs_view_forward_begin enqueues everything including the status readback and
 * returns a HANDLE (>= 0; negative: status code); cgs_view_forward_wait(handle, &n_visible) blocks on that readback, releases
 * the handle and returns what cgs_view_forward_checked returns (n_visible, optional: splats with radii > 0 -- sizes render()'s
 * visibility_filter = (radii > 0).nonzero(), gaussian_renderer/__init__.py:150, without a device-wide sync).  Any number of
 * forwards (threads, devices, streams, models) may be outstanding up to a pool of 64 status slots, which cgs_rasterize_forward
 * shares (one slot per call in progress); a slot idle on one device serves another.  A handle that will never be waited on
 * (an exception between the two halves) is returned with cgs_view_forward_abandon. */
int cgs_view_forward_begin(int B, int m, const float* curve_points, const float* width, const uint8_t* is_bezier, const float* coef,
                     float eps, double* norms, const float* opacity_logit, const float* mask_logit, float mask_thr,
                     const float* colors_precomp, void* geometry_buffer, void* binning_buffer, size_t binning_bytes,
                     void* image_buffer, uint32_t bucket_capacity, const float* background, int width_px, int height_px,
                     const float* viewmatrix, const float* projmatrix, const float* cam_pos, float tan_fovx, float tan_fovy,
                     float* out_color, float* out_invdepth, float* out_all_map, int* radii, float* xyz, float* rotation,
                     float* scaling, void* stream);
/* The view forward WITH render()'s epilogue (gaussian_renderer/__init__.py:138-145) written by the compositor itself instead of
 * a separate pass over the image (cgs_render_epilogue below): out_color_clamped [H,W] = clamp(out_color, 0, 1) beside the raw
 * out_color (torch.clamp's gradient rule needs the raw value: cgs_view_backward_render), out_rend_dir [3,H,W] = all_map[0:3]
 * taken from view to world space; either may be NULL.  Unit colours only (no colors_precomp); checked != 0: like
 * cgs_view_forward_begin (returns a handle for cgs_view_forward_wait), checked == 0: like cgs_view_forward (sync-free). */
int cgs_view_forward_render(int checked, int B, int m, const float* curve_points, const float* width, const uint8_t* is_bezier,
                            const float* coef, float eps, double* norms, const float* opacity_logit, const float* mask_logit,
                            float mask_thr, void* geometry_buffer, void* binning_buffer, size_t binning_bytes, void* image_buffer,
                            uint32_t bucket_capacity, const float* background, int width_px, int height_px, const float* viewmatrix,
                            const float* projmatrix, const float* cam_pos, float tan_fovx, float tan_fovy, float* out_color,
                            float* out_invdepth, float* out_all_map, int* radii, float* out_color_clamped, float* out_rend_dir,
                            void* stream);
int64_t cgs_view_forward_wait(int handle, int64_t* n_visible);
void cgs_view_forward_abandon(int handle);
/* ------------------------------------------------------------------------------------------------
 * The depth gate on the TRAINING render: cgs_view_forward and cgs_view_forward_render -- the two forwards every training
 * route calls -- with the occlusion rule of cgs_point_mask_depth (nv_hidden, csrc/point_projection.h) applied per splat
 * inside the fused per-splat kernel (k_view_fwd<true>, csrc/view.hip).  The edge map of a real scan of a solid has its
 * hidden lines removed; without the gate a curve on a far rim is drawn into every view that looks at it through the solid
 * and the photometric loss of those views pushes against it.  Opt-in, OFF BY DEFAULT, UNTUNED; the five ungated forwards are
 * unchanged to the bit.  cgs_view_forward_shared, cgs_view_forward_checked and cgs_view_forward_begin get NO gated sibling:
 * shared-sampling view batches are out of the gate's scope, and the checked / two-halves forms are reached through
 * cgs_view_forward_render_depth(checked != 0), which returns the handle cgs_view_forward_wait takes.
 *
 * Each entry takes the arguments of its sibling, with their meaning and their checks, plus `gate` before the stream:
 *   planes      float32 [V,height,width], device: camera z per training view, +inf where there is no surface (the planes of
 *               cgs_mesh_depth / cgs_surfel_depth / the caller's maps, usually after cgs_depth_window_max), ALL views resident
 *   intr, w2c   float64 [V,4] = (fx, fy, cx, cy) and [V,12] = [R | T] row-major, device: the cameras the planes were drawn with
 *   view_index  int32 [1], device, or NULL.  When set the kernel reads the view from it (a captured graph picks the step's
 *               plane and camera the way cgs_photometric_loss_indexed picks its ground-truth map) and `view` is ignored; a
 *               value outside [0, V) reads nothing and hides nothing
 *   slack       float64 >= 0 in the units of the planes; +inf is allowed and hides nothing
 *   V, view     the number of views in the stack and, without view_index, this forward's view in [0, V)
 *   height, width   the planes' size: it must be the image's (height_px, width_px)
 *
 * THE RULE, frozen, for splat p and the gate's view v:
 *   1. splat_geometry decides first, as in the sibling: a splat it rejects (behind the near plane, outside the frustum,
 *      degenerate) gets radius 0 and the plane is not read.
 *   2. Otherwise X = the splat's centre, the float32 sample position of the kernel (the bits of the xyz output), widened to
 *      float64, goes through the projection of cgs_point_mask_depth with view v's camera: c = R X + T with every row
 *      ((r0*X + r1*Y) + r2*Z) + t, u = fx * (c0 / c2) + cx, v = fy * (c1 / c2) + cy, float64, one rounded operation at a time.
 *   3. If c2 <= 0 or (u, v) is outside [0, width) x [0, height) the splat is visible exactly as without the gate and the plane
 *      is not read: a large splat whose centre is off the image keeps drawing.
 *   4. Otherwise the splat is HIDDEN iff c2 > (double)planes[v][floor(v)][floor(u)] + slack (a NaN entry hides nothing):
 *      radii[p] = 0 and no splat record is written; else nothing changes.
 * A hidden splat is never binned; cgs_view_backward skips radii == 0, so it receives no gradient from this view and stays out of
 * the densification statistics and the regularisers' visible set -- exactly how a frustum-culled splat is treated.  The gate
 * is piecewise constant and has no derivative of its own.  It judges the splat's CENTRE, not its footprint.  The stack is
 * indexed in size_t.  With planes that hide nothing (all +inf, or slack = +inf) every output equals the sibling's to the bit.
 *
 * CGS_ERR_INVALID_ARGUMENT, before anything is launched and with a message naming the entry that was called: a NULL gate; a NULL
 * planes / intr / w2c; V < 1; without view_index a view outside [0, V); a slack that is negative or NaN; planes whose size
 * is not the image's.  Checked after the sibling's own arguments and before the bucket capacity.
 * ------------------------------------------------------------------------------------------------ */
typedef struct cgs_view_gate {
    const float* planes;
    const double* intr;
    const double* w2c;
    const int32_t* view_index;
    double slack;
    int32_t V, view, height, width;
} cgs_view_gate;
int cgs_view_forward_depth(int B, int m, const float* curve_points, const float* width, const uint8_t* is_bezier, const float* coef,
                           float eps, double* norms, const float* opacity_logit, const float* mask_logit, float mask_thr,
                           const float* colors_precomp, void* geometry_buffer, void* binning_buffer, size_t binning_bytes,
                           void* image_buffer, uint32_t bucket_capacity, const float* background, int width_px, int height_px,
                           const float* viewmatrix, const float* projmatrix, const float* cam_pos, float tan_fovx, float tan_fovy,
                           float* out_color, float* out_invdepth, float* out_all_map, int* radii, float* xyz, float* rotation,
                           float* scaling, const cgs_view_gate* gate, void* stream);
int cgs_view_forward_render_depth(int checked, int B, int m, const float* curve_points, const float* width,
                                  const uint8_t* is_bezier, const float* coef, float eps, double* norms,
                                  const float* opacity_logit, const float* mask_logit, float mask_thr, void* geometry_buffer,
                                  void* binning_buffer, size_t binning_bytes, void* image_buffer, uint32_t bucket_capacity,
                                  const float* background, int width_px, int height_px, const float* viewmatrix,
                                  const float* projmatrix, const float* cam_pos, float tan_fovx, float tan_fovy, float* out_color,
                                  float* out_invdepth, float* out_all_map, int* radii, float* out_color_clamped,
                                  float* out_rend_dir, const cgs_view_gate* gate, void* stream);
/* Epilogue of render() on the fused route, /root/reference/gaussian_renderer/__init__.py:138-145 in one launch: color_out [H,W] =
 * clamp ? clamp(color_raw, 0, 1) : color_raw (NULL: skipped); dir_out [3,H,W] = all_map[0:3] taken from view to world space,
 * out_i = sum_k all_map[k] * viewmatrix[4 i + k] (viewmatrix = world_view_transform, row-major 4x4; NULL: skipped).
 * cgs_clamp_backward: g_out = (0 <= raw <= 1) ? g_in : 0, torch.clamp's gradient rule. */
int cgs_render_epilogue(int height, int width, const float* color_raw, const float* all_map, const float* viewmatrix, int clamp,
                        float* color_out, float* dir_out, void* stream);
int cgs_clamp_backward(int64_t n, const float* raw, const float* g_in, float* g_out, void* stream);
uint32_t cgs_bucket_capacity_hint(int P, int width, int height);
/* Number of splats with radii > 0 in the calling thread's last cgs_view_forward_checked (-1: none yet); the two-halves form
 * hands it out through cgs_view_forward_wait. */
int64_t cgs_last_forward_visible(void);
/* (radii > 0).nonzero() (gaussian_renderer/__init__.py:150) in ONE launch and without a host sync, for the radii of a CHECKED
 * forward (cgs_view_forward_checked / _begin / _render with checked != 0, or cgs_rasterize_forward on its bucket path): that
 * forward left the visible count of every 1/64th of the splats in its image buffer, and n_visible = their sum came back with
 * its status readback.  out_indices [n_visible] int64, ascending (what torch's nonzero() returns, as a column). */
int cgs_visible_indices(int P, const int* radii, const void* image_buffer, int width, int height, int64_t* out_indices, void* stream);
/* Several views of ONE parameter state (a view batch between two optimizer steps; not the reference's one-view iteration):
 * cgs_view_forward_shared is cgs_view_forward without the grid-wide norm pass of prepare_scaling_rot, and cgs_view_backward
 * with CGS_VIEW_SHARED in its flags adds its per-curve partial gradients into `scratch` and skips the closing pass of the sampling
 * backward (linear in them); the caller brackets the batch with cgs_view_shared_begin (zeroes norms and scratch, computes the
 * norms once) and cgs_view_shared_end (that last pass, once: dL/dcurve_points, dL/dwidth written or added to).  Every view of
 * the batch must use the SAME norms and scratch buffers; opacity / mask gradients keep coming from cgs_view_backward
 * (CGS_VIEW_ACCUMULATE to sum them over the batch).  The mode is chosen per call: no process-wide state. */
int cgs_view_forward_shared(int B, int m, const float* curve_points, const float* width, const uint8_t* is_bezier, const float* coef,
                     float eps, double* norms, const float* opacity_logit, const float* mask_logit, float mask_thr,
                     const float* colors_precomp, void* geometry_buffer, void* binning_buffer, size_t binning_bytes,
                     void* image_buffer, uint32_t bucket_capacity, const float* background, int width_px, int height_px,
                     const float* viewmatrix, const float* projmatrix, const float* cam_pos, float tan_fovx, float tan_fovy,
                     float* out_color, float* out_invdepth, float* out_all_map, int* radii, float* xyz, float* rotation,
                     float* scaling, void* stream);
int cgs_view_shared_begin(int B, int m, const float* curve_points, const uint8_t* is_bezier, const float* coef, double* norms,
                          float* scratch, void* stream);
int cgs_view_shared_end(int B, int m, const float* curve_points, const float* width, const uint8_t* is_bezier, const float* coef,
                        float eps, double* norms, float* scratch, float* dL_dcurve_points, float* dL_dwidth, int accumulate,
                        void* stream);
size_t cgs_view_backward_scratch_floats(int B, int m);
/* Layout of the `norms` buffer (f64 words): [0, *first) are the forward's grid-wide sums (written by the norm pass),
 * [*first, *first + *count) the two sums the sampling backward ACCUMULATES -- cleared by the forward's norm pass, so a caller that
 * runs a second backward over one forward (retain_graph) zeroes exactly this range in between.  Returns the buffer's size in words. */
int cgs_view_norms_backward_range(int* first, int* count);
/* flags of cgs_view_backward (a plain 0 / 1 keeps its old meaning: overwrite / accumulate) */
#define CGS_VIEW_ACCUMULATE 1 /* add to dL_dcurve_points, dL_dwidth, dL_dopacity_logit, dL_dmask_logit instead of writing them */
#define CGS_VIEW_SHARED 2     /* shared curve sampling of a view batch (above): per-splat gradients go to `scratch` only */
int cgs_view_backward(int B, int m, const float* curve_points, const float* width, const uint8_t* is_bezier, const float* coef,
                      float eps, double* norms, const float* opacity_logit, const float* mask_logit, float mask_thr,
                      const float* colors_precomp, void* geometry_buffer, const void* binning_buffer, const void* image_buffer, const float* background,
                      int width_px, int height_px, const float* viewmatrix, const float* projmatrix, const float* cam_pos,
                      float tan_fovx, float tan_fovy, const int* radii, const float* dL_dout_color,
                      const float* dL_drotation_extra, float* dL_dmeans2D, float* dL_dcurve_points, float* dL_dwidth,
                      float* dL_dopacity_logit, float* dL_dmask_logit, float* scratch, int flags, void* stream);
/* cgs_view_backward for an image that went through render()'s clamp: dL_dout_color is the gradient of the CLAMPED image,
 * color_raw the forward's unclamped one; the gradient counts only where 0 <= color_raw <= 1 (torch.clamp's rule), applied
 * where the compositor loads the pixel's upstream gradient -- no separate cgs_clamp_backward pass.  Unit colours only. */
int cgs_view_backward_render(int B, int m, const float* curve_points, const float* width, const uint8_t* is_bezier, const float* coef,
                      float eps, double* norms, const float* opacity_logit, const float* mask_logit, float mask_thr,
                      void* geometry_buffer, const void* binning_buffer, const void* image_buffer, const float* background,
                      int width_px, int height_px, const float* viewmatrix, const float* projmatrix, const float* cam_pos,
                      float tan_fovx, float tan_fovy, const int* radii, const float* dL_dout_color, const float* color_raw,
                      float* dL_dmeans2D, float* dL_dcurve_points, float* dL_dwidth,
                      float* dL_dopacity_logit, float* dL_dmask_logit, float* scratch, int flags, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Curve -> Gaussian sampling.  Replaces GaussianCurveModel.prepare_scaling_rot
 * (/root/reference/scene/gaussian_curve_model.py:180-198 with get_curve_gaussians :70-78, get_curve_tangent :80-89 and
 * rot_to_quat_batch, utils/general_utils.py:33-86) and its autograd backward.
 *   curve_points [B,4,3], width [B,1] (log), is_bezier [B] u8 or NULL (= all Bezier).  P = B*m, splat = b*m + i.
 *   coef [m,16] f32: per-sample weights computed by the host with the reference's float32 expressions
 *     {c0..c3 at t_i, c0..c3 at t_i-0.5/m, 3(1-t)^2, 6(1-t)t, 3t^2, (1-t), t, (1-t'), t', pad}.
 *   norms [384] f64 scratch: [0..191] = 64 partial sums each of three global sums written by the forward and needed
 *     by the backward (the two Frobenius norms of the reference's global normalisations and one cross term);
 *     [192..319] are backward scratch (cleared by the forward's norm pass; cgs_sample_curves_backward clears them itself
 *     on entry, the per-view backward of cgs_view_backward does not: ONE view backward per view forward); the rest is
 *     reserved.  The buffer needs no initialisation by the caller.
 *   outputs xyz [P,3], rotation [P,4] (w,x,y,z, un-normalised), scaling [P,3].
 * The backward accepts NULL for any upstream gradient (treated as zero).  m <= 32.
 * ------------------------------------------------------------------------------------------------ */
int cgs_sample_curves_forward(int B, int m, const float* curve_points, const float* width, const uint8_t* is_bezier,
                              const float* coef, float eps, double* norms, float* xyz, float* rotation,
                              float* scaling, void* stream);
int cgs_sample_curves_backward(int B, int m, const float* curve_points, const float* width, const uint8_t* is_bezier,
                               const float* coef, float eps, double* norms, const float* dL_dxyz,
                               const float* dL_drotation, const float* dL_dscaling, float* dL_dcurve_points,
                               float* dL_dwidth, float* scratch /* [P,9] f32, required when dL_drotation != NULL */,
                               void* stream);

/* Per-view splat attributes fed to the rasterizer (one fused kernel each way instead of ~40 PyTorch kernels):
 *   rotation_n = F.normalize(rotation_raw)                      gaussian_curve_model.py:121-122
 *   opacity    = sigmoid(opacity_logit[b]) expanded to splats    :108-110   (* mask when mask_logit != NULL)
 *   scaling_out = scaling * mask (only when mask_logit != NULL; straight-through mask,
 *                 gaussian_renderer/__init__.py:72-76); pass scaling_out = NULL otherwise
 *   all_map    = [ R(rotation_n)[:,0] flipped toward the camera @ view[:3,:3], 1 ]   :99-105, renderer :98-104
 * opacity_logit [B,1], mask_logit [B,m,1] or NULL, campos [3], viewmatrix [16] (world_view_transform, row-major). */
int cgs_splat_attrs_forward(int B, int m, const float* rotation_raw, const float* xyz, const float* opacity_logit,
                            const float* mask_logit, float mask_thr, const float* scaling, const float* campos,
                            const float* viewmatrix, float* rotation_n, float* opacity, float* scaling_out,
                            float* all_map, void* stream);
int cgs_splat_attrs_backward(int B, int m, const float* rotation_raw, const float* xyz, const float* opacity_logit,
                             const float* mask_logit, float mask_thr, const float* scaling, const float* campos,
                             const float* viewmatrix, const float* dL_drotation_n, const float* dL_dopacity,
                             const float* dL_dscaling_out, const float* dL_dall_map, float* dL_drotation_raw,
                             float* dL_dopacity_logit, float* dL_dmask_logit, float* dL_dscaling, void* stream);

/* ------------------------------------------------------------------------------------------------
 * fused-ssim.  Replaces fusedssim / fusedssim_backward (/root/reference/submodules/fused-ssim/ssim.cu:368-404,
 * :406-444; kernels :187-286, :288-366; declared in ssim.h:7-26).  img [batch, channels, H, W] f32 contiguous, zero
 * padding ("same"); the "valid" crop is done by the Python wrapper like the reference (fused_ssim/__init__.py:13-14).
 * dm_* may be NULL (train == false).
 * ------------------------------------------------------------------------------------------------ */
int cgs_ssim_forward(int batch, int channels, int height, int width, float C1, float C2, const float* img1,
                     const float* img2, float* ssim_map, float* dm_dmu1, float* dm_dsigma1_sq, float* dm_dsigma12,
                     void* stream);
int cgs_ssim_backward(int batch, int channels, int height, int width, float C1, float C2, const float* img1,
                      const float* img2, const float* dL_dmap, const float* dm_dmu1, const float* dm_dsigma1_sq,
                      const float* dm_dsigma12, float* dL_dimg1, void* stream);

/* Fused class-balanced edge loss: edge_aware_loss(image, gt_image, threshold) of
 * /root/reference/utils/loss_utils.py:94-115 (train.py:101).  image, gt [C,H,W] f32.  scratch16: 16 bytes of device
 * scratch; after the call (stream order) the f64 at scratch16+8 holds SUM (image-gt)^2 * mask, so
 * loss = that / (C*H*W); the u32 at scratch16 holds the edge-pixel count.  dL_dimage (optional) = d loss / d image. */
int cgs_edge_aware_loss(int channels, int height, int width, const float* image, const float* gt, float threshold,
                        void* scratch16, float* dL_dimage, void* stream);

/* The photometric part of the training loss (train.py:101-107) for a 1-channel render, value and gradient in ONE
 * pass of three kernels (SSIM forward, SSIM backward + edge-loss/clamp epilogue, scalar finish):
 *   loss = lambda_edge * edge_aware_loss(x, gt, threshold) + lambda_ssim * (1 - fused_ssim(x, gt)),
 *   x = clamp_input ? clamp(image, 0, 1) : image          (render()'s clamp, gaussian_renderer/__init__.py:138)
 * with lambda_edge = lambda_mse (1 - lambda_dssim), lambda_ssim = lambda_mse lambda_dssim in train.py's notation.
 * n_pos: device u32 = #{gt > threshold}, from cgs_edge_count (depends on gt only: compute once per gt image).
 * workspace: cgs_photometric_workspace_bytes(H, W) bytes, zero-filled before its FIRST use, then reusable as is, also
 * for any other H' x W' whose workspace size is not larger.
 * Outputs: dL_dimage [H*W] = d loss / d image (0 where the clamp is active), loss [1]. */
size_t cgs_photometric_workspace_bytes(int height, int width);
int cgs_edge_count(int channels, int height, int width, const float* gt, float threshold, uint32_t* n_pos, void* stream);
int cgs_photometric_loss(int height, int width, const float* image, const float* gt, float threshold,
                         const uint32_t* n_pos, float lambda_edge, float lambda_ssim, int clamp_input, void* workspace,
                         float* dL_dimage, float* loss, void* stream);
/* Same, with the target picked on the device: gt_stack [V,H,W], n_pos_table [V], *view_index (device int) selects the
 * entry.  For stream-captured training iterations (train.py:95 picks a random view per iteration): the captured launch
 * is the same for every view, no 4*H*W-byte copy of the step's edge map into a staging buffer. */
int cgs_photometric_loss_indexed(int height, int width, const float* image, const float* gt_stack, const int* view_index,
                                 float threshold, const uint32_t* n_pos_table, float lambda_edge, float lambda_ssim,
                                 int clamp_input, void* workspace, float* dL_dimage, float* loss, void* stream);

/* End-point connection loss of /root/reference/train.py:133-146 (active after opt.conn_from_iter): over the 2B curve end
 * points (first and last control point of every curve), loss = weight * mean distance of all ordered pairs of DIFFERENT
 * curves closer than distance_threshold (0.05 in the reference); 0 when there is no such pair.  The reference builds the
 * (2B)^2 cdist matrix; this is a neighbour search on a hashed uniform grid, O(B) memory and time.  curve_points [B,4,3].
 * dL_dcurve_points [B,4,3]: accumulate != 0 adds the gradient to the rows 0 and 3 (the other rows are untouched),
 * accumulate == 0 writes the whole tensor (rows 1, 2 zero).  workspace: cgs_endpoint_connection_workspace_bytes(B).
 * Coordinate range: grid cells are indexed with (int)floorf(x / (1.0001 distance_threshold)), so every end-point
 * coordinate must satisfy |x| < 2^30 distance_threshold; beyond that the cell index overflows and pairs are missed. */
size_t cgs_endpoint_connection_workspace_bytes(int B);
int cgs_endpoint_connection_loss(int B, const float* curve_points, float distance_threshold, float weight, void* workspace,
                                 float* loss, float* dL_dcurve_points, int accumulate, void* stream);

/* The per-iteration regularisers of /root/reference/train.py:113-131 (PyTorch ops over all P splats in the reference),
 * value and gradients in three launches:
 *   loss = w_opacity * gate * mean_{splats with radii > 0} log(1 + sigmoid(opacity_logit[b])^2 / 0.5)
 *        + w_smooth * [any radii > 0] * mean_{b, i < m-1} (1 - |cos(d_i, d_{i+1})|),
 *              d = column 0 of quaternion_to_matrix(normalize(rotation_raw))  (main axis of splat b*m + i)
 *        + w_width * mean_{curves with exp(width_log[b]) >= width_threshold} (exp(width_log[b]) - width_threshold)
 * Empty selections contribute 0 (the reference guards them with host-side ifs).  opacity_gate: device float or NULL
 * (= 1): train.py's `reset_timestep > 0` switch, kept on the device so a captured graph need not be re-captured.
 * rotation_raw [B*m,4] (16-byte aligned), opacity_logit [B], width_log [B], radii [B*m] int32.  workspace:
 * cgs_curve_regularizers_workspace_bytes() bytes, zero-filled before its FIRST use, then reusable as is.
 * Outputs: loss [1]; dL_drotation_raw [B*m,4], dL_dopacity_logit [B], dL_dwidth_log [B] (every element written). */
size_t cgs_curve_regularizers_workspace_bytes(void);
int cgs_curve_regularizers(int B, int m, const float* rotation_raw, const float* opacity_logit, const float* width_log,
                           const int* radii, float w_opacity, const float* opacity_gate, float w_smooth, float w_width,
                           float width_threshold, void* workspace, float* loss, float* dL_drotation_raw,
                           float* dL_dopacity_logit, float* dL_dwidth_log, void* stream);

/* One-launch Adam over a flat parameter buffer (torch.optim.Adam semantics: no weight decay, no amsgrad), replacing
 * the per-group foreach step of the reference (scene/gaussian_curve_model.py:200-213, train.py:235).
 * segments: HOST array of n_segments (<= 16) x {int64 begin; float lr; float pad}, sorted by begin,
 * segments[0].begin == 0; element i uses the lr of the last segment with begin <= i (the table is passed to the
 * kernel by value, so a per-iteration learning-rate change costs no copy).  step = 1-based step count (bias
 * correction).  zero_grads != 0 also clears grads (optimizer.zero_grad(), train.py:236) in the same pass. */
int cgs_adam_step_flat(int64_t n, float* params, float* grads, float* exp_avg, float* exp_avg_sq,
                       const void* segments, int n_segments, float beta1, float beta2, float eps, int step,
                       int zero_grads, void* stream);

/* Graph-replayable Adam: as cgs_adam_step_flat, but the per-step scalars live in DEVICE memory
 * (device_state: cgs_adam_state_bytes() bytes = 16 x {int64 begin; float lr; float pad} followed by
 * {float 1 - beta1^t; float sqrt(1 - beta2^t); float pad[2]}, refreshed by the caller with a stream-ordered copy), and
 * when skip_flag != NULL and *skip_flag != 0 (e.g. status word [2] of a cgs_rasterize_forward_static image buffer) the
 * parameters and moments are left untouched (gradients are still cleared if zero_grads). */
int cgs_adam_step_flat_dev(int64_t n, float* params, float* grads, float* exp_avg, float* exp_avg_sq,
                           const void* device_state, int n_segments, float beta1, float beta2, float eps, int zero_grads,
                           const uint32_t* skip_flag, void* stream);
/* The same step with a report for replayed iterations: report_seq (device u32, set by the caller once) counts the executions;
 * execution number n writes 1 (skipped) or 0 into report_ring[n % report_len].  report_ring may be pinned host memory mapped into
 * the device (hipHostMalloc / torch pin_memory): the host then learns about skipped iterations without a device-to-host copy
 * queued between one replay and the next -- it reads entry n once an event recorded behind replay n has completed. */
int cgs_adam_step_flat_dev_report(int64_t n, float* params, float* grads, float* exp_avg, float* exp_avg_sq,
                                  const void* device_state, int n_segments, float beta1, float beta2, float eps, int zero_grads,
                                  const uint32_t* skip_flag, uint32_t* report_seq, uint32_t* report_ring, int report_len,
                                  void* stream);
size_t cgs_adam_state_bytes(void);

/* ------------------------------------------------------------------------------------------------
 * simple-knn.  Replaces distCUDA2 -> SimpleKNN::knn (/root/reference/submodules/simple-knn/spatial.cu:15-26,
 * simple_knn.cu:186-222): mean_dist2[i] = mean of the 3 smallest SQUARED distances from point i to other points.
 * workspace: cgs_knn_workspace_bytes(P) bytes of device scratch.
 * ------------------------------------------------------------------------------------------------ */
size_t cgs_knn_workspace_bytes(int P);
int cgs_knn_mean_dist2(int P, const float* points /*[P,3]*/, float* mean_dist2 /*[P]*/, void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Exact 1-nearest-neighbour (edge evaluation).  Replaces the point_cloud_utils.k_nearest_neighbors(x, y, k=1) KD-tree
 * queries of the reference's evaluator (edge_extraction/eval_utils.py:77-115, 195-249) and its scipy cKDTree query
 * (eval_ABC.py:27-38): for every query point q[i], dist[i] = min_j |q[i] - ref[j]| and index[i] = the argmin.
 * Squared distances are the fp32 value of (dx*dx + dy*dy) + dz*dz (no FMA contraction, no GEMM expansion), brute force.
 * Ties: the LOWEST index among reference points at the same fp32 distance (duplicates are normal in ABC ground truth);
 * the result is deterministic, bit for bit.  n_query = 0 is a no-op; n_ref = 0 with n_query > 0, negative sizes, sizes
 * above 2^30 and NULL pointers are CGS_ERR_INVALID_ARGUMENT, rejected before anything is launched.
 * workspace: cgs_nn1_workspace_bytes(n_query) bytes of device scratch.
 * ------------------------------------------------------------------------------------------------ */
size_t cgs_nn1_workspace_bytes(int n_query);
int cgs_nn1(int n_query, const float* query /*[n_query,3]*/, int n_ref, const float* ref /*[n_ref,3]*/,
            float* dist /*[n_query]*/, int* index /*[n_query]*/, void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Edge-map visibility check (extraction).  Replaces the (edge, frame) loop of the reference's compute_visibility
 * (edge_extraction/extract_para_edge.py:145-197, called by get_parametric_edge(visible_checking=True) :200-249):
 * counts[e] = the number of frames f in which edge e is seen by the 2D edge detector.  Edges are the curves (4 control
 * points each) followed by the lines (2 end points each); only these points are projected, never sampled points.
 * Per frame: K[f] (row-major 3x3) and w2c[f] = inv(camtoworld)[:3,:4] (row-major 3x4, inverted on the host); each point
 * is projected in float64 as x = K (R X + T), every dot product ((a0*b0 + a1*b1) + a2*b2) + t without FMA contraction,
 * then divided by x[2] with IEEE division.  Quirks kept: no z > 0 test (a point behind the camera projects mirrored and
 * counts if it lands in the image); z = 0 gives inf / NaN and drops the point; coordinates round half to even (np.round)
 * and a point is kept if 0 <= u < width and 0 <= v < height.  The cell is 0 with no kept point, else
 * mean(values) > 0.1 && max(values) > 0.5 with the mean summed left to right in control-point order (np.mean over <= 4
 * values); values are maps[f][v][u] / 255.0, or 1 - maps[f][v][u] / 255.0 when invert = 1 (DexiNed).
 * maps: uint8 [n_frames, height, width], one byte per pixel (offsets are 64-bit: the buffer may exceed 2^31 bytes).
 * The caller applies the reference's mask, counts > ceil(0.05 * n_frames).  Counts are deterministic (integer sums).
 * n_curves + n_lines = 0 is a no-op; negative sizes, more than 2^30 edges, height or width <= 0 with n_frames > 0 and
 * NULL pointers with a non-zero size are CGS_ERR_INVALID_ARGUMENT, rejected before anything is launched.
 * ------------------------------------------------------------------------------------------------ */
int cgs_edge_visibility(int n_curves, const double* curves /*[n_curves,4,3]*/, int n_lines,
                        const double* lines /*[n_lines,2,3]*/, int n_frames, const double* K /*[n_frames,3,3]*/,
                        const double* w2c /*[n_frames,3,4]*/, int height, int width,
                        const unsigned char* maps /*[n_frames,height,width]*/, int invert, int* counts /*[E]*/,
                        void* stream);

/* ------------------------------------------------------------------------------------------------
 * Per-call options of the operator API.  The `debug` argument of cgs_rasterize_forward / cgs_rasterize_backward is a bit
 * set: bit 0 is the reference's debug flag (rasterize_points.cu:53: synchronise and check after every kernel), the bits
 * below select measurement / parity variants FOR THAT CALL ONLY -- nothing process-wide, nothing another thread's call
 * can see (rounds 1-5 had cgs_set_tile_culling / cgs_set_fused_tile_sort / cgs_set_operator_unit_route here).
 * ------------------------------------------------------------------------------------------------ */
#define CGS_OPT_DEBUG 0x1
#define CGS_OPT_NO_TILE_CULLING 0x100   /* cgs_rasterize_forward: bin like the reference (below) */
#define CGS_OPT_GENERAL_BACKWARD 0x200  /* cgs_rasterize_backward: never the unit-colour kernel (below) */
/* Tile-level culling (default on; CGS_OPT_NO_TILE_CULLING switches it off for one forward).  The reference bins a splat into EVERY tile of the
 * bounding square of radius ceil(3 sigma) (forward.cu:318-321 getRect, rasterizer_impl.cu:70-110) and lets the
 * compositor skip it per pixel when alpha < 1/255 (forward.cu:371-377).  With culling on, an instance
 * (splat, tile) is only created when the splat can reach alpha >= 1/255 at some pixel of that tile, so
 * num_rendered is smaller than the reference's while images, radii and every gradient are unchanged (the
 * dropped instances are exactly those the compositor would skip at all 256 pixels).  With culling off,
 * num_rendered and the per-tile lists are bit-identical to the reference's.
 *
 * Unit-colour route of the backward (default on; CGS_OPT_GENERAL_BACKWARD keeps the general instance for one backward): a
 * cgs_rasterize_backward that is asked for neither colour nor depth / all_map gradients (the training configuration of the
 * reference's own call, gaussian_renderer/__init__.py:96-129) lets the GPU choose between the pair-major unit-colour compositor
 * and the general one: the forward's scatter raises a word of the image buffer when some visible splat's colour or all_map[3]
 * is not exactly 1, and both kernels test it on entry (no host sync; the forward tags its tile-list entries with quadrant
 * masks whenever P < 2^28).
 *
 * The tile sort inside the forward compositor (sync-free forwards whose bucket capacity allows it) has a read-once environment
 * switch for A/B measurements: CGS_FUSED_TILE_SORT=0 -> separate per-tile sort launch.
 * ------------------------------------------------------------------------------------------------ */
/* Introspection of the calling thread's last cgs_rasterize_forward: num_rendered, the longest per-tile list and
 * which binning path produced it (0 = exact count/scan/scatter layout, 1 = single-pass fixed-capacity buckets). */
/* ------------------------------------------------------------------------------------------------
 * Sync-free forward for stream-ordered and hipGraph-captured pipelines (no counterpart in the reference, whose
 * forward blocks on a device-to-host copy of num_rendered, rasterizer_impl.cu:287).  Same inputs, outputs and saved
 * state as cgs_rasterize_forward, but:
 *   - the three buffers are allocated by the caller: cgs_geometry_bytes(P), cgs_image_bytes(W, H) and
 *     cgs_binning_bytes(bucket_capacity * tiles) bytes, tiles = ceil(W/16) * ceil(H/16);
 *   - binning is the single-pass bucket layout with `bucket_capacity` slots per tile (<= cgs_bucket_capacity_limit());
 *     a good value is 1.25-2 x the longest tile list reported by cgs_last_forward_stats after a normal forward;
 *   - nothing is read back: no num_rendered, no host wait -- the call only enqueues work on `stream`.
 * Status words (u32) at byte offset cgs_image_status_offset(W, H) of the image buffer, valid in stream order:
 *   [2] != 0: some tile list outgrew its bucket -> the image and every gradient of this forward are INVALID (redo it
 *       with cgs_rasterize_forward or a larger capacity); [4 + 2k], [5 + 2k], k < (cgs_status_words() - 4) / 2:
 *       partial sums / maxima of the tile list lengths (num_rendered = sum of the sums, longest list = max of maxima);
 *   [3]: number of splats whose tile rectangle exceeds 96 tiles (near-camera splats of room-scale scenes).  When a
 *       previous cgs_rasterize_forward of the same (P, width, height) saw any, such splats are binned by a second kernel, one workgroup
 *       each, instead of inside the wave that owns them (cgs_reset_binning_hints clears that memory too).
 *   word [cgs_status_words()] (right behind the status words) is a STICKY count of overflowed tile lists: the library only
 *       ever adds to it, so a caller that zeroes the image buffer once can replay many views and check one word at the
 *       end instead of one flag per view.
 * The backward is cgs_rasterize_backward with R = 1.
 * ------------------------------------------------------------------------------------------------ */
int cgs_rasterize_forward_static(void* geometry_buffer, void* binning_buffer, size_t binning_bytes, void* image_buffer,
                                 uint32_t bucket_capacity, int P, int D, int M, const float* background, int width,
                                 int height, const float* means3D, const float* shs, const float* colors_precomp,
                                 const float* opacities, const float* scales, float scale_modifier,
                                 const float* rotations, const float* cov3D_precomp, const float* all_map,
                                 const float* viewmatrix, const float* projmatrix, const float* cam_pos, float tan_fovx,
                                 float tan_fovy, float* out_color, float* out_invdepth, float* out_all_map,
                                 int antialiasing, int render_geo, int* radii, void* stream);
size_t cgs_image_status_offset(int width, int height);
int cgs_status_words(void);
uint32_t cgs_bucket_capacity_limit(void);

/* cgs_rasterize_forward learns, per workload shape (P, width, height), how large the previous forward of that shape was
 * (num_rendered, longest tile list, oversized splats) and sizes its speculative buffers from it; shapes do not disturb
 * each other (a process may alternate train / test cameras, resolutions or models; the 32 most recent shapes are kept).
 * This call forgets everything learnt (the next forward of every shape takes the exact path and re-learns). */
void cgs_reset_binning_hints(void);
void cgs_last_forward_stats(int64_t* num_rendered, int64_t* longest_tile_list, int* binning_path);

/* ------------------------------------------------------------------------------------------------
 * Per-kernel timing hook used by bench.py: when enabled, every kernel launched by the library is
 * bracketed by hipEvents on the caller's stream; cgs_prof_collect synchronises and accumulates.
 * ------------------------------------------------------------------------------------------------ */
void cgs_prof_enable(int on);
void cgs_prof_reset(void);
/* Fills up to `cap` entries; returns the number of distinct kernels seen.  names[i] points to static storage. */
int cgs_prof_collect(const char** names, double* total_ms, int64_t* launches, int cap);

/* ------------------------------------------------------------------------------------------------
 * Held-out image metrics (training_report, reference train.py:321-376): for each of n_views views, in one launch,
 *   sums[v] = (sum |d|, sum d^2) in float64 over c < channels, y < height, x0 <= x < width,
 *   d = clamp(image[y,x], 0, 1) - clamp(gt[c,y,x], 0, 1) computed in float32 (NaN propagates as in torch.clamp),
 * and, when `means` is not NULL, means[v] = sums[v] / (channels * height * (width - x0)).  `image` is [1,height,width]
 * (broadcast over the gt's channels), `gt` [channels,height,width], both contiguous float32; views may differ in size.
 * Deterministic: fixed slices per view, partial sums added in index order by the view's last workgroup; the bits of view
 * v depend only on view v.  No host synchronisation: the descriptor table travels with one stream-ordered copy into
 * `workspace` (cgs_view_metrics_workspace_bytes(n_views) bytes of device memory; no initialisation needed).
 * n_views = 0 is a no-op; n_views < 0 or > 65535, NULL pointers, channels / height / width <= 0 and x0 outside
 * [0, width) are CGS_ERR_INVALID_ARGUMENT, rejected before anything is launched.
 * ------------------------------------------------------------------------------------------------ */
typedef struct cgs_metric_view {
    const float* image; /* [1,height,width] */
    const float* gt;    /* [channels,height,width] */
    int channels;
    int height;
    int width;
    int x0;             /* first column (train_test_exp: width / 2) */
} cgs_metric_view;
size_t cgs_view_metrics_workspace_bytes(int n_views);
int cgs_view_metrics(int n_views, const cgs_metric_view* views /*host, [n_views]*/, void* workspace,
                     double* sums /*[n_views,2]*/, double* means /*[n_views,2] or NULL*/, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Image summaries of the training report (reference train.py:346-364): for each of n_views views, five 8-bit RGB panels
 * packed as uint8 [5, height, width, 3] at out + out_offset, in the order
 *   0 render, 1 ground_truth, 2 depth, 3 rend_dir, 4 rend_alpha.
 * Per pixel, in float32 and in this order of operations (no fused multiply-add):
 *   q(x)          = (uint8) clip(x * 255, 0, 255), truncated; q(NaN) = 0      (what a tensorboard image summary does to a
 *                   float image)
 *   render, rend_alpha, ground_truth:  q(clamp(x, 0, 1)), a one-channel value replicated to R, G, B; a gt with
 *                   gt_channels = 3 gives its channels as R, G, B
 *   depth:          m = max(0, largest non-NaN pixel of the view),  s = depth / m * 256,
 *                   i = s >= 255 ? 255 : (s > 0 ? (int)s : 0),  colour = q(turbo[i]) (csrc/turbo_table.h); a view with
 *                   m = 0 and every pixel whose s is NaN are (0, 0, 0).  PRECONDITION: depth >= 0, which is what the
 *                   rasterizer's depth map is (a blend of positive view depths over a zero background); a negative pixel
 *                   is not an error, it takes table entry 0
 *   rend_dir:       n = v / max(|v|, 1e-12) over the three channels (F.normalize(dim=0)), q(n * 0.5 + 0.5) per channel
 * Inputs are contiguous float32: render, depth, rend_alpha [1,height,width], rend_dir [3,height,width], gt
 * [gt_channels,height,width] with gt_channels 1 or 3.  Any of the five may be NULL: that panel's bytes are left untouched
 * and its bit in `written` stays clear (bit p = panel p; `written` is filled in the caller's host table before the call
 * returns).  Views may differ in size; their output ranges must not overlap.  16-byte aligned planes are read with
 * 16-byte loads and 4-byte aligned panels written 12 bytes (four pixels) per lane; anything else takes the element path,
 * with the same results.
 * Two launches for all views, nothing else: (1) every view's depth maximum as cgs_report_panels_workspace_bytes(n_views)
 * bytes of per-workgroup partial maxima in `workspace` -- every slot is rewritten by every call, so the workspace needs
 * no initialisation, and no atomics are involved; (2) the panels.  The table travels as a kernel argument: no copy, no
 * host synchronisation, and a stream capture of the call holds everything it needs.  That argument bounds n_views by
 * CGS_REPORT_MAX_VIEWS per call.  n_views = 0 is a no-op; n_views outside [0, CGS_REPORT_MAX_VIEWS], NULL table /
 * workspace / out, height or width <= 0, gt_channels other than 1 or 3 with a gt, and overlapping output ranges are
 * CGS_ERR_INVALID_ARGUMENT, rejected before anything is launched.
 * ------------------------------------------------------------------------------------------------ */
#define CGS_REPORT_MAX_VIEWS 32
#define CGS_REPORT_PANELS 5
typedef struct cgs_report_view {
    const float* render;     /* [1,height,width] or NULL */
    const float* gt;         /* [gt_channels,height,width] or NULL */
    const float* depth;      /* [1,height,width] or NULL */
    const float* rend_dir;   /* [3,height,width] or NULL */
    const float* rend_alpha; /* [1,height,width] or NULL */
    int gt_channels;         /* 1 or 3 (read only when gt is not NULL) */
    int height;
    int width;
    unsigned int written;    /* out: bit p set when panel p was written */
    size_t out_offset;       /* byte offset of this view's [5,height,width,3] block in `out` */
} cgs_report_view;
size_t cgs_report_panels_workspace_bytes(int n_views);
int cgs_report_panels(int n_views, cgs_report_view* views /*host, [n_views]*/, void* workspace, unsigned char* out,
                      void* stream);

/* ------------------------------------------------------------------------------------------------
 * Densification statistics (reference train.py:184-187, GaussianModel.add_densification_stats): for every splat i < P
 * with radii[i] > 0, in one launch,
 *   max_radii2D[i] = max(max_radii2D[i], (float)radii[i]);
 *   xyz_gradient_accum[i] += sqrt(gx*gx + gy*gy);   gx, gy = dL_dmeans2D[i * grad_stride + 0 / 1]
 *   denom[i] += 1;
 * splats with radii[i] <= 0 are not touched.  The reference indexes with the list of visible splats (a device-to-host
 * sync); here every splat is decided on the device.  One thread per splat, no atomics: deterministic, bit for bit.
 * skip_flag != NULL and *skip_flag != 0 (the convention of cgs_adam_step_flat_dev: status word [2] of a replayed
 * forward that overflowed its buckets) writes nothing.  max_radii2D [P], xyz_gradient_accum [P,1], denom [P,1] float32.
 * P = 0 is a no-op; P < 0, grad_stride < 2 and NULL pointers with P > 0 are CGS_ERR_INVALID_ARGUMENT, rejected before
 * anything is launched.
 * ------------------------------------------------------------------------------------------------ */
int cgs_densification_stats(int64_t P, const int* radii /*[P]*/, const float* dL_dmeans2D /*[P,grad_stride]*/,
                            int64_t grad_stride, float* max_radii2D /*[P]*/, float* xyz_gradient_accum /*[P]*/,
                            float* denom /*[P]*/, const uint32_t* skip_flag /*device, may be NULL*/, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Multi-view projection of extracted edges (novel views).  Replaces the per-point, per-view Python loops of the
 * reference's eval_ABC.py --render_mv (project_points_to_camera / visualize_projection :66-138) and eval_replica.py
 * (process_scan :100-212).  Cameras: intr[v] = (fx, fy, cx, cy) and w2c[v] = [R | T] (row-major 3x4), float64.
 * Projection, in float64 with the reference's operation order: X = (double)points[i], c = R X + T with every row
 * ((r0*X + r1*Y) + r2*Z) + t (no FMA contraction), dropped if c2 <= 0, u = fx * (c0 / c2) + cx, v = fy * (c1 / c2) + cy
 * (IEEE division), kept if 0 <= u < width and 0 <= v < height.
 *
 * cgs_project_points writes uv_out[v][i] = (u, v) of every kept point and (NaN, NaN) for a dropped one.  P = 0 or V = 0
 * is a no-op; negative sizes, height or width <= 0 and NULL pointers are CGS_ERR_INVALID_ARGUMENT.
 *
 * cgs_render_points draws the kept points into float32 images out[V,height,width,3]: a kept point covers pixel
 * (floor(u), floor(v)); the n points of a pixel are composited in ascending point index with constant `alpha` over
 * `background` (host, 3 values): out = bg (1-alpha)^n + sum_j alpha c_j (1-alpha)^r_j, r_j = the number of later points
 * in that pixel, in float64, rounded to float32 once.  Only the newest K points of a pixel enter the sum, K the smallest
 * k with (1-alpha)^k <= 2^-25 (25 at alpha = 0.5, 1 at alpha = 1): the terms left out add up to at most 2^-25 max|c|.
 * Deterministic (integer atomics only; the result depends only on the set of points in each pixel).  kept (device,
 * [V], may be NULL) receives the number of kept points of each view.  `workspace` is device scratch of
 * `workspace_bytes` bytes: cgs_render_points_workspace_bytes(P, V, height, width) processes every view in one pass
 * (capped at 2^31 (view, point) pairs and 65535 views per pass); less processes the views in chunks, down to
 * cgs_render_points_workspace_bytes(P, 1, height, width).  P = 0 writes the background; V = 0 is a no-op; negative
 * sizes, height or width <= 0, height * width > 2^31, alpha outside [0, 1], a workspace too small for one view and NULL
 * pointers are CGS_ERR_INVALID_ARGUMENT, rejected before anything is launched.
 * ------------------------------------------------------------------------------------------------ */
int cgs_project_points(int P, const float* points /*[P,3]*/, int V, const double* intr /*[V,4]*/,
                       const double* w2c /*[V,12]*/, int height, int width, double* uv_out /*[V,P,2]*/, void* stream);
size_t cgs_render_points_workspace_bytes(int P, int V, int height, int width);
int cgs_render_points(int P, const float* points /*[P,3]*/, const float* colors /*[P,3]*/, int V,
                      const double* intr /*[V,4]*/, const double* w2c /*[V,12]*/, int height, int width, double alpha,
                      const double* background /*host [3]*/, float* out /*[V,height,width,3]*/, int* kept /*[V]*/,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Ellipsoid mesh of the splats (GaussianCurveModel.draw_ellipsoids, the reference's scene/gaussian_curve_model.py:634-709:
 * one Open3D sphere per splat, scaled, rotated, moved, painted, merged and written with write_triangle_mesh).  The kernels
 * write the binary little-endian body of the PLY file: every splat contributes V0 vertex records of 27 bytes (double x,
 * y, z; uchar red, green, blue) and F0 face records of 13 bytes (uchar 3; int a, b, c).  At resolution r the sphere has
 * V0 = 2 + 2 r (r - 1) vertices and F0 = 4 r (r - 1) triangles (182 and 360 at r = 10).
 *
 * cgs_ellipsoid_mesh_body_bytes returns the body size of P splats (vertex_bytes + face_bytes, each stored if not NULL),
 * or -1 for P < 0, resolution outside [2, 1024], or P * V0 > 2^31 (a vertex index would not fit in an int).
 *
 * cgs_ellipsoid_mesh_vertices writes the vertex records of splats [first, first + count) to `out`: xyz [P,3], rot [P,4]
 * (w, x, y, z, used as given), scale [P,3] and rgb [P,3] are float32 device arrays indexed by the absolute splat
 * number; unit_vertices [V0,3] is the float64 sphere template with its radius applied.  Vertex k of splat i, in float64
 * without FMA contraction: p_j = unit_vertices[k][j] * (double)scale[i][j]; R = Eigen's toRotationMatrix of the quaternion;
 * every row ((r0*p0 + r1*p1) + r2*p2) + (double)xyz[i][j].  Colour: uint8(round(min(1, max(0, c)) * 255)) (half away
 * from zero; NaN gives 0).  Record r of the chunk (r = (i - first) * V0 + k) starts at byte 27 r of `out`.
 *
 * cgs_ellipsoid_mesh_faces writes the face records of splats [first, first + count): record (i - first) * F0 + k holds
 * template_faces[k] + i * V0, at byte 13 ((i - first) * F0 + k).
 *
 * Both: `out` is 16-byte aligned device memory of the chunk size rounded up to a multiple of 16 bytes; every 16-byte
 * word of it is written, the padding after the last record with zeros.  The bytes do not depend on the chunking.
 * count = 0 is a no-op; negative sizes, (first + count) * V0 > 2^31, a misaligned `out` and NULL pointers are
 * CGS_ERR_INVALID_ARGUMENT, rejected before anything is launched.
 * ------------------------------------------------------------------------------------------------ */
int64_t cgs_ellipsoid_mesh_body_bytes(int P, int resolution, int64_t* vertex_bytes, int64_t* face_bytes);
int cgs_ellipsoid_mesh_vertices(int first, int count, const float* xyz /*[P,3]*/, const float* rot /*[P,4] wxyz*/,
                                const float* scale /*[P,3]*/, const float* rgb /*[P,3]*/, int V0,
                                const double* unit_vertices /*[V0,3]*/, void* out, void* stream);
int cgs_ellipsoid_mesh_faces(int first, int count, int V0, int F0, const int* template_faces /*[F0,3]*/, void* out,
                             void* stream);

/* ------------------------------------------------------------------------------------------------
 * Line fitting and merging (GaussianCurveModel.fit_curve_to_line / merge_curves, the reference's
 * scene/gaussian_curve_model.py:459-632 over edge_extraction/fitting.py and merging.py): the data-parallel parts of the
 * two edits.  Inputs are the model's float32 tensors, all arithmetic is float64, every result is deterministic (no
 * floating-point atomics, reductions in a fixed order).  Sizes of 0 are no-ops; negative sizes, sizes above the limits
 * below, thresholds that are NaN and NULL pointers are CGS_ERR_INVALID_ARGUMENT, rejected before anything is launched.
 *
 * cgs_curve_straightness (is_curve_straight for every curve): the sample_num cubic Bernstein samples of curve b at
 * t = i / (sample_num - 1), their mean and 3x3 covariance, the unit eigenvector of its largest eigenvalue, the
 * projections t_i on it; mean_dist[b] / max_dist[b] = mean / maximum distance of the samples to the foot
 * mean + clip(t_i, min t, max t) * direction; straight[b] = is_bezier[b] && mean_dist < threshold && max_dist <
 * threshold_max.  Samples that all coincide give distances 0.  2 <= sample_num <= CGS_CURVE_FIT_MAX_SAMPLES.
 *
 * cgs_segment_merge_labels (merge_curves, straight segments): segments a < b are joined when
 * |cos(dir a, dir b)| >= similarity_threshold and min(dist(b.start, a), dist(b.end, a)) <= distance_threshold, the
 * distance of a point to segment a with its foot clipped to the segment; a segment of zero length is joined to nothing.
 * labels[i] = the smallest segment index of i's connected component, *n_components (device) = the number of components.
 * n <= CGS_SEGMENT_MERGE_MAX.  workspace: cgs_segment_merge_workspace_bytes(n) bytes of device memory (an n x
 * ceil(n / 64) bit matrix; no initialisation needed).
 *
 * cgs_pair_consensus_fit (merge_curves, Bezier pairs): for pair k the N = 2 sample_num samples of curves pairs[k][0] and
 * pairs[k][1] (in that order) are (1) searched exhaustively for the two-point line with the most points closer than
 * ransac_thresh (then the smallest sum of squared residuals, then the smallest (i, j); point pairs at distance 0 are no
 * candidates), (2) the inliers fitted by their centroid, principal direction and the extent of their projections, (3) all
 * N points ordered by their projection on that segment's direction about its midpoint (ties by index), (4) fitted by the
 * least-squares cubic Bezier at t = linspace(0, 1, N): ctrl[k] its control points, rmse[k] its root-mean-square error,
 * inliers[k] the winning count, ok[k] = rmse <= error_threshold.  A pair without a line (best count < 2) gets ok = 0,
 * rmse = 0 and zero control points.  Curve indices must lie in [0, B) (not checked: they are device data).
 * 2 <= sample_num <= CGS_CURVE_FIT_MAX_SAMPLES.
 * ------------------------------------------------------------------------------------------------ */
#define CGS_CURVE_FIT_MAX_SAMPLES 256
#define CGS_SEGMENT_MERGE_MAX 12288
int cgs_curve_straightness(int B, const float* curve_points /*[B,4,3]*/, const uint8_t* is_bezier /*[B]*/, int sample_num,
                           double threshold, double threshold_max, double* mean_dist /*[B]*/, double* max_dist /*[B]*/,
                           uint8_t* straight /*[B]*/, void* stream);
size_t cgs_segment_merge_workspace_bytes(int n);
int cgs_segment_merge_labels(int n, const float* seg /*[n,6]: start, end*/, double distance_threshold,
                             double similarity_threshold, void* workspace, int* labels /*[n]*/,
                             int* n_components /*device, [1]*/, void* stream);
int cgs_pair_consensus_fit(int B, const float* curve_points /*[B,4,3]*/, int K, const int* pairs /*[K,2]*/, int sample_num,
                           double ransac_thresh, double error_threshold, float* ctrl /*[K,4,3]*/, double* rmse /*[K]*/,
                           int* inliers /*[K]*/, uint8_t* ok /*[K]*/, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Undistortion of the edge maps of a COLMAP scan (no counterpart in the reference, which reads undistorted scans only):
 * every view's [channels,height,width] float32 image `src`, detected in a camera with lens distortion and any principal
 * point, is resampled into `dst`, the same pixel grid seen by the ideal pinhole camera with focal lengths out_fx, out_fy
 * and its principal point at (width / 2, height / 2).  One launch for all views; views may differ in size.
 * Per output pixel (i, j), coordinates in float64 in this order of operations (no fused multiply-add):
 *   x = (i + 0.5 - width / 2) / out_fx,  y = (j + 0.5 - height / 2) / out_fy,  r2 = x x + y y
 *   (xd, yd) by `model`, a COLMAP camera model id with its coefficients k[] in COLMAP's parameter order:
 *     0 SIMPLE_PINHOLE, 1 PINHOLE   xd = x, yd = y
 *     2 SIMPLE_RADIAL (k)           xd = x s, yd = y s,  s = 1 + k r2
 *     3 RADIAL (k1, k2)             xd = x s, yd = y s,  s = 1 + k1 r2 + k2 r2^2
 *     4 OPENCV (k1, k2, p1, p2)     xd = x s + 2 p1 x y + p2 (r2 + 2 x^2),  yd = y s + p1 (r2 + 2 y^2) + 2 p2 x y,  s as RADIAL
 *     6 FULL_OPENCV (k1, k2, p1, p2, k3, k4, k5, k6)   as OPENCV with
 *                                   s = (1 + k1 r2 + k2 r2^2 + k3 r2^3) / (1 + k4 r2 + k5 r2^2 + k6 r2^3)
 *   u = fx xd + cx - 0.5,  v = fy yd + cy - 0.5      (fx, fy, cx, cy: the source camera at the resolution of `src`)
 *   x0 = floor(u), y0 = floor(v), a = u - x0, b = v - y0; the four taps (x0 | x0 + 1, y0 | y0 + 1) carry the weights
 *   (1-a)(1-b), a(1-b), (1-a) b, a b, rounded to float32; a tap outside [0, width-1] x [0, height-1] reads `fill`;
 *   dst = ((w00 t00 + w01 t01) + w10 t10) + w11 t11 in float32, per channel.
 * An integer position therefore copies its pixel bit for bit.  A pixel is BLANK, and holds `fill`, unless -1 < u < width
 * and -1 < v < height: outside that range, or with a position that is not finite, no tap of non-zero weight lies inside
 * the source.  Every view's number of blank pixels is ADDED to blank_counts[v] (device, [n_views];
 * the caller zeroes it) with integer atomics, at most one per workgroup: the result does not depend on their order.
 * The table travels as a kernel argument, which bounds n_views by CGS_UNDISTORT_MAX_VIEWS per call; no copy, no host
 * synchronisation.  n_views = 0 is a no-op; n_views outside [0, CGS_UNDISTORT_MAX_VIEWS], a NULL table / blank_counts /
 * src / dst, dst == src, channels outside [1, CGS_UNDISTORT_MAX_CHANNELS], height or width <= 0, focal lengths that are
 * not positive and finite, a `fill`, principal point or coefficient that is not finite and any other model id are
 * CGS_ERR_INVALID_ARGUMENT, rejected before anything is launched.
 * ------------------------------------------------------------------------------------------------ */
#define CGS_UNDISTORT_MAX_VIEWS 24
#define CGS_UNDISTORT_MAX_CHANNELS 4
typedef struct cgs_undistort_view {
    const float* src;   /* [channels,height,width] */
    float* dst;         /* [channels,height,width], no overlap with any src */
    int channels;
    int height;
    int width;
    int model;          /* COLMAP camera model id */
    double fx, fy, cx, cy;   /* the source camera, in pixels of `src` */
    double out_fx, out_fy;   /* the pinhole camera of `dst` */
    double k[8];        /* distortion coefficients in COLMAP's order; the unused ones are ignored */
} cgs_undistort_view;
int cgs_undistort_images(int n_views, const cgs_undistort_view* views /*host, [n_views]*/, float fill,
                         int* blank_counts /*device, [n_views]*/, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Edge maps from photographs: a classical (Canny) detector with a soft response.  No counterpart in the reference, whose
 * edge maps come from a learned detector outside it; this is not one.  Two calls per batch of views, views may differ in
 * size, every table travels as a kernel argument (at most CGS_EDGE_MAX_VIEWS views per call, no host -> device copy).
 *
 * cgs_edge_gradients: pixels (uint8, [height,width,channels] interleaved, channels 1, 3 or 4; a fourth channel is ignored)
 * -> gx, gy, m, float32 [height,width] each.  All arithmetic float32, no fused multiply-add, correctly rounded divide
 * and square root:
 *   Y = ((0.299f R + 0.587f G) + 0.114f B) / 255f, or value / 255f for one channel
 *   smoothing with the 2 radius + 1 taps (host, [2 radius + 1], offset -radius first; radius 0 with the tap 1 is none):
 *     rows first, then columns, coordinates outside the image clamped, each sum accumulated from the lowest offset
 *     to the highest, starting from the first product
 *   gx = ((S(x+1,y-1) + 2 S(x+1,y)) + S(x+1,y+1)) - ((S(x-1,y-1) + 2 S(x-1,y)) + S(x-1,y+1)), times 0.25f
 *   gy = ((S(x-1,y+1) + 2 S(x,y+1)) + S(x+1,y+1)) - ((S(x-1,y-1) + 2 S(x,y-1)) + S(x+1,y-1)), times 0.25f
 *     (S: the smoothed image, coordinates clamped), m = sqrtf(gx gx + gy gy).
 * One launch for all views.  No host synchronisation.
 *
 * cgs_edge_trace: gx, gy, m (finite) -> e, float32 [height,width] in [0,1].  With ax = |gx|, ay = |gy|, T = 0.41421357f:
 *   thin != 0: the neighbour pair of a pixel is (x-1,y),(x+1,y) when ay <= T ax, else (x,y-1),(x,y+1) when ax <= T ay,
 *     else (x-1,y-1),(x+1,y+1) when gx gy > 0, else (x+1,y-1),(x-1,y+1); a neighbour outside the image has magnitude 0;
 *     m' = m iff m > m(first) and m >= m(second), else 0.  thin == 0: m' = m.
 *   candidates: m' >= low; strong: m' >= high; a candidate is kept iff its 8-connected component of candidates holds a
 *     strong pixel; e = min(m' / high, 1) for kept pixels, 0 elsewhere.
 * Launches: one classification (m' into `e`, a state byte per pixel into `state`: 0 none, 1 candidate, 2 kept), then
 * propagation rounds, each one launch that settles every 64x16 tile against its 1-pixel halo and sets *changed_flag
 * (device, one int) when a tile changed, followed by a 4-byte readback and a stream synchronisation; rounds repeat until
 * one leaves the flag 0; then one launch turns m' into e.  The set of kept pixels does not depend on the order of
 * propagation.  RETURNS the number of propagation rounds (>= 1) on success.  Not capturable into a graph.
 *
 * Both: n_views outside [1, CGS_EDGE_MAX_VIEWS], a NULL table / taps / changed_flag / image pointer, height or width
 * <= 0, channels other than 1, 3, 4, radius outside [0, CGS_EDGE_MAX_RADIUS], low <= 0, low > high or a threshold that
 * is NaN are CGS_ERR_INVALID_ARGUMENT, rejected before anything is launched.
 * ------------------------------------------------------------------------------------------------ */
#define CGS_EDGE_MAX_VIEWS 24
#define CGS_EDGE_MAX_RADIUS 12
typedef struct cgs_edge_gradient_view {
    const uint8_t* pixels;   /* [height,width,channels] */
    float* gx;               /* [height,width] */
    float* gy;
    float* m;
    int height;
    int width;
    int channels;
    int reserved;
} cgs_edge_gradient_view;
typedef struct cgs_edge_trace_view {
    const float* gx;   /* [height,width] */
    const float* gy;
    const float* m;
    float* e;          /* [height,width]; holds m' between the launches */
    uint8_t* state;    /* [height,width] bytes of scratch; no initialisation needed */
    int height;
    int width;
} cgs_edge_trace_view;
int cgs_edge_gradients(int n_views, const cgs_edge_gradient_view* views /*host, [n_views]*/,
                       const float* taps /*host, [2 radius + 1]*/, int radius, void* stream);
int cgs_edge_trace(int n_views, const cgs_edge_trace_view* views /*host, [n_views]*/, float low, float high, int thin,
                   int* changed_flag /*device, [1]*/, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Reprojection score of extracted edges: the edges projected into every camera against that camera's edge map, in pixels
 * (precision / recall / F-score at pixel tolerances, 2D accuracy / completeness).  No ground truth in 3D is needed.  The
 * reference has no counterpart.  Three entry points; masks are uint8 [V,height,width], nonzero = set, all views of a call
 * share one size.  All of them: caller's stream, no allocation, no host synchronisation.
 *
 * cgs_point_mask builds the prediction mask: mask_out[v][floor(v_px)][floor(u_px)] = 1 for every point that
 * cgs_project_points keeps in view v (the same device function: float64, the same operation order, no FMA contraction),
 * 0 elsewhere; the call zeroes the mask itself.  Points that share a pixel store the same byte: plain stores, no atomics
 * on the mask.  kept (device, [V], may be NULL) receives the number of kept points of each view (integer atomics).
 * V = 0 is a no-op, P = 0 leaves zero masks; negative sizes, height or width <= 0 and NULL pointers are
 * CGS_ERR_INVALID_ARGUMENT, rejected before anything is launched.
 *
 * cgs_edt_squared is the exact squared Euclidean distance transform: dist2_out[v][y][x] = the minimum over the set pixels
 * (x', y') of view v of (x - x')^2 + (y - y')^2, CGS_EDT_INF everywhere in a view without a set pixel.  Integer
 * arithmetic: the result is bit-identical to a brute-force minimum and does not depend on the launch geometry.  Two
 * passes: per column, the distance g to the nearest set pixel of that column (uint16, in `workspace`,
 * cgs_edt_workspace_bytes(V, height, width) bytes of device memory, no initialisation needed); per pixel, the minimum of
 * d^2 + g[x -+ d]^2 outward over d while d^2 is below the best so far.  Cost per pixel: its true distance, O(width) in a
 * view with (almost) no set pixel.  height and width lie in [1, CGS_EDT_MAX_SIZE], so a finite result is below 2^30.
 * V = 0 is a no-op; V < 0, a size outside that range and NULL pointers are CGS_ERR_INVALID_ARGUMENT, rejected before
 * anything is launched.
 *
 * cgs_edge_score_reduce reduces every view to its counts and sums.  pred_dist2 is the transform of pred_mask (the distance
 * to the nearest predicted pixel), det_dist2 that of det_mask.  tol2 (host, n_tol <= CGS_EDGE_SCORE_MAX_TOL values >= 0)
 * are squared tolerances.  Per view v:
 *   counts[v] = (n_pred, n_det, pred_hits[0 .. n_tol), det_hits[0 .. n_tol))        int64, 2 + 2 n_tol values
 *     pred_hits[t] = #{p in pred : det_dist2(p) <= tol2[t]},  det_hits[t] = #{q in det : pred_dist2(q) <= tol2[t]}
 *   sums[v]   = (sum over p in pred of sqrt((double)det_dist2(p)), sum over q in det of sqrt((double)pred_dist2(q)))
 *   both_nonempty[v] = 1 when n_pred > 0 and n_det > 0, else 0; such a view keeps n_pred and n_det and gets zero hits
 *     and zero sums.
 * Deterministic: integer counts; the float64 sums are partial sums over fixed slices of the view, added in index order by
 * the view's last workgroup (an integer counter decides which), as cgs_view_metrics does: the bits of view v depend on
 * view v's size and content only.  `workspace`: cgs_edge_score_workspace_bytes(V) bytes of device memory, no
 * initialisation needed.  V = 0 is a no-op; V < 0, a size outside [1, CGS_EDT_MAX_SIZE], n_tol outside
 * [0, CGS_EDGE_SCORE_MAX_TOL], a negative tolerance and NULL pointers are CGS_ERR_INVALID_ARGUMENT, rejected before
 * anything is launched.
 * ------------------------------------------------------------------------------------------------ */
#define CGS_EDT_INF 2147483647 /* INT32_MAX */
#define CGS_EDT_MAX_SIZE 16384
#define CGS_EDGE_SCORE_MAX_TOL 8
int cgs_point_mask(int P, const float* points /*[P,3]*/, int V, const double* intr /*[V,4]*/,
                   const double* w2c /*[V,12]*/, int height, int width, uint8_t* mask_out /*[V,height,width]*/,
                   int* kept /*[V] or NULL*/, void* stream);
size_t cgs_edt_workspace_bytes(int V, int height, int width);
int cgs_edt_squared(int V, int height, int width, const uint8_t* mask /*[V,height,width]*/, void* workspace,
                    int32_t* dist2_out /*[V,height,width]*/, void* stream);
size_t cgs_edge_score_workspace_bytes(int V);
int cgs_edge_score_reduce(int V, int height, int width, const uint8_t* pred_mask, const uint8_t* det_mask,
                          const int32_t* pred_dist2, const int32_t* det_dist2, int n_tol, const int* tol2 /*host*/,
                          void* workspace, int64_t* counts /*[V, 2 + 2 n_tol]*/, double* sums /*[V,2]*/,
                          uint8_t* both_nonempty /*[V]*/, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Multi-view voxel vote: a seed for the curves from the scan's own edge maps.  Every voxel centre of a regular grid is
 * projected into every view; a voxel records in how many views it lies inside the image and in how many of those it lands
 * within a tolerance of a detected edge pixel.  The reference has no counterpart (it seeds a fixed 15^3 grid, or the SfM
 * cloud).  There is no occlusion reasoning in these entries (cgs_ray_claims / cgs_ray_wins below refine the selection without
 * depth); cgs_voxel_votes_depth, cgs_ray_claims_depth and cgs_ray_wins_depth, documented after cgs_sample_snap_terms_depth
 * further down, are the same three held against a depth plane per view.  Both entry points: caller's stream, no allocation, no host synchronisation, no atomics, results independent of
 * the launch geometry.
 *
 * Grid: lo, step (host, float64 [3]; step = (hi - lo) / dims, formed by the caller) and dims (nx, ny, nz), each >= 1.
 * Voxel (i, j, k) has the linear index (k ny + j) nx + i (x fastest) and the centre lo + (i + 0.5) step per axis, computed
 * in float64 without FMA contraction and rounded to float32; that float32 point is projected.
 *
 * cgs_pack_near_bits: near[v][y][x] = (dist2[v][y][x] <= tol2), dist2 the cgs_edt_squared transform of a view's detected
 * mask, packed one bit per pixel into uint32 words: word w of row y holds pixels 32 w .. 32 w + 31, bit b is pixel
 * 32 w + b; the row stride is ceil(width / 32) words, padding bits are 0.  bits_out is [V, height, ceil(width / 32)]; the
 * kernel writes every word (no memset).  A view without a feature (all CGS_EDT_INF) packs to zero.  V = 0 is a no-op;
 * V < 0, tol2 < 0, a size outside [1, CGS_EDT_MAX_SIZE] and NULL pointers are CGS_ERR_INVALID_ARGUMENT, rejected before
 * anything is launched.
 *
 * cgs_voxel_votes, for voxel g over the V views of the call (intr [V,4] = (fx, fy, cx, cy), w2c [V,12] = [R | T] row-major,
 * device, float64; all views of a call share one size):
 *   seen[g] = the number of views in which the projection rule of cgs_project_points keeps the centre (the same device
 *             function, the same operation order: c2 > 0, 0 <= u < width, 0 <= v < height)
 *   hit[g]  = the number of those views whose near bit at (floor(v), floor(u)) is set
 * accumulate == 0 stores the counts, accumulate != 0 adds them to what seen / hit hold (a plain read-add-store of the
 * thread's own voxel), so a scan is voted chunk of views by chunk of views.  Counts are uint16: the caller keeps the total
 * number of views over the accumulating calls at or below CGS_SEED_MAX_VIEWS.  V = 0 with accumulate == 0 zeroes the
 * counts (intr, w2c and bits may then be NULL); V = 0 with accumulate != 0 is a no-op.  V outside [0, CGS_SEED_MAX_VIEWS],
 * a non-positive dim, more than 2^31 - 1 voxels, a size outside [1, CGS_EDT_MAX_SIZE], a non-finite lo, a non-finite or
 * non-positive step and NULL pointers are CGS_ERR_INVALID_ARGUMENT, rejected before anything is launched.
 * ------------------------------------------------------------------------------------------------ */
#define CGS_SEED_MAX_VIEWS 65535
int cgs_pack_near_bits(int V, int height, int width, const int32_t* dist2 /*[V,height,width]*/, int tol2,
                       uint32_t* bits_out /*[V,height,ceil(width/32)]*/, void* stream);
int cgs_voxel_votes(int nx, int ny, int nz, const double* lo /*host, [3]*/, const double* step /*host, [3]*/, int V,
                    const double* intr /*[V,4]*/, const double* w2c /*[V,12]*/, int height, int width,
                    const uint32_t* bits /*[V,height,ceil(width/32)]*/, int accumulate, uint16_t* seen /*[nx ny nz]*/,
                    uint16_t* hit /*[nx ny nz]*/, void* stream);

/* cgs_voxel_moments: the direction of a seed from the kept voxels around it.  keep_bits is the selection mask of the grid
 * packed like the near masks with x fastest: word w of row (j, k) holds voxels i = 32 w .. 32 w + 31, bit b is voxel
 * 32 w + b; the row stride is ceil(nx / 32) words, rows are ordered (k ny + j), padding bits are 0 -- [nz, ny, ceil(nx / 32)]
 * uint32, device.  centres is int32 [N,3], device: the centre voxel (cx, cy, cz) of every seed, inside the grid (a centre
 * outside it reads nothing and gives a zero row).  The window of a seed is every voxel q of the grid with its keep bit set
 * and |q - c|^2 <= radius^2 (an integer comparison: a ball clipped to the grid, not a cube).  With d = q - c over the
 * window, moments[s] = (m, sum dx, sum dy, sum dz, sum dx^2, sum dy^2, sum dz^2, sum dx dy, sum dx dz, sum dy dz), int32
 * [N,10]: every value is bounded by (2 radius + 1)^3 radius^2 <= 6.8e6, so the sums are exact and their order cannot
 * matter.  One wave per seed; no atomics, no float, the kernel writes every output word (no memset), the caller's stream,
 * no allocation, no host synchronisation; the result does not depend on the launch geometry.  N = 0 is a no-op.  N < 0, a
 * non-positive dim, more than 2^31 - 1 voxels, a radius outside [1, CGS_SEED_MAX_RADIUS] and NULL pointers are
 * CGS_ERR_INVALID_ARGUMENT, rejected before anything is launched. */
#define CGS_SEED_MAX_RADIUS 15
int cgs_voxel_moments(int nx, int ny, int nz, const void* keep_bits /*[nz,ny,ceil(nx/32)] uint32*/, int N,
                      const void* centres /*int32 [N,3], inside the grid*/, int radius, void* moments /*int32 [N,10]*/,
                      void* stream);

/* cgs_ray_claims / cgs_ray_wins: a ray-exclusive refinement of the vote's selection (winner take all, no depth).  The
 * voxels that the selection kept are LISTED: index is int32 [M], device, their linear indices (ascending when the caller
 * is ops/edge_seed.py; the kernels do not need an order), and support is uint16 [M], device,
 * support[m] = (hit * 65535) / seen of that voxel in integers, formed by the caller.  Grid, cameras, sizes and bits as for
 * cgs_voxel_votes.  Listed voxel m HITS in view v when the rule of cgs_voxel_votes keeps its centre and finds its near bit
 * set: the same float32 centre, the same projection (c2 > 0, 0 <= u < width, 0 <= v < height), the bit at
 * (floor(v), floor(u)) -- the same device functions, so a vote and a claim cannot land on different pixels.
 *
 * cgs_ray_claims: best[v][y][x] (uint32 [V,height,width], device) becomes the maximum of what it held and of support[m]
 * over the listed voxels that hit at pixel (x, y) of view v, by an integer atomic maximum: the result does not depend on
 * the order or on the launch geometry.  clear != 0 first zeroes best (an asynchronous memset on the caller's stream), so
 * best is 0 where no voxel hits; clear == 0 claims into what best holds (a list claimed piece by piece).
 *
 * cgs_ray_wins: wins[m] (uint16 [M], device) = the number of views in which m hits and
 * support[m] + margin >= max(best[v][y][x] over |x - px| <= window, |y - py| <= window clipped to the image), (px, py)
 * being m's pixel; the sum is formed in 32 bits.  At most (2 window + 1)^2 plain loads per hit; no atomics.
 * accumulate == 0 stores the count (every listed voxel's word is written), accumulate != 0 adds it to what wins[m] holds
 * (a plain read-add-store of the thread's own word), so a scan is refined chunk of views by chunk of views; the caller keeps
 * the views of the accumulating calls at or below CGS_SEED_MAX_VIEWS.  best must hold the claims of ALL listed voxels for
 * the views of the call.
 *
 * Both: one thread per listed voxel, the caller's stream, no allocation, no host synchronisation.  An index outside
 * [0, nx ny nz) is the caller's error: the kernels read nothing for it, it claims nothing and its wins are 0.  M = 0 or
 * V = 0 is a no-op apart from the requested clear (pointers that the call does not touch may then be NULL).  M < 0, V
 * outside [0, CGS_SEED_MAX_VIEWS], a window outside [0, CGS_SEED_MAX_WINDOW], a margin outside [0, 65535], a non-positive
 * dim, more than 2^31 - 1 voxels, a size outside [1, CGS_EDT_MAX_SIZE], a non-finite lo, a non-finite or non-positive step
 * and NULL pointers are CGS_ERR_INVALID_ARGUMENT, rejected before anything is launched or cleared. */
#define CGS_SEED_MAX_WINDOW 4
int cgs_ray_claims(int nx, int ny, int nz, const double* lo /*host, [3]*/, const double* step /*host, [3]*/, int M,
                   const int32_t* index /*[M]*/, const uint16_t* support /*[M]*/, int V, const double* intr /*[V,4]*/,
                   const double* w2c /*[V,12]*/, int height, int width, const uint32_t* bits /*[V,height,ceil(width/32)]*/,
                   int clear, uint32_t* best /*[V,height,width]*/, void* stream);
int cgs_ray_wins(int nx, int ny, int nz, const double* lo /*host, [3]*/, const double* step /*host, [3]*/, int M,
                 const int32_t* index /*[M]*/, const uint16_t* support /*[M]*/, int V, const double* intr /*[V,4]*/,
                 const double* w2c /*[V,12]*/, int height, int width, const uint32_t* bits /*[V,height,ceil(width/32)]*/,
                 const uint32_t* best /*[V,height,width]*/, int window, int margin, int accumulate, uint16_t* wins /*[M]*/,
                 void* stream);

/* ------------------------------------------------------------------------------------------------
 * Per-edge 2D support: every extracted edge checked along its length against every view's detected edge pixels.  The
 * reference's visibility check (cgs_edge_visibility) looks at a curve's four control points or a line's two end points;
 * this counts the edge's own samples.  The reference has no counterpart.
 *
 * points is float32 [P,3], device: the samples of all edges, edge after edge.  offsets is int32 [E+1], device,
 * non-decreasing with offsets[0] = 0 and offsets[E] = P: edge e owns the points offsets[e] .. offsets[e+1] - 1 (the kernel
 * clips both ends to [0, P], so offsets that break the contract read nothing out of bounds).  Cameras as for
 * cgs_point_mask: intr [V,4] = (fx, fy, cx, cy) and w2c [V,12] = [R | T] row-major, device, float64; all views of a call
 * share one size.  d2 is int32 [V,height,width], device: the cgs_edt_squared transform of every view's detected mask.
 * tol2 is int32 [T], device, 1 <= T <= CGS_EDGE_SUPPORT_MAX_TOL: squared tolerances.
 *
 * counts is int32 [E,V,1+T], device.  A point is SEEN in view v when the projection rule of cgs_project_points keeps it
 * (the same device function, the same operation order, no FMA contraction, IEEE division: c2 > 0, 0 <= u < width,
 * 0 <= v < height).
 *   counts[e][v][0]     = the number of seen points of edge e
 *   counts[e][v][1 + t] = the number of seen points with d2[v][floor(v)][floor(u)] <= tol2[t]
 * One wave per (edge, view); integers only, no atomics, no LDS, no barrier: the result does not depend on the launch
 * geometry.  The kernel writes every output word (no memset); an edge without points gives a zero row.  The caller's
 * stream, no allocation, no host synchronisation.  E = 0 or V = 0 is a no-op (nothing to write).  E, P or V < 0, T outside
 * [1, CGS_EDGE_SUPPORT_MAX_TOL], a size outside [1, CGS_EDT_MAX_SIZE] and NULL pointers (points only when P > 0) are
 * CGS_ERR_INVALID_ARGUMENT, rejected before anything is launched.
 * ------------------------------------------------------------------------------------------------ */
#define CGS_EDGE_SUPPORT_MAX_TOL 4
int cgs_edge_support(int E, int P, const float* points /*[P,3]*/, const int32_t* offsets /*[E+1]*/, int V,
                     const double* intr /*[V,4]*/, const double* w2c /*[V,12]*/, int height, int width,
                     const int32_t* d2 /*[V,height,width]*/, int T, const int32_t* tol2 /*[T]*/,
                     int32_t* counts /*[E,V,1+T]*/, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Per-sample 2D support: the tally of cgs_edge_support the other way round -- per SAMPLE over the views -- so that an edge
 * can be trimmed to the spans of its length that the images show (ops/edge_trim.py).  The reference has no counterpart.
 *
 * points, intr, w2c, d2 and tol2 as for cgs_edge_support (no offsets: a sample does not know its edge); SEEN is the same
 * device function, so no two entries disagree on a boundary point.  tally is int32 [P,1+T], device:
 *   tally[i][0]     += the number of the V views that see sample i
 *   tally[i][1 + t] += the number of those with d2[v][floor(v)][floor(u)] <= tol2[t]
 * The entry ADDS: the caller hands in a zeroed tally and calls once per chunk of views (all views of a call share one
 * size).  One thread per sample with the view loop inside it (any number of views in one launch), the sums in registers
 * and one read-modify-write of the thread's own row: integers only, no atomics, no LDS, no barrier, so the result does not
 * depend on the launch geometry or on how the views are cut into calls.  Offsets are 64-bit.  The caller's stream, no
 * allocation, no clearing, no host synchronisation.
 *
 * Every argument is checked, whether or not there is work: P or V < 0, T outside [1, CGS_EDGE_SUPPORT_MAX_TOL], a size
 * outside [1, CGS_EDT_MAX_SIZE] and NULL pointers (points and tally only when P > 0) are CGS_ERR_INVALID_ARGUMENT, rejected
 * before anything is launched.  Then P = 0 or V = 0 is a no-op (nothing to add).
 * ------------------------------------------------------------------------------------------------ */
int cgs_sample_support(int P, const float* points /*[P,3]*/, int V, const double* intr /*[V,4]*/,
                       const double* w2c /*[V,12]*/, int height, int width, const int32_t* d2 /*[V,height,width]*/, int T,
                       const int32_t* tol2 /*[T]*/, int32_t* tally /*[P,1+T]*/, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Which samples of the extracted edges a longer edge already covers: the pieces of a chord that runs along a real edge
 * duplicate that edge, and ops/edge_dedupe.py drops them.  An all-pairs, sample-against-sample test in 3D; the reference has
 * no counterpart.
 *
 * points is float32 [P,3], device, finite, as ``sample_edges`` gives it: edge e owns points[offsets[e]:offsets[e+1]];
 * offsets is int32 [E+1], device, non-decreasing from 0 to P (NOT checked here: it lives on the device; the ops layer
 * checks it); rank is int32 [E], device, a permutation of 0..E-1, rank 0 the edge that outranks all others.
 *
 * The rule, frozen.  Every operation is one IEEE fp32 operation in the written order, nothing is contracted into an FMA,
 * so numpy float32 arrays reproduce it bit for bit.  Sample i is sample k of the n samples of edge a; sample j lies on
 * edge b:
 *   t_i = points[offsets[a] + min(k + 1, n - 1)] - points[offsets[a] + max(k - 1, 0)]      (0 on an edge of one sample)
 *   q_i = (t.x*t.x + t.y*t.y) + t.z*t.z
 *   j COVERS i iff  rank[b] < rank[a]                                                      (strict: never its own edge)
 *              and  (dx*dx + dy*dy) + dz*dz <= tol2,      dx = p_i.x - p_j.x, ...
 *              and  dot*dot >= (cos2 * q_i) * q_j,        dot = (t_i.x*t_j.x + t_i.y*t_j.y) + t_i.z*t_j.z
 *   cover[i] = the minimum of rank[b] over the samples j that cover i, INT32_MAX when there is none
 * A zero tangent makes the direction test 0 >= 0, which passes.  tol2 and cos2 are the squares, formed once by the caller.
 *
 * cover is int32 [P], device; the call writes every word (no initialisation needed).  workspace is
 * cgs_sample_cover_workspace_bytes(P) bytes of device scratch, no initialisation needed.  A first kernel writes per sample
 * its tangent and rank and per tile of 256 samples the bounding box and the rank range; the second tests 256 queries per
 * workgroup against tiles of 256 candidates staged through LDS, skips a tile whose ranks cannot outrank a query or whose
 * box lies further than the tolerance from the queries' box (a conservative test: csrc/edge_dedupe.hip), splits the
 * candidates over grid.y and merges with an integer atomic minimum -- the result does not depend on the launch geometry.
 * Offsets are 64-bit.  The caller's stream, no allocation, no host synchronisation.
 *
 * Every argument is checked, whether or not there is work: P or E < 0, tol2 negative or NaN, cos2 outside [0, 1] or NaN
 * and NULL pointers (points and cover only when P > 0) are CGS_ERR_INVALID_ARGUMENT, rejected before anything is launched.
 * Then P = 0 or E = 0 is a no-op (nothing is written).
 * ------------------------------------------------------------------------------------------------ */
size_t cgs_sample_cover_workspace_bytes(int P);
int cgs_sample_cover(int P, const float* points /*[P,3]*/, int E, const int32_t* offsets /*[E+1]*/,
                     const int32_t* rank /*[E]*/, float tol2, float cos2, int32_t* cover /*[P]*/, void* workspace,
                     void* stream);

/* ------------------------------------------------------------------------------------------------
 * Where the ends of the extracted edges land on other edges: trimming and deduping cut edges short of their junctions, and
 * ops/edge_join.py rejoins them.  A test of all ends against all samples in 3D, with a direction; the reference's
 * merge_endpoints knows only end point against end point inside one ball.
 *
 * points is float32 [P,3], device, finite, as ``sample_edges`` gives it: edge e owns points[offsets[e]:offsets[e+1]];
 * offsets is int32 [E+1], device, non-decreasing from 0 to P (NOT checked here: it lives on the device; the ops layer
 * checks it).
 *
 * The rule, frozen.  Every operation is one IEEE fp32 operation in the written order, nothing is contracted into an FMA,
 * so numpy float32 arrays reproduce it bit for bit.  Edge e with n >= 1 samples has end 2e at its first sample and end
 * 2e+1 at its last; an edge without samples has no end.  For an end of edge a at sample i with point p:
 *   t = points[i] - points[inner],  inner = i + min(1, n-1) for the first end, i - min(1, n-1) for the last   (outward)
 *   q = (t.x*t.x + t.y*t.y) + t.z*t.z,  rq = reach2*q,  tq = tol2*q                   (an edge of one sample: t = 0, q = 0)
 * Sample j of edge b, with w = points[j] - p, w2 = (w.x*w.x + w.y*w.y) + w.z*w.z and s = (w.x*t.x + w.y*t.y) + w.z*t.z,
 * is ACCEPTED iff b != a and one of
 *   NEAR  w2 <= tol2                                            (the ball of merge_endpoints, any direction)
 *   TUBE  s > 0 and s*s <= rq and (w2*q) - (s*s) <= tq          (ahead, at most reach along the tangent, tolerance beside)
 *   ENDS  j is the first or the last sample of b, s > 0 and w2 <= reach2    (another edge's end ahead within reach)
 *   keys[end] = the minimum over the accepted samples of (uint64(bits(w2)) << 32) | uint32(j); 2^64 - 1 when there is none
 * and for the two ends of an edge without samples.  tol2 and reach2 are the squares, formed once by the caller.
 *
 * keys is uint64 [2E], device; the call writes every word (no initialisation needed).  workspace is
 * cgs_end_attach_workspace_bytes(P, E) bytes of device scratch, no initialisation needed.  A first kernel writes per
 * sample (x, y, z, edge and end flag) and per end its record; the second tests 256 ends per workgroup against tiles of 256
 * samples staged through LDS, splits the samples over grid.y and merges with a 64-bit atomic minimum -- the result does
 * not depend on the launch geometry.  Offsets are 64-bit.  The caller's stream, no allocation, no host synchronisation.
 *
 * Every argument is checked, whether or not there is work: P or E < 0, tol2 or reach2 negative or NaN and NULL pointers
 * (points only when P > 0, keys only when E > 0) are CGS_ERR_INVALID_ARGUMENT, rejected before anything is launched.
 * Then E = 0 is a no-op (nothing is written); with P = 0 every key is written as 2^64 - 1.
 * ------------------------------------------------------------------------------------------------ */
size_t cgs_end_attach_workspace_bytes(int P, int E);
int cgs_end_attach(int P, const float* points /*[P,3]*/, int E, const int32_t* offsets /*[E+1]*/, float tol2, float reach2,
                   uint64_t* keys /*[2E]*/, void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Parallel binary thinning of detected masks: a learned detector's response is several pixels wide, and the 2D checks above
 * (reprojection score, voxel vote, per-edge support) were designed on one-pixel lines.  The reference has no counterpart.
 *
 * The rule is Guo-Hall two-subiteration thinning (Guo & Hall, CACM 1989), frozen.  The state is a binary image; pixels
 * outside the image read as 0.  The neighbours of (y, x): P2 = (y-1, x), P3 = (y-1, x+1), P4 = (y, x+1), P5 = (y+1, x+1),
 * P6 = (y+1, x), P7 = (y+1, x-1), P8 = (y, x-1), P9 = (y-1, x-1).
 *   C  = (!P2 & (P3|P4)) + (!P4 & (P5|P6)) + (!P6 & (P7|P8)) + (!P8 & (P9|P2))
 *   N1 = (P9|P2) + (P3|P4) + (P5|P6) + (P7|P8),  N2 = (P2|P3) + (P4|P5) + (P6|P7) + (P8|P9),  N = min(N1, N2)
 *   m  = (P6 | P7 | !P9) & P8 in sub-iteration 0,  (P2 | P3 | !P5) & P4 in sub-iteration 1
 *   a set pixel is cleared iff C == 1 and 2 <= N <= 3 and m == 0
 * Every pixel of a sub-iteration decides from the state before that sub-iteration; one iteration is sub-iteration 0 followed
 * by sub-iteration 1; the result is the state after the first iteration that changes nothing in any view.  max_iterations
 * = n > 0 stops after n iterations, or sooner when the state has settled; 0 runs until it has.
 *
 * masks is uint8 [V,height,width], device, in: nonzero = set, out: 0 / 1.  scratch is a second buffer of that size, no
 * initialisation needed; the result is in masks whichever buffer the last pass wrote.  A PASS is one launch that performs up
 * to CGS_THIN_PASS_ITERATIONS iterations on tiles of CGS_THIN_TILE_WIDTH x CGS_THIN_TILE_HEIGHT pixels held in LDS with a
 * halo of two pixels per iteration; integers and booleans only, so the result is exact and does not depend on the tile, the
 * iterations per pass or the launch geometry.  changed_flag (device, [1], no initialisation needed) receives per pass the
 * last iteration of that pass in which a pixel changed (an integer atomic maximum, at most one per wave), 0 when none did.
 * iterations_out (host, may be NULL) receives the number of iterations the rule ran: the one that changed nothing counts,
 * so a settled input gives 1.  The call returns the number of passes (>= 1 when V > 0).
 *
 * The caller's stream, no allocation.  The call SYNCHRONISES the stream once per pass to read the flag, as cgs_edge_trace
 * does; all views of a call share one size and settle together.  Offsets are 64-bit; more views than one grid dimension
 * holds go in several launches.  V = 0 is a no-op (returns 0, iterations_out 0).  V < 0, a size outside
 * [1, CGS_EDT_MAX_SIZE], max_iterations < 0 and NULL pointers are CGS_ERR_INVALID_ARGUMENT, rejected before anything is
 * launched.
 * ------------------------------------------------------------------------------------------------ */
#define CGS_THIN_PASS_ITERATIONS 4
#define CGS_THIN_TILE_WIDTH 48
#define CGS_THIN_TILE_HEIGHT 240
int cgs_thin_masks(int V, int height, int width, uint8_t* masks /*[V,height,width], in: nonzero = set, out: 0/1*/,
                   uint8_t* scratch /*[V,height,width], no initialisation needed*/, int* changed_flag /*device, [1]*/,
                   int max_iterations /*0: until stable*/, int* iterations_out /*host, may be NULL*/, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Orientation-aware 2D support: cgs_sample_support asks whether a projected sample lies near a detected pixel, not whether
 * the edge runs the way the detected edge runs, so a chord that crosses a real edge collects support at the crossing.  These
 * three entries give every detected pixel an orientation, gather the orientations over the tolerance disk, and tally per
 * sample with the direction of the sample's own edge held against them (ops/edge_orient.py; opt-in: trim_edges
 * (oriented=True)).  The reference has no counterpart.  The rule, frozen -- integers, and float64 one rounded operation at
 * a time, so the numpy back end agrees on every bit:
 *
 * octant(a, b) for (a, b) != (0, 0): the half-open octant of the doubled angle, by signs and one comparison of magnitudes
 *   a >  0, b >= 0:  0 if |b| < |a| else 1          a <  0, b <= 0:  4 if |b| < |a| else 5
 *   a <= 0, b >  0:  2 if |b| > |a| else 3          a >= 0, b <  0:  6 if |b| > |a| else 7
 * Bin k is a line orientation in [22.5 k, 22.5 (k + 1)) degrees, x to the right and y down: a horizontal line gives 0, the
 * line y = x gives 2, a vertical line 4, the line y = -x gives 6.
 *
 * cgs_mask_orientation: code[v][y][x], uint8, from view v's mask (nonzero = set; pixels outside the image are unset).  An
 * unset pixel gets 0.  For a set pixel, over the set pixels of its window (dx, dy) in [-R, R]^2, R = CGS_ORIENT_RADIUS = 3:
 *   N = sum 1, Sx = sum dx, Sy = sum dy, Sxx = sum dx dx, Syy = sum dy dy, Sxy = sum dx dy
 *   A = N Sxx - Sx Sx,  B = N Sxy - Sx Sy,  C = N Syy - Sy Sy,  a = A - C,  b = 2 B
 *   ORIENTED iff N >= 3 and (a, b) != (0, 0) and 4 (a a + b b) >= (A + C)(A + C)          (a coherence of at least 0.5)
 *   code = 1 << octant(a, b) when oriented, else 0xFF: it accepts every direction (lone pixels, junctions, blobs, strokes
 *   wider than about 3 pixels).  A + C <= 49 * 392 and a a + b b <= (A + C)^2, so 4 (a a + b b) < 2^31.
 * One workgroup per tile of CGS_ORIENT_TILE_WIDTH x CGS_ORIENT_TILE_HEIGHT pixels, the tile and its halo staged in LDS once,
 * separable sums, every output byte written by its one owner (no initialisation needed), no atomics.
 *
 * cgs_oriented_near: near[v][y][x] = the OR of code[v][y + dy][x + dx] over dx dx + dy dy <= tol2 (inside the image),
 * 0 <= tol2 <= CGS_ORIENT_MAX_TOL2 = CGS_EDGE_SUPPORT_MAX_TOL^2.  near != 0 iff the cgs_edt_squared transform of the mask is
 * <= tol2: the oriented path needs no distance transform.  Same tiles; every output byte written.  code and near must not
 * overlap: a tile reads its halo from code while its neighbours write near, so overlapping ranges are rejected.
 *
 * cgs_sample_support_oriented: points, intr, w2c and SEEN as for cgs_sample_support.  partner is int32 [P], device: the
 * neighbour on its edge that gives sample i a direction (ops.edge_orient.sample_partners: i + 1, i - 1 for the last sample
 * of an edge, i for an edge of one sample).  For a sample seen in view v at (u, v), the accepted orientations are
 *   acc = 0xFF                       if partner[i] == i, or partner[i] lies outside [0, P), or the partner is not seen in v
 *   else with dx = u_p - u, dy = v_p - v, a = dx dx - dy dy, b = 2 (dx dy)    (float64, each operation rounded, this order)
 *   acc = 0xFF                       if (a, b) == (0, 0)
 *   acc = the bits (octant(a, b) + s) mod 8 for s = -spread .. spread,  0 <= spread <= CGS_ORIENT_MAX_SPREAD = 4 (all bits)
 *   tally[i][0] += the number of the V views that see sample i
 *   tally[i][1] += the number of those with (near[v][floor(v)][floor(u)] & acc) != 0
 * spread = 1 accepts every pair of orientations nearer than 22.5 degrees and refuses every pair further than 45.  tally is
 * int32 [P,2], device; the entry ADDS, like cgs_sample_support.  One thread per sample with the view loop inside it, the
 * partner's point read once, one read-modify-write of the thread's own row: no atomics, no LDS, no barrier, 64-bit offsets.
 *
 * All three run on the caller's stream with no allocation and no host synchronisation, and their results do not depend on
 * the launch geometry or on how the views are cut into calls.  Every argument is checked, whether or not there is work: V or
 * P < 0, a size outside [1, CGS_EDT_MAX_SIZE], tol2 outside [0, CGS_ORIENT_MAX_TOL2], spread outside
 * [0, CGS_ORIENT_MAX_SPREAD], NULL pointers (points, partner and tally only when P > 0) and overlapping code and near are
 * CGS_ERR_INVALID_ARGUMENT, rejected before anything is launched.  Then V = 0 (or P = 0) is a no-op.
 * ------------------------------------------------------------------------------------------------ */
#define CGS_ORIENT_RADIUS 3
#define CGS_ORIENT_MAX_TOL2 16
#define CGS_ORIENT_MAX_SPREAD 4
#define CGS_ORIENT_TILE_WIDTH 64
#define CGS_ORIENT_TILE_HEIGHT 32
int cgs_mask_orientation(int V, int height, int width, const uint8_t* mask /*[V,height,width]*/,
                         uint8_t* code /*[V,height,width]*/, void* stream);
int cgs_oriented_near(int V, int height, int width, const uint8_t* code /*[V,height,width]*/, int tol2,
                      uint8_t* near /*[V,height,width]*/, void* stream);
int cgs_sample_support_oriented(int P, const float* points /*[P,3]*/, const int32_t* partner /*[P]*/, int V,
                                const double* intr /*[V,4]*/, const double* w2c /*[V,12]*/, int height, int width,
                                const uint8_t* near /*[V,height,width]*/, int spread, int32_t* tally /*[P,2]*/,
                                void* stream);

/* ------------------------------------------------------------------------------------------------
 * Snapping extracted edges onto the detected edges: per SAMPLE, over the views, the 3x3 normal equations of "move me onto
 * the nearest detected edge in every image" (ops/edge_snap.py solves them per sample on the host and refits each edge's
 * own control points).  The reference has no counterpart.
 *
 * points, intr, w2c and d2 as for cgs_sample_support, SEEN the same device function.  cap2 = floor(capture_px^2) lies in
 * [1, CGS_SNAP_MAX_CAP2]; dist_lut is float64 [cap2 + 1], device, dist_lut[k] = sqrt(k) computed ON THE HOST: the kernel
 * takes no square root.  terms is float64 [P, CGS_SNAP_TERMS], device, a row = (Axx, Axy, Axz, Ayy, Ayz, Azz, bx, by, bz,
 * rr); views is int32 [P], device.  The rule, frozen -- float64, one rounded operation at a time in the written order,
 * nothing contracted into an FMA, IEEE division; R = w2c's rotation (R_jk = w2c[4 j + k]), and for a view that sees the
 * sample (c0, c1, c2), x = c0 / c2, y = c1 / c2, u and v are the values of the projection:
 *   a = u - 0.5, b = v - 0.5, j0 = floor(a), i0 = floor(b)
 *   the view is SKIPPED unless 0 <= j0, j0 + 1 <= width - 1, 0 <= i0, i0 + 1 <= height - 1   (a plane under 2 x 2: never)
 *   k00, k01, k10, k11 = d2[v][i0][j0], d2[v][i0][j0 + 1], d2[v][i0 + 1][j0], d2[v][i0 + 1][j0 + 1]
 *   the view is SKIPPED unless 0 <= k <= cap2 for all four    (CGS_EDT_INF included; compared BEFORE dist_lut is indexed)
 *   d00 .. d11 = dist_lut[k00] .. dist_lut[k11],  fa = a - j0, fb = b - i0, ga = 1 - fa, gb = 1 - fb
 *   r  = gb * (ga * d00 + fa * d01) + fb * (ga * d10 + fa * d11)
 *   gu = gb * (d01 - d00) + fb * (d11 - d10),  gv = ga * (d10 - d00) + fa * (d11 - d01)
 *   su = (gu * fx) / c2,  sv = (gv * fy) / c2,  gc = -(su * x + sv * y)
 *   g_k = (R_0k * su + R_1k * sv) + R_2k * gc                                         for k = x, y, z
 *   Axx += gx * gx, Axy += gx * gy, Axz += gx * gz, Ayy += gy * gy, Ayz += gy * gz, Azz += gz * gz
 *   bx += gx * r, by += gy * r, bz += gz * r, rr += r * r, views += 1
 * r is the bilinear distance to the nearest detected pixel at the sample's image point, in pixels, g its gradient with
 * respect to the world point.  The entry ADDS: one thread per sample loads its own row and view count first, adds view by
 * view in view order and stores them -- one owner per row, no atomics -- so a row is the same floating-point sequence
 * however the views are cut into calls, and so on every launch geometry.  The table is staged in LDS behind the kernel's
 * one barrier, which every thread reaches.  Offsets are 64-bit.  The caller's stream, no allocation, no clearing, no host
 * synchronisation.
 *
 * Every argument is checked, whether or not there is work: P or V < 0, cap2 outside [1, CGS_SNAP_MAX_CAP2], a size outside
 * [1, CGS_EDT_MAX_SIZE] and NULL pointers (points, terms and views only when P > 0) are CGS_ERR_INVALID_ARGUMENT, rejected
 * before anything is launched.  Then P = 0 or V = 0 is a no-op (nothing to add).
 * ------------------------------------------------------------------------------------------------ */
#define CGS_SNAP_MAX_CAP2 64
#define CGS_SNAP_TERMS 10
int cgs_sample_snap_terms(int P, const float* points /*[P,3]*/, int V, const double* intr /*[V,4]*/,
                          const double* w2c /*[V,12]*/, int height, int width, const int32_t* d2 /*[V,height,width]*/,
                          int cap2, const double* dist_lut /*[cap2+1]*/, double* terms /*[P,CGS_SNAP_TERMS]*/,
                          int32_t* views /*[P]*/, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Occlusion for the 2D operators: a triangle mesh rendered into one camera-z plane per view (a z-buffer), the plane widened
 * by a window maximum, and the prediction mask of cgs_point_mask gated by it (ops/edge_occlusion.py).  The reference has no
 * counterpart.  intr, w2c as for cgs_point_mask.  Every rule is frozen -- float64, one rounded operation at a time in the
 * written order, nothing contracted into an FMA, IEEE division -- so that the numpy back end agrees on every bit.
 *
 * cgs_mesh_depth: tris is float32 [F,3,3], device (triangle, vertex, xyz); depth is float32 [V,height,width], device.  The
 * entry fills depth with +inf and then, for every (triangle, view):
 *   the vertices widened to float64, c = R X + T in the operation order of cgs_project_points; z_k = c2 of vertex k
 *   the triangle is SKIPPED in the view unless z_k > 0 for all three (NaN included): there is no clipping
 *   u_k = fx * (c0 / c2) + cx, v_k = fy * (c1 / c2) + cy, the projection's values, with no in-frame test
 *   the triangle is SKIPPED if any u_k or v_k is NaN
 *   area = (u1 - u0) * (v2 - v0) - (v1 - v0) * (u2 - u0); the triangle is SKIPPED if area is 0 or NaN
 *   pixel (j, i) has its centre at (px, py) = (j + 0.5, i + 0.5); the CANDIDATES are jlo <= j <= jhi, ilo <= i <= ihi with
 *     jlo = min(max(ceil(min(u0, u1, u2) - 0.5), 0), width)        jhi = max(min(floor(max(u0, u1, u2) - 0.5), width - 1), -1)
 *     ilo = min(max(ceil(min(v0, v1, v2) - 0.5), 0), height)       ihi = max(min(floor(max(v0, v1, v2) - 0.5), height - 1), -1)
 *     all in float64 (min and max of three taken left to right), converted to int after the clamp: the pixel centres inside
 *     the vertices' bounding box, its border included, inside the image
 *   e0 = (u2 - u1) * (py - v1) - (v2 - v1) * (px - u1)       (the directed side opposite vertex 0, at the pixel centre)
 *   e1 = (u0 - u2) * (py - v2) - (v0 - v2) * (px - u2)
 *   e2 = (u1 - u0) * (py - v0) - (v1 - v0) * (px - u0)       (area is e2 at vertex 2)
 *   the pixel is COVERED iff e0, e1, e2 are all >= 0 or all <= 0: both windings, borders inclusive, no fill rule
 *   w_k = e_k / area,  invz = (w0 / z0 + w1 / z1) + w2 / z2,  z = (float)(1 / invz)           (perspective correct)
 *   depth[v][i][j] = min(depth[v][i][j], z) if z is a positive finite float; otherwise nothing is stored
 * The minimum is an integer atomic minimum on the float's bit pattern (non-negative floats order like their bits).  A pixel
 * on a side shared by two triangles is covered by both, which is harmless under a minimum.  The result does not depend on
 * the launch geometry or on the order of the triangles.  Limits: a triangle with a vertex at or behind the camera plane is
 * dropped whole, not clipped (cgs_mesh_depth_clipped below clips it); each (triangle, view) costs its bounding box.
 *
 * cgs_depth_window_max: out[v][i][j] = the maximum of depth[v][i + di][j + dj] over |di|, |dj| <= radius inside the image,
 * 0 <= radius <= CGS_DEPTH_MAX_WINDOW.  +inf (no surface) wins: after it a sample is hidden only if EVERY pixel around its
 * own has a surface in front, which keeps the samples of a silhouette edge.  A NaN never wins (the planes of cgs_mesh_depth
 * hold none).  Every output word is written.  depth and out must not overlap: a tile reads its halo from depth while its
 * neighbours write out, so overlapping ranges are rejected.
 *
 * cgs_point_mask_depth: cgs_point_mask with the gate.  points, mask_out, kept as there; depth is float32 [V,height,width],
 * device, camera z, +inf where there is no surface; hidden is int32 [V], device, or NULL.  mask_out, kept and hidden are
 * cleared first.  A sample is SEEN in a view by the rule of cgs_project_points (the same device function, which here also
 * returns c2).  A seen sample is HIDDEN iff
 *   c2 > (double)depth[v][floor(v_px)][floor(u_px)] + slack                      (one float64 addition; slack finite, >= 0)
 * -- the one occlusion rule, the device function nv_hidden of csrc/point_projection.h.  A seen sample that is not hidden
 * stores the byte 1 at its pixel and counts in kept[v]; a hidden one stores nothing and counts in hidden[v].  With an
 * all-+inf plane the outputs are those of cgs_point_mask.
 *
 * All three run on the caller's stream with no allocation and no host synchronisation.  Every argument is checked, whether
 * or not there is work: F, P or V < 0, a size outside [1, CGS_EDT_MAX_SIZE], a radius outside [0, CGS_DEPTH_MAX_WINDOW], a
 * slack that is negative, NaN or infinite, NULL pointers (tris only when F > 0, points only when P > 0; kept and hidden may
 * be NULL) and overlapping depth and out are CGS_ERR_INVALID_ARGUMENT, rejected before anything is launched.  Then V = 0 is
 * a no-op.
 * ------------------------------------------------------------------------------------------------ */
#define CGS_DEPTH_MAX_WINDOW 4
int cgs_mesh_depth(int F, const float* tris /*[F,3,3]*/, int V, const double* intr /*[V,4]*/, const double* w2c /*[V,12]*/,
                   int height, int width, float* depth /*[V,height,width]*/, void* stream);
int cgs_depth_window_max(int V, int height, int width, int radius, const float* depth /*[V,height,width]*/,
                         float* out /*[V,height,width]*/, void* stream);
int cgs_point_mask_depth(int P, const float* points /*[P,3]*/, int V, const double* intr /*[V,4]*/,
                         const double* w2c /*[V,12]*/, int height, int width, const float* depth /*[V,height,width]*/,
                         double slack, uint8_t* mask_out /*[V,height,width]*/, int32_t* kept /*[V]*/,
                         int32_t* hidden /*[V]*/, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The depth gate on the four per-sample 2D operators of the extraction chain: cgs_edge_support, cgs_sample_support,
 * cgs_sample_support_oriented and cgs_sample_snap_terms, each with the occlusion rule of cgs_point_mask_depth.  Opt-in; the
 * ungated entries above are unchanged to the bit.  Each entry takes the arguments of its sibling, with their meaning, plus
 *   depth   float32 [V,height,width], device: camera z per view, +inf where there is no surface (cgs_mesh_depth followed by
 *           cgs_depth_window_max, or the caller's own maps); height and width are those of d2 / near
 *   slack   float64, finite and >= 0, in the units of depth
 * THE RULE, the same in all four: a (sample, view) pair that the projection rule of cgs_project_points keeps -- the same
 * device function, which here also returns the camera-space depth c2 -- is HIDDEN iff
 *   c2 > (double)depth[v][floor(v_px)][floor(u_px)] + slack                      (one float64 addition, one comparison)
 * -- the device function nv_hidden of csrc/point_projection.h, the one statement of the rule.  A hidden pair counts as NOT
 * SEEN: everything the sibling does for a seen pair is skipped, and the pair counts in the entry's hidden counter instead.
 * A NaN depth hides nothing.  Seen and hidden of a gated entry always add up to seen of its sibling; with an all-+inf depth
 * the outputs are the sibling's, and hidden is zero.
 *
 * cgs_edge_support_depth: counts int32 [E,V,1+T] is WRITTEN, every word, like the sibling's: counts[e][v][0] = the samples of
 * edge e that view v sees and does not hide, counts[e][v][1+t] = those of them within tolerance t.  hidden is int32 [E,V],
 * device, or NULL: hidden[e][v] = the samples of edge e that view v sees and hides, WRITTEN (not added to), every word.
 *
 * cgs_sample_support_depth: tally int32 [P,1+T]; the entry ADDS, like its sibling: tally[i][0] += the views that see sample
 * i and do not hide it, tally[i][1+t] += those of them within tolerance t.  hidden is int32 [P], device, or NULL:
 * hidden[i] += the views that see sample i and hide it -- ADDED to, like the tally, so that one call per chunk of views
 * accumulates both.
 *
 * cgs_sample_support_oriented_depth: tally int32 [P,2] and hidden int32 [P] or NULL, both ADDED to as above.  ONLY THE
 * SAMPLE ITSELF IS GATED.  The partner gives a direction and nothing else: it is projected by the projection rule alone
 * and is NEVER tested against depth -- a partner behind a surface still gives its direction, exactly as a partner that
 * the sibling would use.  (A partner the projection does not keep gives no direction, as in the sibling.)
 *
 * cgs_sample_snap_terms_depth: terms float64 [P,10], views int32 [P] and hidden int32 [P] or NULL, all ADDED to.  A hidden
 * pair contributes NO TERM AND NO VIEW: the view is left right after the projection's verdict, before the footprint test,
 * and counts in hidden[i] whether or not its footprint would have captured the sample.  For every other view the
 * floating-point sequence is exactly the sibling's, view by view in view order into the sample's own row, so the sums do
 * not depend on how the views are cut into calls and both back ends agree on every bit.
 *
 * Geometry as the siblings': one wave per (edge, view) for cgs_edge_support_depth, one thread per sample with the view loop
 * inside for the other three -- each kernel is the sibling's own body instantiated with the gate; integers or uncontracted
 * float64, no atomics, one owner per output row, so no result depends on the launch geometry.  The gate costs one float32
 * gather per seen pair.  All four run on the caller's stream with no allocation and no host synchronisation.  Every
 * argument is checked as the sibling checks it, and in addition a slack that is negative, NaN or infinite and a NULL
 * depth are CGS_ERR_INVALID_ARGUMENT, rejected before anything is launched (hidden may be NULL).
 * LIMITS, those of the rule: no near-plane clipping in the z-buffer that usually draws depth; along a concave edge samples of
 * a visible edge can be hidden by their own faces; the window and the slack that make depth are the caller's, and untuned.
 * ------------------------------------------------------------------------------------------------ */
int cgs_edge_support_depth(int E, int P, const float* points /*[P,3]*/, const int32_t* offsets /*[E+1]*/, int V,
                           const double* intr /*[V,4]*/, const double* w2c /*[V,12]*/, int height, int width,
                           const int32_t* d2 /*[V,height,width]*/, int T, const int32_t* tol2 /*[T]*/,
                           const float* depth /*[V,height,width]*/, double slack, int32_t* counts /*[E,V,1+T]*/,
                           int32_t* hidden /*[E,V]*/, void* stream);
int cgs_sample_support_depth(int P, const float* points /*[P,3]*/, int V, const double* intr /*[V,4]*/,
                             const double* w2c /*[V,12]*/, int height, int width, const int32_t* d2 /*[V,height,width]*/,
                             int T, const int32_t* tol2 /*[T]*/, const float* depth /*[V,height,width]*/, double slack,
                             int32_t* tally /*[P,1+T]*/, int32_t* hidden /*[P]*/, void* stream);
int cgs_sample_support_oriented_depth(int P, const float* points /*[P,3]*/, const int32_t* partner /*[P]*/, int V,
                                      const double* intr /*[V,4]*/, const double* w2c /*[V,12]*/, int height, int width,
                                      const uint8_t* near /*[V,height,width]*/, int spread,
                                      const float* depth /*[V,height,width]*/, double slack, int32_t* tally /*[P,2]*/,
                                      int32_t* hidden /*[P]*/, void* stream);
int cgs_sample_snap_terms_depth(int P, const float* points /*[P,3]*/, int V, const double* intr /*[V,4]*/,
                                const double* w2c /*[V,12]*/, int height, int width, const int32_t* d2 /*[V,height,width]*/,
                                int cap2, const double* dist_lut /*[cap2+1]*/, const float* depth /*[V,height,width]*/,
                                double slack, double* terms /*[P,10]*/, int32_t* views /*[P]*/, int32_t* hidden /*[P]*/,
                                void* stream);

/* ------------------------------------------------------------------------------------------------
 * The depth gate on the edge vote: cgs_voxel_votes, cgs_ray_claims and cgs_ray_wins (above, beside cgs_pack_near_bits), each
 * with the occlusion rule of cgs_point_mask_depth.  Opt-in; the ungated entries are unchanged to the bit.  Why: a voxel on a
 * rim projects into every view and is detected only where the rim is visible, so on a scan with its hidden lines removed the
 * views that look at it through the solid count in seen and hit / seen never reaches a sensible ratio.  Each entry takes the
 * arguments of its sibling, with their meaning, plus -- after the last per-view input --
 *   depth   float32 [V,height,width], device: camera z per view, +inf where there is no surface (cgs_mesh_depth followed by
 *           cgs_depth_window_max, or the caller's own maps); height and width are those of bits
 *   slack   float64, finite and >= 0, in the units of depth.  The point that is held against depth is the voxel's CENTRE,
 *           which can lie half a voxel diagonal behind the surface that carries the edge: the slack is the caller's, and a
 *           sample's slack (2 x the sampling step) is far too tight for a voxel
 * THE RULE is the one of the four entries above: a (centre, view) pair that the projection keeps -- the float32 centre of
 * cgs_voxel_votes, the same device function, the same operation order -- is HIDDEN iff
 *   c2 > (double)depth[v][floor(v_px)][floor(u_px)] + slack                      (one float64 addition, one comparison)
 * (nv_hidden, csrc/point_projection.h).  A hidden pair counts as NOT SEEN: its near bit is not read.  A NaN depth hides
 * nothing; with an all-+inf depth the outputs are the sibling's.
 *
 * cgs_voxel_votes_depth: seen[g] = the views that keep the centre and do not hide it, hit[g] = those of them whose near bit
 * is set, hidden[g] = the views that keep the centre and hide it: uint16 [nx ny nz], device, or NULL.  All three follow
 * `accumulate` (stored, or added to what they hold).  seen + hidden is the sibling's seen, voxel for voxel.  V = 0 as in the
 * sibling: with accumulate == 0 the counts (hidden too, when given) are zeroed and intr, w2c, bits and depth may be NULL; with
 * accumulate != 0 it is a no-op.
 *
 * cgs_ray_claims_depth / cgs_ray_wins_depth: a listed voxel HITS in a view only if the view does not hide it -- hidden, it
 * claims nothing there and wins nothing there.  A voxel hidden in every view leaves best untouched and has 0 wins.  best of
 * cgs_ray_wins_depth must be the gated claims of all listed voxels for the same depth and slack.  clear, accumulate, M = 0
 * and V = 0 as in the siblings.
 *
 * The three kernels are the siblings' own bodies -- one walk over the views, shared by the three and instantiated with the
 * gate, so a vote, a claim and a win cannot disagree on a pixel or a verdict; integers on uncontracted float64, no atomics
 * beyond the sibling's integer maximum, no result depends on the launch geometry.  The gate costs one float32 gather per kept
 * pair and saves a hidden pair its gather from the masks.  Caller's stream, no allocation, no host synchronisation.  Every
 * argument is checked as the sibling checks it; in addition a slack that is negative, NaN or infinite and -- where the
 * sibling needs bits -- a NULL depth are CGS_ERR_INVALID_ARGUMENT, rejected before anything is launched or cleared.
 * LIMITS, those of the rule: no near-plane clipping in the z-buffer that usually draws depth; a voxel on a concave edge lies
 * behind both of its faces in the views that see it at a grazing angle; the window and the slack are untuned, checked on the
 * drawn solids of scene/solid_scan.py only.  cgs_voxel_moments and cgs_pack_near_bits have no gate (neither walks the views
 * of a voxel), and cgs_edge_visibility, the control-point check, is ungated unless its sibling cgs_edge_visibility_depth
 * (below) is called instead.
 * ------------------------------------------------------------------------------------------------ */
int cgs_voxel_votes_depth(int nx, int ny, int nz, const double* lo /*host, [3]*/, const double* step /*host, [3]*/, int V,
                          const double* intr /*[V,4]*/, const double* w2c /*[V,12]*/, int height, int width,
                          const uint32_t* bits /*[V,height,ceil(width/32)]*/, const float* depth /*[V,height,width]*/,
                          double slack, int accumulate, uint16_t* seen /*[nx ny nz]*/, uint16_t* hit /*[nx ny nz]*/,
                          uint16_t* hidden /*[nx ny nz] or NULL*/, void* stream);
int cgs_ray_claims_depth(int nx, int ny, int nz, const double* lo /*host, [3]*/, const double* step /*host, [3]*/, int M,
                         const int32_t* index /*[M]*/, const uint16_t* support /*[M]*/, int V, const double* intr /*[V,4]*/,
                         const double* w2c /*[V,12]*/, int height, int width,
                         const uint32_t* bits /*[V,height,ceil(width/32)]*/, const float* depth /*[V,height,width]*/,
                         double slack, int clear, uint32_t* best /*[V,height,width]*/, void* stream);
int cgs_ray_wins_depth(int nx, int ny, int nz, const double* lo /*host, [3]*/, const double* step /*host, [3]*/, int M,
                       const int32_t* index /*[M]*/, const uint16_t* support /*[M]*/, int V, const double* intr /*[V,4]*/,
                       const double* w2c /*[V,12]*/, int height, int width,
                       const uint32_t* bits /*[V,height,ceil(width/32)]*/, const uint32_t* best /*[V,height,width]*/,
                       const float* depth /*[V,height,width]*/, double slack, int window, int margin, int accumulate,
                       uint16_t* wins /*[M]*/, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The depth gate on the control-point visibility check and on the drawn views: cgs_edge_visibility, cgs_project_points and
 * cgs_render_points, each with the occlusion rule of cgs_point_mask_depth (nv_hidden, csrc/point_projection.h).  Opt-in,
 * UNTUNED, checked on the drawn solids of scene/solid_scan.py only; the ungated entries are unchanged to the bit.  Each entry
 * takes the arguments of its sibling, with their meaning, plus
 *   depth   float32 [F or V,height,width], device: camera z per frame, +inf where there is no surface
 *   slack   float64, finite and >= 0, in the units of depth
 *
 * cgs_edge_visibility_depth.  THE RULE, frozen -- float64, one rounded operation at a time, nothing contracted into an FMA:
 *   c = w2c X with every row ((m0*X + m1*Y) + m2*Z) + t and x = K c with every row (k0*c0 + k1*c1) + k2*c2, as the sibling;
 *   the raw coordinates are ur = x0 / x2, vr = x1 / x2; the camera depth is c2, the third row of w2c X, NOT x2
 *   the sibling keeps a point when its ROUNDED pixel (rint(ur), rint(vr)) is in the image: that test stays as it is, and the
 *   edge map is still read at the rounded pixel
 *   a kept point is HIDDEN iff  ur >= 0 && vr >= 0 && c2 > (double)depth[f][floor(vr)][floor(ur)] + slack
 * The plane is read at the FLOORED pixel, the convention the planes are drawn in (a pixel's centre is (j + 0.5, i + 0.5)): the
 * two conventions differ by up to one pixel, which the window maximum that usually follows cgs_mesh_depth covers.  A point
 * kept by rounding with ur or vr in [-0.5, 0) has no plane pixel and is never hidden; rint(ur) <= width - 1 implies
 * floor(ur) <= width - 1, so there is no upper test.  A point behind the camera (c2 <= 0; the sibling keeps it, mirrored: the
 * reference's quirk) is never hidden by a positive plane.  A NaN plane entry hides nothing.  A hidden point is dropped exactly
 * as an out-of-image point is: it enters neither the sum, the maximum nor the number of points of its (edge, frame) cell, and a
 * cell whose points are all hidden is 0.  counts_out is int32 [E,2], device, E = n_curves + n_lines, zeroed by a kernel and
 * then WRITTEN: counts_out[e][0] = the frames in which edge e is visible, counts_out[e][1] = the frames in which the gate
 * dropped at least one of its points.  On 0 / 255 maps counts_out[e][0] never exceeds the sibling's count (a cell is visible
 * iff some kept point reads 255; dropping points cannot create one); with an all-+inf depth it is the sibling's count and
 * counts_out[e][1] is 0.  The kernel is the sibling's body instantiated with the gate: two register counters, at most two
 * integer atomicAdds per (edge, slice of frames), deterministic.  With K a pinhole matrix (no skew, K22 == 1), (ur, vr) is the
 * image point the planes of cgs_mesh_depth are drawn for; for any other K the caller's planes must be in K's image.
 *
 * cgs_project_points_depth: uv_out as the sibling's, and (NaN, NaN) also for a point the view hides.  hidden_out is uint8
 * [V,P], device, or NULL: 1 iff the projection kept the point and the gate hid it, WRITTEN, every byte.
 *
 * cgs_render_points_depth: a hidden point is dropped -- it is in no pixel's list, in neither the count pass nor the fill pass
 * (both take the verdict from the same device function on the same data).  Hidden means dropped: nothing is drawn dashed or
 * dimmed.  kept[v] stays "points in the image" that are drawn; hidden is int32 [V], device, or NULL: the points view v keeps
 * and hides, cleared by a kernel and tallied in the count pass; kept[v] + hidden[v] is the sibling's kept[v].  The workspace
 * is the sibling's (cgs_render_points_workspace_bytes): the lists can only get shorter.  The result does not depend on how the
 * workspace cuts the views into chunks; with an all-+inf depth it is the sibling's image to the bit.
 *
 * Every argument is checked as the sibling checks it, and in addition a slack that is negative, NaN or infinite and a NULL
 * depth are CGS_ERR_INVALID_ARGUMENT, rejected before anything is launched.  Caller's stream, no allocation, no host
 * synchronisation.  LIMITS, those of the rule (see cgs_point_mask_depth): the window and the slack are the caller's.
 * ------------------------------------------------------------------------------------------------ */
int cgs_edge_visibility_depth(int n_curves, const double* curves /*[n_curves,4,3]*/, int n_lines,
                              const double* lines /*[n_lines,2,3]*/, int n_frames, const double* K /*[n_frames,3,3]*/,
                              const double* w2c /*[n_frames,3,4]*/, int height, int width,
                              const unsigned char* maps /*[n_frames,height,width]*/, int invert,
                              const float* depth /*[n_frames,height,width]*/, double slack, int32_t* counts_out /*[E,2]*/,
                              void* stream);
int cgs_project_points_depth(int P, const float* points /*[P,3]*/, int V, const double* intr /*[V,4]*/,
                             const double* w2c /*[V,12]*/, int height, int width, const float* depth /*[V,height,width]*/,
                             double slack, double* uv_out /*[V,P,2]*/, uint8_t* hidden_out /*[V,P] or NULL*/, void* stream);
int cgs_render_points_depth(int P, const float* points /*[P,3]*/, const float* colors /*[P,3]*/, int V,
                            const double* intr /*[V,4]*/, const double* w2c /*[V,12]*/, int height, int width,
                            const float* depth /*[V,height,width]*/, double slack, double alpha,
                            const double* background /*host, [3]*/, float* out /*[V,height,width,3]*/, int* kept /*[V] or NULL*/,
                            int* hidden /*[V] or NULL*/, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Occluding contours of a triangle mesh: the edges along which a view sees a smooth surface turn away, drawn into one uint8
 * mask per view (ops/mesh_contours.py).  A contour is an edge in every image and an edge nowhere in 3D; this entry predicts
 * where a view has one.  The reference has no counterpart.  intr, w2c as for cgs_point_mask.
 *
 * edges is float32 [E,4,3], device: rows (a, b, c, d), (a, b) a mesh edge shared by exactly two triangles and c, d those
 * triangles' third vertices.  WHICH edges are candidates (the smooth ones, or all) is the caller's choice: the entry sees
 * only the selected rows.  depth is float32 [V,height,width], device, camera z, +inf where there is no surface (usually
 * cgs_mesh_depth followed by cgs_depth_window_max), or NULL: no gate, and slack is not read.  mask_out is uint8
 * [V,height,width], device; the entry clears it first.  E = 0 only clears.
 *
 * THE RULE, frozen -- float64, one rounded operation at a time in the written order, nothing contracted into an FMA, IEEE
 * division -- for every (row, view):
 *   the twelve floats widened to float64; A, B, C, D = R X + T of a, b, c, d in the operation order of cgs_project_points
 *   (the device function nv_camera_xyz of csrc/point_projection.h)
 *   the row is SKIPPED in the view unless A2 > 0 and B2 > 0 (NaN included): there is no clipping at the camera plane
 *   m = A x B:  m0 = A1 * B2 - A2 * B1,  m1 = A2 * B0 - A0 * B2,  m2 = A0 * B1 - A1 * B0
 *   sc = (m0 * C0 + m1 * C1) + m2 * C2,  sd = (m0 * D0 + m1 * D1) + m2 * D2
 *   the row is a CONTOUR iff sc * sd > 0: both triangles lie on the same side of the plane through the eye and the edge.
 *     The test does not depend on the triangles' winding or on the order of c and d; an edge-on triangle (a zero) and a NaN
 *     are no contour
 *   (ua, va), (ub, vb) = fx * (X0 / X2) + cx, fy * (X1 / X2) + cy of A and B (nv_image_uv), with no in-frame test
 *   du = ub - ua,  dv = vb - va
 *   THE CLIP of the segment (ua, va) + t (du, dv), t in [t0, t1], to 0 <= u <= width, 0 <= v <= height: t0 = 0, t1 = 1, then
 *   for (p, q) = (-du, ua), (du, width - ua), (-dv, va), (dv, height - va) in this order:
 *     p == 0:  the row draws nothing if q < 0
 *     p <  0:  r = q / p;  the row draws nothing if r > t1;  t0 = r if r > t0
 *     p >  0:  r = q / p;  the row draws nothing if r < t0;  t1 = r if r < t1
 *   (a NaN p or q fails every comparison and changes nothing)
 *   dt = t1 - t0,  len = max(|dt * du|, |dt * dv|);  the row draws nothing unless len <= width + height (a NaN fails)
 *   n = (int)ceil(2 * len): THE STEPS are k = 0 .. n, at most half a pixel apart on either axis, so two consecutive steps
 *   never lie in pixels that are not 8-neighbours
 *   step k:  f = k / n (0 when n = 0),  t = t0 + dt * f,  u = ua + t * du,  v = va + t * dv
 *     dropped unless 0 <= u < width and 0 <= v < height (the projection's in-frame test; this test, not the clip, keeps
 *     the store inside the plane -- the clip bounds n)
 *     with depth:  z = 1 / ((1 - t) / A2 + t / B2)   (1/z is linear along the image segment, as in cgs_mesh_depth);
 *       dropped if z > (double)depth[v][floor(v)][floor(u)] + slack -- the one occlusion rule, nv_hidden
 *     a kept step stores the byte 1 at mask_out[view][floor(v)][floor(u)]
 * A byte store of a constant is idempotent: no atomics, and the result does not depend on the order of the rows or on the
 * launch geometry (one lane classifies one row of a view; a wave ballot gives the contours among 64 rows and the whole wave
 * draws each of them, its lanes striding over the steps).
 *
 * Runs on the caller's stream with no allocation and no host synchronisation.  Every argument is checked, whether or not
 * there is work: E or V < 0, a size outside [1, CGS_EDT_MAX_SIZE], with a depth plane a slack that is negative, NaN or
 * infinite, and NULL pointers (edges only when E > 0; depth may be NULL) are CGS_ERR_INVALID_ARGUMENT, rejected before
 * anything is launched.  Then V = 0 is a no-op.
 * LIMITS: no near-plane clipping (a row with an end at or behind the camera plane is skipped whole;
 * cgs_mesh_contours_clipped below clips it); boundary edges of an
 * open mesh have one triangle and are never rows; the silhouette edges of a general triangulation zigzag across its facets.
 * ------------------------------------------------------------------------------------------------ */
int cgs_mesh_contours(int E, const float* edges /*[E,4,3]*/, int V, const double* intr /*[V,4]*/,
                      const double* w2c /*[V,12]*/, int height, int width, const float* depth /*[V,height,width] or NULL*/,
                      double slack, uint8_t* mask_out /*[V,height,width]*/, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Near-plane clipping for the two mesh entries: occluders seen from INSIDE (a room, a coarse proxy mesh whose large
 * triangles reach behind the camera plane while most of them fills the image).  Opt-in siblings: cgs_mesh_depth and
 * cgs_mesh_contours are untouched.  near is in the camera's units (world units), finite and > 0.  A camera-space point is
 * IN iff its c2 >= near; a NaN c2 is OUT.
 *
 * THE CUT, frozen -- float64, one rounded operation at a time in the written order, nothing contracted into an FMA, IEEE
 * division -- of an edge is ALWAYS taken from its IN end a toward its OUT end b:
 *   t = (a2 - near) / (a2 - b2)
 *   p0 = a0 + t * (b0 - a0),  p1 = a1 + t * (b1 - a1),  p2 = near            (p2 is assigned, not computed)
 * so two triangles that share a straddling edge compute the same point to the bit and no crack opens between them.  (One
 * device function, near_cut of csrc/mesh_depth.h, serves both entries.)
 *
 * cgs_mesh_depth_clipped: cgs_mesh_depth with one step between the camera transform and the projection.  For every
 * (triangle, view):
 *   C_k = R X_k + T of the three vertices (nv_camera_xyz); a NaN in any coordinate of any C_k SKIPS the triangle
 *   three IN:  the triangle goes on unchanged -- exactly the bits of cgs_mesh_depth
 *   none IN:   the triangle is SKIPPED
 *   one IN, at index i:       a = i, b = (i+1)%3, c = (i+2)%3;  the piece is (a, cut(a,b), cut(a,c))
 *   two IN, the OUT one at i: c = i, a = (i+1)%3, b = (i+2)%3;  the pieces are (a, b, cut(b,c)) and (a, cut(b,c), cut(a,c))
 *   every piece then runs through the set-up and the pixel rule of cgs_mesh_depth unchanged, with its three camera-space
 *   vertices: z_k = c2 (> 0 or skipped), u_k, v_k, the NaN and area tests, the candidate box (clamped in float64 before the
 *   conversion: a clipped piece often has image coordinates of 1e4 and more), coverage, the perspective-correct depth and
 *   the integer atomic minimum
 * The minimum still makes the plane independent of the launch geometry and of the order of the triangles and pieces.
 *
 * cgs_mesh_contours_clipped: cgs_mesh_contours with the ends A, B of a row clipped.  For every (row, view):
 *   A, B, C, D as there; the row is SKIPPED when neither A nor B is IN
 *   the contour test sc * sd > 0 is unchanged and uses the UNCLIPPED A, B, C, D
 *   a row with one end OUT has that end replaced by the cut from the IN end toward it, before nv_image_uv
 *   the clip to the image, the steps, and the per-step depth z = 1 / ((1 - t) / A2 + t / B2) use the clipped ends
 *   a row with both ends IN produces the bytes of cgs_mesh_contours
 *
 * CONSEQUENCE.  The projection rule and nv_hidden are not touched: a sample with 0 < c2 < near is still SEEN by
 * cgs_project_points and can only be hidden by a surface at c2 >= near -- the part of the mesh nearer than the plane is cut
 * away and hides nothing.  With every vertex of every triangle IN (any camera outside the mesh, farther than near from it)
 * both entries equal their siblings bit for bit.
 *
 * The arguments are checked as the siblings check theirs, plus one: near that is NaN, infinite or <= 0 is
 * CGS_ERR_INVALID_ARGUMENT.  Every check happens before anything is launched; then V = 0 is a no-op.  Same stream rules: no
 * allocation, no host synchronisation.  Limits: only the near plane -- the side planes of the frustum need no clip (the
 * candidate box clamps them); each piece costs its bounding box, which for a clipped piece is usually the whole image.
 * ------------------------------------------------------------------------------------------------ */
int cgs_mesh_depth_clipped(int F, const float* tris /*[F,3,3]*/, int V, const double* intr /*[V,4]*/,
                           const double* w2c /*[V,12]*/, int height, int width, double near,
                           float* depth /*[V,height,width]*/, void* stream);
int cgs_mesh_contours_clipped(int E, const float* edges /*[E,4,3]*/, int V, const double* intr /*[V,4]*/,
                              const double* w2c /*[V,12]*/, int height, int width,
                              const float* depth /*[V,height,width] or NULL*/, double slack, double near,
                              uint8_t* mask_out /*[V,height,width]*/, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Occlusion from an oriented point cloud: every point drawn as a disk (a "surfel") into the camera-z planes that
 * cgs_mesh_depth draws a mesh into, for scans that have a dense cloud (COLMAP's fused.ply) and no mesh.  The planes then go
 * through cgs_depth_window_max and gate every operator exactly as a mesh's do.  The reference has no counterpart.  intr, w2c
 * as for cgs_point_mask.  The rule is frozen -- float64, one rounded operation at a time in the written order, nothing
 * contracted into an FMA, IEEE division -- so that the numpy back end agrees on every bit.
 *
 * cgs_surfel_depth: points is float32 [P,3], device; normals is float32 [P,3], device, or NULL; radii is float32 [P], device
 * (world units); depth is float32 [V,height,width], device.  The entry fills depth with +inf and then, for every
 * (surfel, view):
 *   the point widened to float64, c = R X + T in the operation order of cgs_project_points
 *   the normal widened to float64, n = R N: per row (r0 * Nx + r1 * Ny) + r2 * Nz, no translation
 *   with normals == NULL, n = (0, 0, 1): the disk faces the camera plane (for clouds without normals)
 *   r = (double)radii[p]; the surfel is SKIPPED in the view unless r > 0 and c2 - r > 0 (a NaN fails the test, and so does
 *     r = +inf): there is no clipping, a disk that could reach the camera plane is dropped whole
 *   zlo = c2 - r, zhi = c2 + r;  a = c0 - r, b = c0 + r
 *   ulo = fx * min(a / zlo, a / zhi) + cx,  uhi = fx * max(b / zlo, b / zhi) + cx      (min, max: a NaN operand loses)
 *   vlo, vhi likewise from c1 - r, c1 + r and fy, cy: the image box of the bounding box of the disk's sphere
 *   the surfel is SKIPPED if ulo, uhi, vlo or vhi is NaN (that takes a NaN or infinite c0 / c1 or a NaN camera, with which
 *     no pixel below is covered: the skip changes no output)
 *   the CANDIDATES are jlo <= j <= jhi, ilo <= i <= ihi, formed as cgs_mesh_depth forms its own:
 *     jlo = min(max(ceil(ulo - 0.5), 0), width)        jhi = max(min(floor(uhi - 0.5), width - 1), -1)
 *     ilo = min(max(ceil(vlo - 0.5), 0), height)       ihi = max(min(floor(vhi - 0.5), height - 1), -1)
 *     all in float64, converted to int after the clamp.  The box is part of the rule, as the triangle's is of the mesh's
 *   num = (n0 * c0 + n1 * c1) + n2 * c2, once per (surfel, view)
 *   at the pixel centre (px, py) = (j + 0.5, i + 0.5):
 *     dx = (px - cx) / fx,  dy = (py - cy) / fy                  (the ray through the centre is (dx, dy, 1) * s)
 *     den = (n0 * dx + n1 * dy) + n2,  s = num / den             (where the ray meets the disk's plane: its camera z)
 *     qx = s * dx - c0,  qy = s * dy - c1,  qz = s - c2
 *     d2 = (qx * qx + qy * qy) + qz * qz;  the pixel is COVERED iff d2 <= r * r
 *     z = (float)s;  depth[v][i][j] = min(depth[v][i][j], z) if z is a positive finite float; otherwise nothing is stored
 * The minimum is cgs_mesh_depth's: the integer atomic minimum on the float's bit pattern, behind a plain read.
 *
 * CONSEQUENCES.  The disk is two-sided.  The normal need not have unit length: s does not change with its scale (to the
 * bit for a power of two; in the last bits otherwise, as num and den round on their own).  A zero normal (0 / 0), a grazing
 * ray (den == 0: s is infinite) and a NaN anywhere store nothing.  The result does not depend on the launch geometry or
 * on the order of the points.  Limits: no near-plane clipping; a disk overhangs a silhouette by up to its radius and pokes
 * through the other face at a concave corner, so a cloud hides slightly MORE than the surface it samples; isotropic disks
 * only; each (surfel, view) costs its candidate box.
 *
 * Runs on the caller's stream with no allocation and no host synchronisation.  Every argument is checked, whether or not
 * there is work: P or V < 0, a size outside [1, CGS_EDT_MAX_SIZE] and NULL pointers (points and radii only when P > 0;
 * normals may always be NULL) are CGS_ERR_INVALID_ARGUMENT, rejected before anything is launched.  Then V = 0 is a no-op;
 * P = 0 still fills the planes with +inf.
 * ------------------------------------------------------------------------------------------------ */
int cgs_surfel_depth(int P, const float* points /*[P,3]*/, const float* normals /*[P,3] or NULL*/,
                     const float* radii /*[P]*/, int V, const double* intr /*[V,4]*/, const double* w2c /*[V,12]*/,
                     int height, int width, float* depth /*[V,height,width]*/, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Depth maps from a scan's own photographs: plane-sweep stereo, for scans that have photographs and poses and neither a
 * mesh, a dense cloud nor depth maps.  One camera-z map per view, 0 where stereo gives nothing -- the format the caller's
 * depth maps have (ops.edge_occlusion.check_depth_maps turns <= 0 into +inf: the gate fails open).  The reference has no
 * counterpart.  The rule is frozen -- float64, one rounded operation at a time in the written order, nothing contracted
 * into an FMA, IEEE division, NO square root, every sum a running sum from 0.0 in the stated order -- so that the numpy
 * back end (ops/stereo_depth.py) agrees on every bit.  It is stated once for the kernels, in csrc/stereo_depth.h.
 *
 * Inputs, all device arrays.  gray: uint8 [V,height,width] luminance.  intr: [V,4] doubles fx, fy, cx, cy.  inv: [V,D]
 * doubles, the inverse depths of view v's hypotheses.  src: int32 [V,S], the source views of reference view v; an entry
 * outside [0, V) (-1 by convention) is no source.  rel: [V,S,12] doubles, row-major [R | T] taking reference-camera
 * coordinates to the source's camera coordinates.  inv, src and rel are made by the host, so both back ends read the same
 * bits.  Scalars: the patch radius R, min_var, max_cost, min_sources.  n = (2R+1)^2 as a double; thr = (min_var * n) * n.
 *
 * cgs_stereo_sweep, reference pixel (i, j) of view v; depth[v][i][j] is written exactly once, by a plain store:
 *   0 unless the whole patch lies inside the image: i - R >= 0, i + R <= height - 1, j - R >= 0, j + R <= width - 1
 *   taps k in row-major order (di = -R..R outer, dj = -R..R inner); r_k = (double)gray[v][i+di][j+dj]
 *   sr = sum r_k, srr = sum r_k * r_k, var_r = n * srr - sr * sr;  0 unless var_r > thr
 *   hypothesis d = 0..D-1: z = 1.0 / inv[v][d].  Source s = 0..S-1 in order, skipped when src[v][s] is no source; with
 *   w = src[v][s], M = rel[v][s] and (fx', fy', cx', cy') = intr[w], per tap:
 *     px = (j + dj) + 0.5, py = (i + di) + 0.5;  X = ((px - cx) / fx) * z,  Y = ((py - cy) / fy) * z    (intr[v])
 *     c = M (X, Y, z): per row ((m0 * X + m1 * Y) + m2 * z) + m3, the operation order of cgs_project_points
 *     the tap is INVALID if !(c2 > 0);  u = fx' * (c0 / c2) + cx',  v = fy' * (c1 / c2) + cy'
 *     x = u - 0.5, y = v - 0.5, x0 = floor(x), y0 = floor(y); INVALID unless 0 <= x0, x0 + 1 <= width - 1, 0 <= y0,
 *       y0 + 1 <= height - 1, compared in float64 (a NaN or an infinity is invalid)
 *     a = x - x0, b = y - y0;  g00 = gray[w][y0][x0], g01 = gray[w][y0][x0+1], g10 = gray[w][y0+1][x0], g11 likewise
 *     top = g00 * (1 - a) + g01 * a,  bot = g10 * (1 - a) + g11 * a,  val = top * (1 - b) + bot * b
 *     ss += val, sss += val * val, srs += r_k * val
 *   the source COUNTS for d iff every tap is valid and var_s = n * sss - ss * ss > thr; then
 *     cov = n * srs - sr * ss;  score = (cov * fabs(cov)) / (var_r * var_s);  cost_s = 1 - score
 *     (score is the signed square of the normalised cross-correlation, in [-1, 1] up to rounding)
 *   cost[d] = (sum of cost_s over the counting sources, in source order) / (double)count; +inf when count < min_sources
 *   WINNER: best = the d of the smallest cost, a strict < keeping the lowest d on a tie; cb = cost[best];
 *     0 unless cb is finite and cb <= max_cost
 *   REFINEMENT: o = 0 unless 0 < best < D - 1, cm = cost[best-1] and cp = cost[best+1] are finite and
 *     den = (cm - 2 * cb) + cp > 0; then o = (0.5 * (cm - cp)) / den, clamped to [-0.5, 0.5]
 *     q = inv[v][best] + o * (o >= 0 ? inv[v][best+1] - inv[v][best] : inv[v][best] - inv[v][best-1]), and q = inv[v][best]
 *     itself when o == 0 (an end has no neighbour to read);  depth[v][i][j] = (float)(1.0 / q)
 * CONSEQUENCES.  D = 1: the one hypothesis wins when its cost is finite and <= max_cost, unrefined.  D = 2: the cheaper of
 * the two (d = 0 on a tie), unrefined: both are ends.  R = 0: one tap has no variance (var_r = r * r - r * r = 0), so every
 * pixel stores 0; matching starts at R = 1.  den = (cm - cb) + (cp - cb) is > 0 for finite costs around a strict minimum;
 * the test guards the division, and at its edge (cp == cb) o is 0.5, the clamp's end.  A source whose pose or depth holds
 * a NaN never counts.  The cost volume is never stored.
 *
 * cgs_stereo_consistency, pixel (i, j) of view v with z = (double)depth[v][i][j]; out[v][i][j] is written exactly once:
 *   0 unless z > 0 (a NaN fails).  Otherwise X = (((j + 0.5) - cx) / fx) * z, Y = (((i + 0.5) - cy) / fy) * z and, per
 *   source as above, c = M (X, Y, z); the source AGREES iff c2 > 0, (u, v) formed as above lies in the image
 *   (0 <= u < width, 0 <= v < height: cgs_point_mask_depth's test), ds = (double)depth[w][floor(v)][floor(u)] > 0 and
 *   fabs(1.0 / ds - 1.0 / c2) <= tol[v], tol a double per view.  out[v][i][j] = depth[v][i][j], the same bits, when at
 *   least min_consistent sources agree, and 0 otherwise.  depth and out must not overlap: a pixel reads other views.
 *
 * Both run on the caller's stream with no allocation, no atomics and no host synchronisation; the result does not depend
 * on the launch geometry.  Every argument is checked whether or not there is work: V < 0, a size outside
 * [1, CGS_EDT_MAX_SIZE], D < 1, S < 1, a radius outside [0, CGS_STEREO_MAX_RADIUS], min_var negative or NaN, a NaN
 * max_cost, min_sources < 1, min_consistent < 0, NULL pointers and overlapping depth / out are
 * CGS_ERR_INVALID_ARGUMENT, rejected before anything is launched.  Then V = 0 is a no-op.
 * ------------------------------------------------------------------------------------------------ */
#define CGS_STEREO_MAX_RADIUS 8
int cgs_stereo_sweep(int V, int height, int width, const uint8_t* gray /*[V,height,width]*/, const double* intr /*[V,4]*/,
                     int D, const double* inv /*[V,D]*/, int S, const int* src /*[V,S]*/, const double* rel /*[V,S,12]*/,
                     int radius, double min_var, double max_cost, int min_sources,
                     float* depth /*[V,height,width]*/, void* stream);
int cgs_stereo_consistency(int V, int height, int width, const float* depth /*[V,height,width]*/,
                           const double* intr /*[V,4]*/, int S, const int* src /*[V,S]*/, const double* rel /*[V,S,12]*/,
                           const double* tol /*[V]*/, int min_consistent, float* out /*[V,height,width]*/, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fusing the stereo depth maps across views.  cgs_stereo_consistency uses the other views only to DELETE depths; a pixel
 * that its own view failed to match stays empty although every other view that saw the same surface holds its depth.
 * cgs_stereo_warp carries every source's map into the target view, cgs_stereo_fuse keeps, per pixel, the largest cluster
 * of agreeing inverse depths (the own depth included) and stores the cluster's mean.  The output is again one camera-z
 * map per view, 0 where there is none.  The reference has no counterpart.  The rule is frozen with the conventions of the
 * sweep above -- float64, one rounded operation at a time in the written order, nothing contracted, IEEE division, no
 * square root, running sums from 0.0 in the stated order -- and stated once for the kernels, in csrc/stereo_fuse.h.
 *
 * Inputs, all device arrays, made by the host so that both back ends read the same bits.  depth: float32
 * [V,height,width].  intr: [V,4] doubles.  fsrc: int32 [V,F], the fusion sources of TARGET view v; an entry outside [0, V)
 * is no source.  into: [V,F,12] doubles, row-major [R | T] taking the SOURCE's camera coordinates to the TARGET's (the
 * sweep's rel goes the other way).  tol: [V] doubles, the consistency tolerance in inverse depth.  Both entries take a
 * range of targets v0 <= v < v0 + nv with 0 <= v0 and v0 + nv <= V, so that the intermediate stays bounded; a DEPTH below
 * is a positive finite float (a NaN, an infinity, zero and negative values are none).
 *
 * cgs_stereo_warp, output warped float32 [nv,F,height,width].  The entry first fills warped with +inf.  Then for every
 * target v of the range, every slot s with a source w = fsrc[v][s], and every source pixel (i, j):
 *   skip unless depth[w][i][j] is a depth; z = (double)depth[w][i][j]
 *   X = (((j + 0.5) - cx_w) / fx_w) * z,  Y = (((i + 0.5) - cy_w) / fy_w) * z                            (intr[w])
 *   c = M (X, Y, z), M = into[v][s]: per row ((m0 * X + m1 * Y) + m2 * z) + m3, the operation order of cgs_project_points
 *   skip unless c2 > 0;  u = fx_v * (c0 / c2) + cx_v,  v' = fy_v * (c1 / c2) + cy_v                        (intr[v])
 *   skip unless 0 <= u < width and 0 <= v' < height (cgs_point_mask_depth's test; a NaN fails)
 *   zf = (float)c2; if zf is a depth: warped[v-v0][s][floor(v')][floor(u)] = min(what it holds, zf)
 *   (the integer atomic minimum on the float's bit pattern behind a plain read, as cgs_mesh_depth stores)
 * The result does not depend on the launch geometry or the order.  depth and warped must not overlap.
 *
 * cgs_stereo_fuse, outputs out float32 [nv,height,width] and support uint8 [nv,height,width] (may be NULL); each pixel is
 * written exactly once, by plain stores, no atomics.  Pixel (i, j) of target v:
 *   candidates k = 0..F: k = 0 is present iff depth[v][i][j] is a depth, k = s + 1 iff warped[v-v0][s][i][j] is one;
 *     q_k = 1.0 / (double)value
 *   support_k = the number of present m (k itself included) with fabs(q_m - q_k) <= tol[v]
 *   WINNER: there is no best at first; scanning k upward, a present k replaces the best iff there is none yet, or
 *     support_k > support_best, or support_k == support_best and q_k < q_best -- the FARTHER candidate wins a tie, the
 *     side on which a gate errs safely; the lowest k stays on a full tie
 *   0 (and support 0) when no candidate is present or support_best < min_support
 *   otherwise sum = the running sum of q_m over the present m = 0..F in order with fabs(q_m - q_best) <= tol[v], count
 *     their number; mean = sum / (double)count; out = (float)(1.0 / mean); support = (uint8_t)count
 * CONSEQUENCES.  The fused map holds NEW values: every cluster of two or more stores a mean, and even where only the own
 * depth supports itself the stored number is (float)(1 / (1 / z)), not a copy (its two float64 roundings lie far inside
 * half a float32 step, so it has z's bits again).  A NaN tol stores 0 everywhere (no candidate supports even itself), and so does a negative one; tol = 0 clusters
 * equal inverse depths only; tol = +inf makes every present candidate a member.  min_support > F + 1 stores 0
 * everywhere.  Two source pixels landing on one target pixel keep the nearer.  A point that is visible in the source and
 * hidden in the target lands BEHIND the target's surface: it loses to the cluster, or alone it yields a far depth; both
 * fail open.  support never saturates: F + 1 <= 17.
 *
 * Both run on the caller's stream with no allocation and no host synchronisation.  Every argument is checked whether or
 * not there is work: V < 0, a size outside [1, CGS_EDT_MAX_SIZE], a range outside [0, V], F outside
 * [1, CGS_STEREO_MAX_FUSE], min_support < 1, NULL pointers (support excepted) and overlapping buffers (warped with depth;
 * out or support with depth, warped or each other) are CGS_ERR_INVALID_ARGUMENT, rejected before anything is launched.
 * Then nv = 0 is a no-op.
 * ------------------------------------------------------------------------------------------------ */
#define CGS_STEREO_MAX_FUSE 16
int cgs_stereo_warp(int V, int height, int width, const float* depth /*[V,height,width]*/, const double* intr /*[V,4]*/,
                    int F, const int* fsrc /*[V,F]*/, const double* into /*[V,F,12]*/, int v0, int nv,
                    float* warped /*[nv,F,height,width]*/, void* stream);
int cgs_stereo_fuse(int V, int height, int width, const float* depth /*[V,height,width]*/, int F,
                    const float* warped /*[nv,F,height,width]*/, const double* tol /*[V]*/, int min_support, int v0, int nv,
                    float* out /*[nv,height,width]*/, uint8_t* support /*[nv,height,width] or NULL*/, void* stream);

/* ------------------------------------------------------------------------------------------------
 * A truncated signed distance field (TSDF) from per-view depth maps, and its surface as a triangle soup by marching
 * tetrahedra.  The maps of a scan -- the stereo maps above, a z-buffer's planes, a sensor's -- are separate estimates of
 * one surface; the field AVERAGES the signed distances that the views report at a point of space (it takes no minimum, so
 * noise on either side of the surface cancels), and its zero set is one surface that all views share, in the float32
 * [T,3,3] layout that cgs_mesh_depth and cgs_mesh_contours take.  The reference has no counterpart.  The rule is frozen
 * with the conventions of this header -- float64, one rounded operation at a time in the written order, nothing
 * contracted, IEEE division, running sums in view order, 64-bit offsets -- and stated once for the kernels, in csrc/tsdf.h.
 *
 * LATTICE.  The lattice points are the voxel centres of the grid of cgs_voxel_votes (nx, ny, nz, lo, step; the same
 * checks): point g = i + nx (j + ny k) is float64 lo + (i + 0.5) * step per axis, rounded to float32 and widened again.  A
 * CELL is the cube between 8 neighbouring points: cell (i, j, k) with 0 <= i < nx - 1, 0 <= j < ny - 1, 0 <= k < nz - 1 has
 * the linear index i + (nx - 1) (j + (ny - 1) k), and its corner c = dx + 2 dy + 4 dz is the point (i + dx, j + dy, k + dz).
 * A grid with a dimension of 1 has no cells.
 *
 * cgs_tsdf_integrate.  State: sum float64 [nx ny nz], weight uint16 [nx ny nz].  Without `accumulate` a point starts
 * from (0.0, 0); with it, from its own stored pair.  Then the views v = 0 .. V-1 in order (cameras and planes as
 * cgs_voxel_votes_depth takes them: intr [V,4], w2c [V,3,4], depth float32 [V,height,width], one size per call):
 *   the point is projected as cgs_point_mask_depth projects (c2 > 0, 0 <= u < width, 0 <= v' < height); a view that does
 *     not keep it contributes nothing
 *   d = (double)depth[v][floor(v')][floor(u)], the pixel the occlusion rule reads
 *   the view OBSERVES the point iff d > 0 && d < +inf: a NaN, 0, a negative depth and +inf all fail (0 is the stereo
 *     maps' "unsure", +inf the z-buffers' "no surface"; neither carves)
 *   sdf = d - c2; if sdf < -trunc the view does not observe the point (it lies too far behind the surface to know of)
 *   if weight == 65535 the view contributes nothing: the weight SATURATES, and the pair stays a sum over `weight` views
 *   t = sdf / trunc; if t > 1.0, t = 1.0; sum += t; weight += 1
 * Because a thread continues its own running sum, integrating V views at once and integrating them in chunks with
 * `accumulate` give the same bits, as cgs_sample_snap_terms guarantees for its sums.  V = 0 without `accumulate` writes
 * (0.0, 0) everywhere; with it, nothing.
 *
 * EXTRACTION, two entries with the caller's exclusive scan between them.  A cell is LIVE iff all 8 corners have
 * weight >= min_weight (1 <= min_weight <= 65535).  A corner's value is f = sum / (double)weight; the corner is INSIDE iff
 * f < 0 (0.0, -0.0 and a NaN are outside).  The cube is cut into the 6 Kuhn tetrahedra around the diagonal from corner 0 to
 * corner 7, the same cut in every cell, so neighbouring cells agree on their shared faces: tetrahedron t = 0..5 belongs to
 * the t-th order (a, b, c) of the axes 0, 1, 2 in lexicographic order and has the corners (q0, q1, q2, q3) =
 * (0, 1 << a, (1 << a) | (1 << b), 7), in ascending corner number; its PARITY is the order's (t = 0, 3, 4 even; 1, 2, 5
 * odd).  E(x, y) is the vertex on the lattice edge from q_x to q_y.  Per tetrahedron, by its inside corners:
 *   none or all four: no triangle
 *   one, x, the others p < q < r:   (E(x,p), E(x,q), E(x,r)), TURNED iff x is odd
 *   three, all but x, p < q < r:    the same triangle, turned iff x is even
 *   two, i < j, outside k < l:      the quad E(i,k) E(i,l) E(j,l) E(j,k), split along the diagonal E(i,k) -- E(j,l):
 *                                   (E(i,k), E(i,l), E(j,l)) then (E(i,k), E(j,l), E(j,k)), both turned iff (i, j, k, l) is an
 *                                   odd permutation of (0, 1, 2, 3)
 * Turning swaps a triangle's second and third vertex; a tetrahedron of odd parity turns every triangle once more.
 * WINDING: with that, (v1 - v0) x (v2 - v0) points from inside to outside (in tetrahedron 0 with corner 0 alone inside,
 * the triangle on the three axes has the normal (1, 1, 1); every other case is this one with the corners relabelled, and
 * an odd relabelling mirrors the tetrahedron).  At most 2 triangles per tetrahedron, 12 per cell.
 * A VERTEX lies on a lattice edge whose ends differ in sign.  With the ends in ascending linear lattice index (a, b),
 * whichever of them is inside: p = Pa + (fa / (fa - fb)) * (Pb - Pa) per component in float64, rounded to float32.  The end
 * order is canonical, so two cells that share an edge produce the same bits and a weld by bits sees no crack.  An outside
 * end of exactly 0.0 puts the vertex ON the lattice point; triangles with two equal vertices are emitted like any other
 * (the Python layer drops them).
 *   cgs_tsdf_mesh_count: counts uint8 [(nx-1)(ny-1)(nz-1)], the triangles of every cell (0 for a cell that is not live).
 *   cgs_tsdf_mesh_emit:  offsets int64 [cells], the exclusive prefix sums of counts; tris float32 [T,3,3].  Cell e writes
 *     its triangles at tris[offsets[e]] .. in the order tetrahedron, then triangle, so the soup is ordered by cell and does
 *     not depend on the launch geometry.  A cell whose range does not lie in [0, T] writes nothing (the caller's error).
 *
 * All three run on the caller's stream with no allocation, no atomics and no host synchronisation.  Every argument is
 * checked whether or not there is work: the grid and the views as cgs_voxel_votes_depth checks them, a trunc that is not
 * finite and > 0, a min_weight outside [1, CGS_TSDF_MAX_WEIGHT], T < 0 and NULL pointers are CGS_ERR_INVALID_ARGUMENT,
 * rejected before anything is launched, so every buffer is untouched.  intr, w2c and depth may be NULL when V = 0; counts,
 * offsets and tris when the grid has no cells; offsets and tris when T = 0.
 * ------------------------------------------------------------------------------------------------ */
#define CGS_TSDF_MAX_WEIGHT 65535
int cgs_tsdf_integrate(int nx, int ny, int nz, const double* lo /*host, [3]*/, const double* step /*host, [3]*/, int V,
                       const double* intr /*[V,4]*/, const double* w2c /*[V,3,4]*/, int height, int width,
                       const float* depth /*[V,height,width]*/, double trunc, int accumulate, double* sum /*[nx ny nz]*/,
                       uint16_t* weight /*[nx ny nz]*/, void* stream);
int cgs_tsdf_mesh_count(int nx, int ny, int nz, const double* sum /*[nx ny nz]*/, const uint16_t* weight /*[nx ny nz]*/,
                        int min_weight, uint8_t* counts /*[cells]*/, void* stream);
int cgs_tsdf_mesh_emit(int nx, int ny, int nz, const double* lo /*host, [3]*/, const double* step /*host, [3]*/,
                       const double* sum /*[nx ny nz]*/, const uint16_t* weight /*[nx ny nz]*/, int min_weight,
                       const int64_t* offsets /*[cells]*/, int64_t T, float* tris /*[T,3,3]*/, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CURVEGS_H_INCLUDED */
