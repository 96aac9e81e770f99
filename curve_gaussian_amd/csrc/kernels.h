// Host-side launchers, one per kernel, defined next to the kernels (each .hip file is its own translation unit;
// no relocatable device code is needed).  api.hip sequences them on the caller's stream.
#pragma once
#include "common.h"

namespace cgs {

// The depth gate of the _depth entries (include/curvegs.h): one float32 [height, width] plane per view and the slack of
// nv_hidden (point_projection.h).  A launcher with a gated form takes `const DepthGate* gate`: nullptr is the entry as it
// always was (the GATED = false instantiation, no plane read, no hidden output written), a gate is its _depth sibling, with
// the hidden output beside it.  The near plane of the _clipped entries is a nullable `const double* near` in the same way.
struct DepthGate {
    const float* depth;
    double slack;
};

// The gate of the training render (cgs_view_forward_depth / cgs_view_forward_render_depth; view.hip, k_view_fwd<true>): it
// needs more than a DepthGate holds, because the kernel projects a splat's centre itself -- the resident stack of planes,
// float32 [V,H,W] with H x W the image of the forward, the float64 cameras the planes were drawn with, and which view this
// forward is: `view` on the host, or *view_index on the device when that pointer is set.  launch_view_forward takes
// `const ViewGate* gate` by the convention above: nullptr is the forward as it always was.  Passed to the kernel by value.
struct ViewGate {
    const float* planes;
    const double* intr;
    const double* w2c;
    const int* view_index;
    double slack;
    int V, view;
};

// preprocess.hip
void launch_preprocess_fwd(hipStream_t s, int P, int D, int M, const float* means3D, const float* scales,
                           float scale_modifier, const float* rotations, const float* opacities, const float* shs,
                           uint8_t* clamped, const float* cov3D_precomp, const float* colors_precomp,
                           const float* all_map, const float* viewmatrix, const float* projmatrix,
                           const float* cam_pos, int W, int H, float tan_fovx, float tan_fovy, float focal_x,
                           float focal_y, int* radii, SplatRec* rec, float* rgb, int grid_x, int grid_y,
                           uint32_t* tile_count, int antialiasing, int cull, float* grad_acc, uint32_t* clear_words,
                           size_t n_clear);
void launch_mark_visible(hipStream_t s, int P, const float* means3D, const float* viewmatrix, uint8_t* present);
void launch_preprocess_bwd(hipStream_t s, int P, int D, int M, const float* means3D, const int* radii,
                           const float* shs, const uint8_t* clamped, const float* opacities, const float* scales,
                           const float* rotations, float scale_modifier, const float* cov3D_precomp,
                           const float* viewmatrix, const float* projmatrix, const float* cam_pos, float focal_x,
                           float focal_y, float tan_fovx, float tan_fovy, int W, int H, const SplatRec* rec,
                           float* grad_acc, float* dL_dmean2D, float* dL_dconic, float* dL_dinvdepth,
                           float* dL_dopacity, float* dL_dmean3D, float* dL_dcolor, float* dL_dall_map,
                           float* dL_dcov3D, float* dL_dsh, float* dL_dscale, float* dL_drot, int antialiasing);

// binning.hip
void launch_scan_tiles(hipStream_t s, int tiles, const uint32_t* tile_count, uint2* ranges, uint32_t* total);
// `cap` = number of instances the binning buffer can hold: tiles whose range does not fit are skipped (speculative launch)
void launch_scatter(hipStream_t s, int P, const int* radii, const SplatRec* rec, int grid_x, int grid_y,
                    const uint2* ranges, uint32_t* tile_cursor, uint64_t* keys, uint32_t cap, int cull,
                    uint32_t* nonunit = nullptr);   // nonunit: word raised when a visible splat's colour / all_map[3] is not 1
// big_count: status word counting the splats whose rect exceeds the wave walk's comfort zone; big_queue (nullable,
// big_cap entries): where they are deferred to for a one-workgroup-per-splat second kernel
void launch_scatter_bucket(hipStream_t s, int P, const int* radii, const SplatRec* rec, int grid_x, int grid_y,
                           uint32_t* tile_count, uint64_t* keys, uint32_t cap, int cull, uint32_t* big_count,
                           uint32_t* big_queue, uint32_t big_cap, uint32_t* nonunit = nullptr,
                           int splats_per_wave = 12);   // 12 (one curve per wave) or 8 (sparse views: more, shorter waves)
void launch_tile_sort_bucket(hipStream_t s, int tiles, const uint32_t* tile_count, uint2* ranges, uint32_t* total,
                             uint64_t* keys, uint32_t* point_list, uint32_t cap);
uint32_t bucket_cap_limit();
void launch_tile_sort_small(hipStream_t s, int tiles, const uint2* ranges, uint64_t* keys, uint32_t* point_list,
                            uint32_t cap);
void launch_tile_sort_big(hipStream_t s, int tiles, const uint2* ranges, uint64_t* keys, uint32_t* point_list,
                          uint32_t max_count);

// render.hip
void launch_render_fwd(hipStream_t s, bool geo, int tiles, const uint2* ranges, const uint32_t* point_list, int W,
                       int H, int grid_x, const SplatRec* rec, float* final_T, uint32_t* n_contrib,
                       const float* bg_color, float* out_color, float* out_invdepth, float* out_all_map,
                       bool unit = false,    // unit: colour == 1 and all_map[3] == 1 for every splat (render.hip, UNIT)
                       bool tag = false);    // tag: staged list entries get the quadrant masks in their top bits (TAG)
bool render_fwd_can_sort(uint32_t cap);
void launch_render_fwd_sorting(hipStream_t s, bool geo, int tiles, const uint32_t* tile_count, const uint64_t* keys,
                               uint32_t cap, uint2* ranges, uint32_t* total, uint32_t* point_list, int W, int H,
                               int grid_x, const SplatRec* rec, float* final_T, uint32_t* n_contrib,
                               const float* bg_color, float* out_color, float* out_invdepth, float* out_all_map,
                               bool unit = false, bool tag = false,
                               // render()'s epilogue written by the same kernel (NULL: not wanted): the image clamped to
                               // [0, 1], the direction map in world space (wv = world_view_transform, device memory)
                               float* color_clamped = nullptr, float* dir_out = nullptr, const float* wv = nullptr);
void launch_render_bwd(hipStream_t s, bool geo, bool invd, bool colg, int tiles, const uint2* ranges,
                       const uint32_t* point_list, int W, int H, int grid_x, const float* bg_color,
                       const SplatRec* rec, const float* final_Ts, const uint32_t* n_contrib, const float* dL_dpixels,
                       const float* dL_dout_invdepth, const float* dL_dout_all_map, float* grad_acc,
                       int acc_stride = ACC_STRIDE,    // floats per accumulator record (ACC_STRIDE_VIEW on the view path)
                       uint32_t id_mask = 0xffffffffu,           // strips the forward's list tags (LIST_ID_MASK when it tagged)
                       const uint32_t* nonunit_gate = nullptr);  // device word: the kernel returns at once when it is zero


// render_unit_bwd.hip: the unit-colour training instance (colour == 1, only dL/dcolour flowing in), lane = (splat, quadrant)
// acc_stride: ACC_STRIDE_VIEW (view path) or ACC_STRIDE (operator API); nonunit_gate: device word, the kernel returns at
// once when it is NOT zero (the general training instance launched beside it takes over)
void launch_render_bwd_unit(hipStream_t s, int tiles, const uint2* ranges, const uint32_t* point_list, int W, int H,
                            int grid_x, const float* bg_color, const SplatRec* rec, const float* final_Ts,
                            const uint32_t* n_contrib, const float* dL_dpixels, float* grad_acc,
                            int acc_stride = ACC_STRIDE_VIEW, const uint32_t* nonunit_gate = nullptr,
                            // torch.clamp's gradient mask folded in: dL/dpixel counts only where 0 <= clamp_raw <= 1 (NULL: all)
                            const float* clamp_raw = nullptr);

// sampling.hip
int sample_norm_words();
void launch_sample_norms(hipStream_t s, int B, int m, const float* cp, const uint8_t* is_bezier, const void* coef, double* norms);
void launch_sample_backward_close(hipStream_t s, int B, int m, const float* cp, const float* width, const uint8_t* is_bezier,
                                  const void* coef, float eps, const double* norms, const float* part, float* g_cp, float* g_width,
                                  int accumulate);
// view.hip
void launch_view_forward(hipStream_t s, int B, int m, const float* cp, const float* width, const uint8_t* is_bezier,
                         const void* coef, float eps, const double* norms, const float* opacity_logit,
                         const float* mask_logit, float mask_thr, const float* colors_precomp, const float* campos,
                         const float* viewmatrix, const float* projmatrix, float tan_fovx, float tan_fovy, float focal_x,
                         float focal_y, int W, int H, int grid_x, int grid_y, float* xyz, float* rot, float* scl, int* radii,
                         SplatRec* rec, float* grad_acc, uint32_t* clear_words, size_t n_clear, const ViewGate* gate = nullptr);
void launch_view_backward(hipStream_t s, int B, int m, const float* cp, const float* width, const uint8_t* is_bezier,
                          const void* coef, float eps, double* norms, const float* opacity_logit, const float* mask_logit,
                          float mask_thr, const float* campos, const float* viewmatrix, const float* projmatrix,
                          float tan_fovx, float tan_fovy, float focal_x, float focal_y, int W, int H, const int* radii,
                          const SplatRec* rec, float* grad_acc, const float* g_rot_raw_extra, float* dL_dmean2D,
                          float* g_opacity_logit, float* g_mask_logit, float* curve_part, int accumulate);
int sample_norm_fwd_words();
void launch_sample_forward(hipStream_t s, int B, int m, const float* cp, const float* width, const uint8_t* is_bezier,
                           const void* coef, float eps, double* norms, float* xyz, float* rot, float* scaling);
void launch_sample_backward(hipStream_t s, int B, int m, const float* cp, const float* width, const uint8_t* is_bezier,
                            const void* coef, float eps, double* norms, const float* g_xyz, const float* g_rot,
                            const float* g_scaling, float* g_cp, float* g_width, float* gv_cache);
void launch_attrs_forward(hipStream_t s, int B, int m, const float* rot_raw, const float* xyz, const float* opacity_logit,
                          const float* mask_logit, float mask_thr, const float* scaling, const float* campos,
                          const float* vm, float* rot_n, float* opac, float* scl_out, float* all_map);
void launch_attrs_backward(hipStream_t s, int B, int m, const float* rot_raw, const float* xyz,
                           const float* opacity_logit, const float* mask_logit, float mask_thr, const float* scaling,
                           const float* campos, const float* vm, const float* g_rot_n, const float* g_opac,
                           const float* g_scl_out, const float* g_all_map, float* g_rot_raw, float* g_opacity_logit,
                           float* g_mask_logit, float* g_scaling);


// ssim.hip
void launch_ssim_fwd(hipStream_t s, int planes, int H, int W, float C1, float C2, const float* img1, const float* img2,
                     float* ssim_map, float* dm_dmu1, float* dm_dsigma1_sq, float* dm_dsigma12);
void launch_ssim_bwd(hipStream_t s, int planes, int H, int W, const float* img1, const float* img2,
                     const float* dL_dmap, const float* dm_dmu1, const float* dm_dsigma1_sq, const float* dm_dsigma12,
                     float* dL_dimg1);
// loss.hip  (scratch16: 16 zeroed bytes = {u32 n_pos, pad, f64 loss_sum})
size_t photometric_workspace_bytes(int H, int W);
void launch_photometric_loss(hipStream_t s, int H, int W, const float* image, const float* gt, const int* view_index,
                             float thr, const unsigned int* n_pos, float lambda_a, float lambda_b, int clamp,
                             void* workspace, float* grad, float* loss);
void launch_edge_count(hipStream_t s, int C, int HW, const float* gt, float thr, unsigned int* n_pos);
void launch_edge_aware_loss(hipStream_t s, int C, int H, int W, const float* image, const float* gt, float thr,
                            void* scratch16, float* grad);
size_t curve_reg_workspace_bytes();
size_t endpoint_connection_workspace_bytes(int B);
void launch_endpoint_connection(hipStream_t s, int B, const float* cp, float thr, float weight, void* workspace, float* loss,
                                float* dL_dcp, int accumulate);
void launch_curve_regularizers(hipStream_t s, int B, int m, const float* rot_raw, const float* opacity_logit,
                               const float* width, const int* radii, float w_op, const float* op_gate, float w_smo,
                               float w_width, float width_thr, void* workspace, float* loss, float* g_rot_raw,
                               float* g_opacity_logit, float* g_width);
int adam_max_segments();
size_t adam_state_bytes();
void launch_adam_flat_dev(hipStream_t s, long long n, float* p, float* g, float* m, float* v, const void* dev_state,
                          int nseg, float b1, float b2, float eps, int zero_grad, const unsigned int* skip_flag,
                          unsigned int* report_seq = nullptr, unsigned int* report_ring = nullptr, int report_len = 0);
void launch_adam_flat(hipStream_t s, long long n, float* p, float* g, float* m, float* v, const void* host_segs, int nseg,
                      float b1, float b2, float eps, float bc1, float sqrt_bc2, int zero_grad);
// knn.hip
size_t knn_workspace_bytes(int P);
void launch_knn(hipStream_t s, int P, const float* pts, float* dists, void* workspace);

// nn.hip
size_t nn1_workspace_bytes(int n_query);
void launch_nn1(hipStream_t s, int n_query, const float* query, int n_ref, const float* ref, float* dist, int* index,
                void* workspace);

// visibility.hip
void launch_edge_visibility(hipStream_t s, int n_curves, const double* curves, int n_lines, const double* lines,
                            int n_frames, const double* K, const double* w2c, int height, int width,
                            const unsigned char* maps, int invert, const DepthGate* gate, int* counts);

// metrics.hip
size_t view_metrics_workspace_bytes(int n_views);
hipError_t launch_view_metrics(hipStream_t s, int n_views, const cgs_metric_view* views_host, void* workspace,
                               double* sums, double* means);

// report.hip
size_t report_panels_workspace_bytes(int n_views);
void launch_report_panels(hipStream_t s, int n_views, const cgs_report_view* views_host, void* workspace,
                          unsigned char* out);

// novel_view.hip
void launch_project_points(hipStream_t s, int P, const float* points, int V, const double* intr, const double* w2c,
                           int height, int width, const DepthGate* gate, double* uv, uint8_t* hidden_out);
size_t render_points_workspace_bytes(int P, int V, int H, int W);
int render_points_views_per_chunk(int P, int V, int H, int W, size_t ws_bytes);
int render_points_keep(double alpha);
void launch_render_points(hipStream_t s, int P, const float* points, const float* colors, int V, const double* intr,
                          const double* w2c, int height, int width, const DepthGate* gate, double alpha, const double* bg,
                          float* out, int* kept, int* hidden, void* ws, int views_per_chunk);

// mesh.hip
void launch_ellipsoid_vertices(hipStream_t s, int first, int count, const float* xyz, const float* rot, const float* scale,
                               const float* rgb, int V0, const double* template_vertices, void* out);
void launch_ellipsoid_faces(hipStream_t s, int first, int count, int V0, int F0, const int* template_faces, void* out);

// densify.hip
void launch_densification_stats(hipStream_t s, long long P, const int* radii, const float* grad, long long stride,
                                float* max_radii, float* accum, float* denom, const unsigned int* skip_flag);

// curve_fit.hip
void launch_curve_straightness(hipStream_t s, int B, const float* cp, const uint8_t* is_bezier, int sample_num,
                               double thr, double thr_max, double* mean_dist, double* max_dist, uint8_t* straight);
size_t segment_merge_workspace_bytes(int n);
void launch_segment_merge_labels(hipStream_t s, int n, const float* seg, double dist_thr, double sim_thr, void* workspace,
                                 int* labels, int* n_components);
void launch_pair_consensus_fit(hipStream_t s, int K, const float* cp, const int* pairs, int sample_num, double ransac_thr,
                               double err_thr, float* ctrl, double* rmse, int* inliers, uint8_t* ok);


// undistort.hip
void launch_undistort_images(hipStream_t s, int n_views, const cgs_undistort_view* views_host, float fill,
                             int* blank_counts);

// edge_detect.hip
void launch_edge_gradients(hipStream_t s, int n_views, const cgs_edge_gradient_view* views_host, const float* taps,
                           int radius);
int launch_edge_trace(hipStream_t s, int n_views, const cgs_edge_trace_view* views_host, float low, float high, int thin,
                      int* changed_flag, hipError_t* err);

// edge_score.hip
hipError_t launch_point_mask(hipStream_t s, int P, const float* points, int V, const double* intr, const double* w2c,
                             int height, int width, uint8_t* mask, int* kept);
size_t edt_workspace_bytes(int V, int height, int width);
void launch_edt_squared(hipStream_t s, int V, int height, int width, const uint8_t* mask, void* workspace, int* dist2);
size_t edge_score_workspace_bytes(int V);
hipError_t launch_edge_score_reduce(hipStream_t s, int V, int height, int width, const uint8_t* pred_mask,
                                    const uint8_t* det_mask, const int* pred_dist2, const int* det_dist2, int n_tol,
                                    const int* tol2, void* workspace, int64_t* counts, double* sums,
                                    uint8_t* both_nonempty);
// edge_seed.hip
void launch_pack_near_bits(hipStream_t s, int V, int height, int width, const int* dist2, int tol2, unsigned int* bits);
struct SeedGrid {   // the voxel grid of a vote; passed by value
    double lo[3];
    double step[3];
    int nx, ny, nz;
};
struct SeedViews {  // the views of one call: cameras and packed near masks, stride = ceil(width / 32) words; passed by value
    int V, height, width, stride;
    const double* intr;
    const double* w2c;
    const unsigned int* bits;
};
using SeedGate = DepthGate;   // the name the seed kernels know it by; passed to them by value
void launch_voxel_votes(hipStream_t s, SeedGrid g, SeedViews views, const DepthGate* gate, int accumulate,
                        unsigned short* seen, unsigned short* hit, unsigned short* hidden);
void launch_voxel_moments(hipStream_t s, int nx, int ny, int nz, const unsigned int* keep, int N, const int* centres,
                          int radius, int* moments);
hipError_t launch_ray_claims(hipStream_t s, SeedGrid g, SeedViews views, const DepthGate* gate, int M, const int* index,
                             const unsigned short* support, int clear, unsigned int* best);
void launch_ray_wins(hipStream_t s, SeedGrid g, SeedViews views, const DepthGate* gate, int M, const int* index,
                     const unsigned short* support, const unsigned int* best, int window, int margin, int accumulate,
                     unsigned short* wins);

// edge_support.hip
void launch_edge_support(hipStream_t s, int E, int P, const float* points, const int* offsets, int V, const double* intr,
                         const double* w2c, int height, int width, const int* d2, int T, const int* tol2,
                         const DepthGate* gate, int* counts, int* hidden);

// edge_trim.hip
void launch_sample_support(hipStream_t s, int P, const float* points, int V, const double* intr, const double* w2c,
                           int height, int width, const int* d2, int T, const int* tol2, const DepthGate* gate, int* tally,
                           int* hidden);

// edge_dedupe.hip
size_t sample_cover_workspace_bytes(int P);
void launch_sample_cover(hipStream_t s, int P, const float* points, int E, const int* offsets, const int* rank, float tol2,
                         float cos2, int* cover, void* workspace);

// edge_join.hip
size_t end_attach_workspace_bytes(int P, int E);
void launch_end_attach(hipStream_t s, int P, const float* points, int E, const int* offsets, float tol2, float reach2,
                       unsigned long long* keys, void* workspace);

// edge_thin.hip
int launch_thin_masks(hipStream_t s, int V, int height, int width, uint8_t* masks, uint8_t* scratch, int* changed_flag,
                      int max_iterations, int* iterations, hipError_t* err);

// edge_orient.hip
void launch_mask_orientation(hipStream_t s, int V, int height, int width, const uint8_t* mask, uint8_t* code);
void launch_oriented_near(hipStream_t s, int V, int height, int width, const uint8_t* code, int tol2, uint8_t* near);
void launch_sample_support_oriented(hipStream_t s, int P, const float* points, const int* partner, int V, const double* intr,
                                    const double* w2c, int height, int width, const uint8_t* near, int spread,
                                    const DepthGate* gate, int* tally, int* hidden);

// edge_snap.hip
void launch_sample_snap_terms(hipStream_t s, int P, const float* points, int V, const double* intr, const double* w2c,
                              int height, int width, const int* d2, int cap2, const double* dist_lut, const DepthGate* gate,
                              double* terms, int* views, int* hidden);

// edge_occlusion.hip
hipError_t launch_mesh_depth(hipStream_t s, int F, const float* tris, int V, const double* intr, const double* w2c,
                             int height, int width, const double* near, float* depth);   // the cut is mesh_depth.h's
void launch_depth_window_max(hipStream_t s, int V, int height, int width, int radius, const float* depth, float* out);
hipError_t launch_point_mask_depth(hipStream_t s, int P, const float* points, int V, const double* intr, const double* w2c,
                                   int height, int width, const float* depth, double slack, uint8_t* mask, int* kept,
                                   int* hidden);

// mesh_contours.hip (a NULL gate is no depth plane; the cut is mesh_depth.h's)
hipError_t launch_mesh_contours(hipStream_t s, int E, const float* rows, int V, const double* intr, const double* w2c,
                                int height, int width, const DepthGate* gate, const double* near, uint8_t* mask);

// surfel_depth.hip (the rule is surfel_depth.h's)
hipError_t launch_surfel_depth(hipStream_t s, int P, const float* points, const float* normals, const float* radii, int V,
                               const double* intr, const double* w2c, int height, int width, float* depth);

// stereo_depth.hip (the rule is stereo_depth.h's)
void launch_stereo_sweep(hipStream_t s, int V, int height, int width, const uint8_t* gray, const double* intr, int D,
                         const double* inv, int S, const int* src, const double* rel, int radius, double min_var,
                         double max_cost, int min_sources, float* depth);
void launch_stereo_consistency(hipStream_t s, int V, int height, int width, const float* depth, const double* intr, int S,
                               const int* src, const double* rel, const double* tol, int min_consistent, float* out);

// stereo_fuse.hip (the rule is stereo_fuse.h's)
hipError_t launch_stereo_warp(hipStream_t s, int V, int height, int width, const float* depth, const double* intr, int F,
                              const int* fsrc, const double* into, int v0, int nv, float* warped);
void launch_stereo_fuse(hipStream_t s, int height, int width, const float* depth, int F, const float* warped,
                        const double* tol, int min_support, int v0, int nv, float* out, uint8_t* support);

// tsdf.hip (the rule is tsdf.h's; the lattice is a SeedGrid's voxel centres)
struct TsdfViews {  // the views of one call: cameras and float32 [V,height,width] depth planes; passed by value
    int V, height, width;
    const double* intr;
    const double* w2c;
    const float* depth;
};
void launch_tsdf_integrate(hipStream_t s, SeedGrid g, TsdfViews views, double trunc, int accumulate, double* sum,
                           unsigned short* weight);
void launch_tsdf_count(hipStream_t s, SeedGrid g, const double* sum, const unsigned short* weight, int min_weight,
                       uint8_t* counts);
void launch_tsdf_emit(hipStream_t s, SeedGrid g, const double* sum, const unsigned short* weight, int min_weight,
                      const long long* offsets, long long T, float* tris);

}  // namespace cgs
