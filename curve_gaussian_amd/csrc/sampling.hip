// Curve -> Gaussian sampling and per-view splat attributes, forward + hand-written backward.
//
// Replaces ~40 tiny PyTorch kernels per step (plus their autograd graph) of the reference:
//   GaussianCurveModel.prepare_scaling_rot   scene/gaussian_curve_model.py:180-198
//     get_curve_gaussians :70-78, get_curve_tangent :80-89, rot_to_quat_batch utils/general_utils.py:33-86
//   get_rotation (F.normalize) :121-122, get_opacity :108-110, get_main_axis :99-105,
//   straight-through mask + all_map build  gaussian_renderer/__init__.py:72-76,98-104
//
// One thread per SPLAT (sample i of curve b, splat index = b*m + i).  The reference divides v1 and v2 by the GLOBAL
// Frobenius norm of the whole [P,3] tensor: the norms couple every sample to every other one, so each
// direction is one pass for its grid-wide sums and one for its outputs (the sums and their slots: curve_math.h).
//   forward   k_sample_f12         S1, S2, BS  ->  N1, N2              k_sample_f3          xyz, rotation, scaling
//   backward  k_sample_bwd_sums    D2, A       ->  D1 in closed form   k_sample_bwd_curves  dL/d{control points, width}
// The fused view route (view.hip) has both backward sums from k_view_bwd and finishes with k_sample_bwd_close.
// The forward's sums are written one slot per workgroup; the backward's are block-reduced and accumulated with one f64
// atomic per block (order effects ~1e-16).
#include <algorithm>

#include "curve_math.h"

namespace cgs {

// ------------------------------------------------------------------------------------------------ forward
constexpr int F12_BLOCK = 1024;   // upper bound; the launch picks the workgroup size by splat count (f12_threads)
__global__ void __launch_bounds__(F12_BLOCK) k_sample_f12(int B, int m, const float* __restrict__ cp,
                                                         const uint8_t* __restrict__ is_bezier,
                                                         const SampleCoef* __restrict__ coef, double* __restrict__ norms) {
    // launched on exactly NORM_SLOTS workgroups: workgroup k owns slot k of the three forward sums (plain stores) and
    // clears slot k of the backward's two
    __shared__ SampleCoef s_coef[MAX_M];
    __shared__ double s_part[3][F12_BLOCK / 64];
    const float* src = reinterpret_cast<const float*>(coef);
    float* dst = reinterpret_cast<float*>(s_coef);
    for (int t = threadIdx.x; t < m * 16; t += blockDim.x) dst[t] = src[t];
    __syncthreads();
    double a1 = 0, a2 = 0, a3 = 0;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < B * m; p += gridDim.x * blockDim.x) {
        const int b = p / m, i = p - b * m;
        const CurveCP c = load_curve(cp, is_bezier, b);
        const V3 t = curve_tangent(c, s_coef[i]);
        const V3 c1 = {t.y, -t.x, 0.f};                 // cross(tan, (0,0,1))
        const V3 x = cross(t, c1);                      // N1 * c2v
        a1 += (double)(t.y * t.y + t.x * t.x);
        a2 += (double)(x.x * x.x + x.y * x.y + x.z * x.z);
        a3 += (double)dot(cross(x, t), c1);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        a1 += __shfl_xor(a1, off, 64);
        a2 += __shfl_xor(a2, off, 64);
        a3 += __shfl_xor(a3, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        s_part[0][threadIdx.x >> 6] = a1; s_part[1][threadIdx.x >> 6] = a2; s_part[2][threadIdx.x >> 6] = a3;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        double t = 0;
        for (int wv = 0; wv < (int)(blockDim.x >> 6); wv++) t += s_part[threadIdx.x][wv];
        norms[threadIdx.x * NORM_SLOTS + blockIdx.x] = t;
    } else if (threadIdx.x < NQ_ALL) {
        norms[threadIdx.x * NORM_SLOTS + blockIdx.x] = 0.0;
    }
}

__global__ void __launch_bounds__(256) k_sample_f3(int B, int m, const float* __restrict__ cp,
                                                   const float* __restrict__ width,
                                                   const uint8_t* __restrict__ is_bezier,
                                                   const SampleCoef* __restrict__ coef, float eps,
                                                   const double* __restrict__ norms, float* __restrict__ xyz,
                                                   float* __restrict__ rot, float* __restrict__ scaling) {
    __shared__ SampleCoef s_coef[MAX_M];
    __shared__ BlockConst s_bc;
    stage_consts(coef, m, norms, s_coef, &s_bc);
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= B * m) return;
    const int b = p / m, i = p - b * m;
    const float N1 = s_bc.N1, N2 = s_bc.N2;
    const CurveCP c = load_curve(cp, is_bezier, b);
    const float w = expf(width[b]);
    const SampleFwd s = sample_forward(c, s_coef[i], N1, N2, eps);
    float M[3][3], q[4];
    rot_matrix(s, M);
    quat_forward(M, q);
    xyz[3 * p] = s.xyz.x; xyz[3 * p + 1] = s.xyz.y; xyz[3 * p + 2] = s.xyz.z;
    reinterpret_cast<float4*>(rot)[p] = make_float4(q[0], q[1], q[2], q[3]);
    scaling[3 * p] = s.dist; scaling[3 * p + 1] = w; scaling[3 * p + 2] = w;
}

// ------------------------------------------------------------------------------------------------ backward
// Sums pass: one thread per splat (the launch covers them all).  The quaternion backward gives dL/d{v0, v1, v2}, the columns
// of the rotation: they feed the two grid-wide sums D2 and A and are cached in gv_cache for the curves pass.
__global__ void __launch_bounds__(SAMPLE_BLOCK) k_sample_bwd_sums(int B, int m, const float* __restrict__ cp,
                                                                  const uint8_t* __restrict__ is_bezier,
                                                                  const SampleCoef* __restrict__ coef, float eps,
                                                                  double* __restrict__ norms, const float* __restrict__ g_rot,
                                                                  float* __restrict__ gv_cache) {
    __shared__ SampleCoef s_coef[MAX_M];
    __shared__ BlockConst s_bc;
    stage_consts(coef, m, norms, s_coef, &s_bc);
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    NormTerms t = {0, 0};
    if (g_rot && p < B * m) {   // without a rotation gradient both sums are zero (the slots still get their +0)
        const int b = p / m, i = p - b * m;
        const SampleFwd s = sample_forward(load_curve(cp, is_bezier, b), s_coef[i], s_bc.N1, s_bc.N2, eps);
        V3 g_v0, g_v1, g_v2;
        quat_grad_to_axes(s, reinterpret_cast<const float4*>(g_rot)[p], g_v0, g_v1, g_v2);
        float* gv = gv_cache + p;   // planes [9][P]: a wave's accesses are contiguous
        const size_t PS = (size_t)B * m;
        gv[0] = g_v0.x; gv[PS] = g_v0.y; gv[2 * PS] = g_v0.z; gv[3 * PS] = g_v1.x; gv[4 * PS] = g_v1.y; gv[5 * PS] = g_v1.z;
        gv[6 * PS] = g_v2.x; gv[7 * PS] = g_v2.y; gv[8 * PS] = g_v2.z;
        t = norm_sum_terms(s, s_bc.N2, g_v1, g_v2);
    }
    const double acc[2] = {t.d2, t.a};
    block_accumulate<2>(acc, norms, 3);
}

// Curves pass: blocks hold whole curves (curve_slot).  Each sample's contribution to dL/d{curve_points, width}, from the
// cached dL/d{v0, v1, v2} and the two sums, is reduced to the 13 per-curve outputs through LDS.
__global__ void __launch_bounds__(SAMPLE_BLOCK) k_sample_bwd_curves(int B, int m, int curves_per_block,
                                                                    const float* __restrict__ cp,
                                                                    const float* __restrict__ width,
                                                                    const uint8_t* __restrict__ is_bezier,
                                                                    const SampleCoef* __restrict__ coef, float eps,
                                                                    const double* __restrict__ norms,
                                                                    const float* __restrict__ g_xyz, bool has_rot,
                                                                    const float* __restrict__ g_scaling,
                                                                    float* __restrict__ g_cp, float* __restrict__ g_width,
                                                                    const float* __restrict__ gv_cache) {
    __shared__ float s_part[CURVE_PART][SAMPLE_BLOCK + 1];
    __shared__ SampleCoef s_coef[MAX_M];
    __shared__ BlockConst s_bc;
    stage_consts(coef, m, norms, s_coef, &s_bc);
    const CurveSlot t = curve_slot(B, m, curves_per_block);
    CurveGrad cg = {};
    if (t.valid) {
        const CurveCP c = load_curve(cp, is_bezier, t.b);
        const SampleCoef k = s_coef[t.i];
        const size_t p = (size_t)t.b * m + t.i;
        const SampleFwd s = sample_forward(c, k, s_bc.N1, s_bc.N2, eps);
        V3 g_v0 = {0, 0, 0}, g_v1 = {0, 0, 0}, g_v2 = {0, 0, 0}, g_x = {0, 0, 0}, g_s = {0, 0, 0};
        if (has_rot) {
            const float* gv = gv_cache + p;   // planes [9][P]
            const size_t PS = (size_t)B * m;
            g_v0 = {gv[0], gv[PS], gv[2 * PS]}; g_v1 = {gv[3 * PS], gv[4 * PS], gv[5 * PS]}; g_v2 = {gv[6 * PS], gv[7 * PS], gv[8 * PS]};
        }
        if (g_xyz) g_x = {g_xyz[3 * p], g_xyz[3 * p + 1], g_xyz[3 * p + 2]};
        if (g_scaling) g_s = {g_scaling[3 * p], g_scaling[3 * p + 1], g_scaling[3 * p + 2]};
        cg = sample_backward_tail(c, k, s, expf(width[t.b]), eps, s_bc.N1, s_bc.N2, s_bc.D2, s_bc.D1, g_v0, g_v1, g_v2, g_x,
                                  g_scaling != nullptr, g_s);
    }
    // 13 outputs per curve, summed over its m samples in sample order (deterministic)
    curve_reduce(cg, s_part, B, m, curves_per_block, [&](int bb, int f, float sum) { store_curve_grad(g_cp, g_width, bb, f, sum, 0); });
}

// Closing pass of the FUSED view backward (k_view_bwd left, per curve, the 13 sums of the tail's gradient-dependent part in
// `part`): the part that carries the two grid-wide sums is evaluated from the curve alone -- tail(0, D2, D1) -- and added.
// Reads 48 + 52 bytes per curve, no per-splat data.
__global__ void __launch_bounds__(SAMPLE_BLOCK) k_sample_bwd_close(int B, int m, int curves_per_block, const float* __restrict__ cp,
                                                                   const float* __restrict__ width,
                                                                   const uint8_t* __restrict__ is_bezier,
                                                                   const SampleCoef* __restrict__ coef, float eps,
                                                                   const double* __restrict__ norms, const float* __restrict__ part,
                                                                   float* __restrict__ g_cp, float* __restrict__ g_width,
                                                                   int accumulate) {
    // thread = sample, blocks hold whole curves, like the curves pass.  (Thread = curve with a loop over its samples -- no LDS, no
    // barrier -- was measured: 14.6 against 9.3 us at cfg3, 20.3 against 19.5 at cfg5: 260 waves do not fill 1 024 SIMDs.)
    __shared__ float s_part[CURVE_PART][SAMPLE_BLOCK + 1];
    __shared__ SampleCoef s_coef[MAX_M];
    __shared__ BlockConst s_bc;
    stage_consts(coef, m, norms, s_coef, &s_bc);
    const CurveSlot t = curve_slot(B, m, curves_per_block);
    CurveGrad cg = {};
    if (t.valid) {
        const CurveCP c = load_curve(cp, is_bezier, t.b);
        const SampleCoef k = s_coef[t.i];
        const SampleFwd s = sample_forward(c, k, s_bc.N1, s_bc.N2, eps);
        const V3 z = {0.f, 0.f, 0.f};
        cg = sample_backward_tail(c, k, s, expf(width[t.b]), eps, s_bc.N1, s_bc.N2, s_bc.D2, s_bc.D1, z, z, z, z, false, z);
    }
    curve_reduce(cg, s_part, B, m, curves_per_block, [&](int bb, int f, float sum) {
        store_curve_grad(g_cp, g_width, bb, f, part[(size_t)bb * CURVE_PART + f] + sum, accumulate);
    });
}

// ------------------------------------------------------------------------------------------------ splat attributes
// Per-view derived per-splat inputs of the rasterizer (one thread per curve, m samples each):
//   rot_n   = F.normalize(rot_raw)                       (eps 1e-12)
//   opac    = sigmoid(opacity_logit[b]) [* mask]         mask = straight-through (sigmoid(mask_logit) > thr)
//   scl_out = scaling [* mask]
//   all_map = [ flip_toward_camera( R(rot_n)[:,0] ) @ view[:3,:3], 1 ]

__global__ void __launch_bounds__(256) k_attrs_fwd(int B, int m, const float* __restrict__ rot_raw,
                                                   const float* __restrict__ xyz,
                                                   const float* __restrict__ opacity_logit,
                                                   const float* __restrict__ mask_logit, float mask_thr,
                                                   const float* __restrict__ scaling,
                                                   const float* __restrict__ campos, const float* __restrict__ vm,
                                                   float* __restrict__ rot_n, float* __restrict__ opac,
                                                   float* __restrict__ scl_out, float* __restrict__ all_map) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= B * m) return;
    const int b = p / m;
    const V3 cam = {campos[0], campos[1], campos[2]};
    const float4 q = reinterpret_cast<const float4*>(rot_raw)[p];
    const V3 x = {xyz[3 * p], xyz[3 * p + 1], xyz[3 * p + 2]};
    const AttrsFwd a = attrs_forward(q, x, opacity_logit[b], mask_logit != nullptr, mask_logit ? mask_logit[p] : 0.f, mask_thr,
                                     cam, vm);
    reinterpret_cast<float4*>(rot_n)[p] = a.rot_n;
    opac[p] = a.opac;
    if (scl_out) {
        scl_out[3 * p] = scaling[3 * p] * a.mk; scl_out[3 * p + 1] = scaling[3 * p + 1] * a.mk;
        scl_out[3 * p + 2] = scaling[3 * p + 2] * a.mk;
    }
    reinterpret_cast<float4*>(all_map)[p] = a.all_map;
}

// Blocks hold whole curves (curves_per_block * m active threads); the per-curve opacity-logit gradient is the
// sample-ordered sum of its m per-splat terms (LDS).
__global__ void __launch_bounds__(SAMPLE_BLOCK) k_attrs_bwd(
    int B, int m, int curves_per_block, const float* __restrict__ rot_raw, const float* __restrict__ xyz,
    const float* __restrict__ opacity_logit, const float* __restrict__ mask_logit, float mask_thr,
    const float* __restrict__ scaling, const float* __restrict__ campos, const float* __restrict__ vm,
    const float* __restrict__ g_rot_n, const float* __restrict__ g_opac, const float* __restrict__ g_scl_out,
    const float* __restrict__ g_all_map, float* __restrict__ g_rot_raw, float* __restrict__ g_opacity_logit,
    float* __restrict__ g_mask_logit, float* __restrict__ g_scaling) {
    __shared__ float s_go[SAMPLE_BLOCK];
    const CurveSlot t = curve_slot(B, m, curves_per_block);
    const int b = t.b;
    float g_op_term = 0.f;
    if (t.valid) {
        const size_t p = (size_t)b * m + t.i;
        const V3 cam = {campos[0], campos[1], campos[2]};
        const float4 q = reinterpret_cast<const float4*>(rot_raw)[p];
        const V3 x = {xyz[3 * p], xyz[3 * p + 1], xyz[3 * p + 2]};
        const float4 gqn = g_rot_n ? reinterpret_cast<const float4*>(g_rot_n)[p] : make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 ga = g_all_map ? reinterpret_cast<const float4*>(g_all_map)[p] : make_float4(0.f, 0.f, 0.f, 0.f);
        V3 gs = {0.f, 0.f, 0.f}, sc = {0.f, 0.f, 0.f};
        if (g_scl_out) {
            gs = {g_scl_out[3 * p], g_scl_out[3 * p + 1], g_scl_out[3 * p + 2]};
            sc = {scaling[3 * p], scaling[3 * p + 1], scaling[3 * p + 2]};
        }
        const AttrsBwd o = attrs_backward(q, x, opacity_logit[b], mask_logit != nullptr, mask_logit ? mask_logit[p] : 0.f,
                                          mask_thr, cam, vm, gqn, g_all_map != nullptr, ga, g_opac ? g_opac[p] : 0.f,
                                          g_scl_out != nullptr, gs, sc);
        reinterpret_cast<float4*>(g_rot_raw)[p] = o.g_rot_raw;
        g_op_term = o.g_op_term;
        if (g_scl_out && g_scaling) { g_scaling[3 * p] = gs.x * o.mk; g_scaling[3 * p + 1] = gs.y * o.mk; g_scaling[3 * p + 2] = gs.z * o.mk; }
        if (g_mask_logit) g_mask_logit[p] = o.g_mask_logit;
    }
    s_go[threadIdx.x] = g_op_term;
    __syncthreads();
    if (t.valid && t.i == 0) {
        float sum = 0.f;
        for (int q = 0; q < m; q++) sum += s_go[threadIdx.x + q];
        g_opacity_logit[b] = sum;
    }
}

// ------------------------------------------------------------------------------------------------ launchers
// Workgroup size of the norm pass (always NORM_SLOTS workgroups): 256 threads up to 128 k splats, 512 up to 600 k, 1024 beyond.
// Big workgroups only fit a CU once several compositor waves of the neighbouring views have drained; with three views in
// flight at cfg3, 1024 threads cost 0.6 % of the headline against 256 / 512 (same box, twice: 813 - 814 vs 818 - 821 Msplats/s),
// while a million splats want the shorter per-thread loop.
static int f12_threads(long long P) { return P <= 128 * 1024 ? 256 : (P <= 600 * 1024 ? 512 : 1024); }

void launch_sample_norms(hipStream_t s, int B, int m, const float* cp, const uint8_t* is_bezier, const void* coef, double* norms) {
    ProfScope p("sample_f12", s);
    hipLaunchKernelGGL(k_sample_f12, dim3(NORM_SLOTS), dim3(f12_threads((long long)B * m)), 0, s, B, m, cp, is_bezier,
                       reinterpret_cast<const SampleCoef*>(coef), norms);
}
void launch_sample_forward(hipStream_t s, int B, int m, const float* cp, const float* width, const uint8_t* is_bezier,
                           const void* coef, float eps, double* norms, float* xyz, float* rot, float* scaling) {
    launch_sample_norms(s, B, m, cp, is_bezier, coef, norms);
    ProfScope p("sample_f3", s);
    hipLaunchKernelGGL(k_sample_f3, dim3((B * m + 255) / 256), dim3(256), 0, s, B, m, cp, width, is_bezier,
                       reinterpret_cast<const SampleCoef*>(coef), eps, norms, xyz, rot, scaling);
}
void launch_sample_backward(hipStream_t s, int B, int m, const float* cp, const float* width, const uint8_t* is_bezier,
                            const void* coef, float eps, double* norms, const float* g_xyz, const float* g_rot,
                            const float* g_scaling, float* g_cp, float* g_width, float* gv_cache) {
    const CurveLaunch cl = curve_launch(B, m);
    const dim3 block(SAMPLE_BLOCK), sgrid(std::max((B * m + SAMPLE_BLOCK - 1) / SAMPLE_BLOCK, 1));   // one thread per splat
    const SampleCoef* k = reinterpret_cast<const SampleCoef*>(coef);
    { ProfScope p("sample_b1", s); hipLaunchKernelGGL(k_sample_bwd_sums, sgrid, block, 0, s, B, m, cp, is_bezier, k, eps, norms, g_rot, gv_cache); }
    { ProfScope p("sample_b3", s); hipLaunchKernelGGL(k_sample_bwd_curves, cl.grid, block, 0, s, B, m, cl.cpb, cp, width, is_bezier, k, eps, norms, g_xyz, g_rot != nullptr, g_scaling, g_cp, g_width, gv_cache); }
}
void launch_attrs_forward(hipStream_t s, int B, int m, const float* rot_raw, const float* xyz, const float* opacity_logit,
                          const float* mask_logit, float mask_thr, const float* scaling, const float* campos,
                          const float* vm, float* rot_n, float* opac, float* scl_out, float* all_map) {
    ProfScope p("attrs_fwd", s);
    hipLaunchKernelGGL(k_attrs_fwd, dim3((B * m + 255) / 256), dim3(256), 0, s, B, m, rot_raw, xyz, opacity_logit, mask_logit,
                       mask_thr, scaling, campos, vm, rot_n, opac, scl_out, all_map);
}
void launch_attrs_backward(hipStream_t s, int B, int m, const float* rot_raw, const float* xyz,
                           const float* opacity_logit, const float* mask_logit, float mask_thr, const float* scaling,
                           const float* campos, const float* vm, const float* g_rot_n, const float* g_opac,
                           const float* g_scl_out, const float* g_all_map, float* g_rot_raw, float* g_opacity_logit,
                           float* g_mask_logit, float* g_scaling) {
    ProfScope p("attrs_bwd", s);
    const CurveLaunch cl = curve_launch(B, m);
    hipLaunchKernelGGL(k_attrs_bwd, cl.grid, dim3(SAMPLE_BLOCK), 0, s, B, m, cl.cpb, rot_raw, xyz, opacity_logit, mask_logit,
                       mask_thr, scaling, campos, vm, g_rot_n, g_opac, g_scl_out, g_all_map, g_rot_raw, g_opacity_logit,
                       g_mask_logit, g_scaling);
}

void launch_sample_backward_close(hipStream_t s, int B, int m, const float* cp, const float* width, const uint8_t* is_bezier,
                                  const void* coef, float eps, const double* norms, const float* part, float* g_cp, float* g_width,
                                  int accumulate) {
    const CurveLaunch cl = curve_launch(B, m);
    ProfScope p("sample_b3", s);
    hipLaunchKernelGGL(k_sample_bwd_close, cl.grid, dim3(SAMPLE_BLOCK), 0, s, B, m, cl.cpb, cp, width, is_bezier,
                       reinterpret_cast<const SampleCoef*>(coef), eps, norms, part, g_cp, g_width, accumulate);
}

int sample_norm_words() { return NORM_WORDS; }
int sample_norm_fwd_words() { return NQ_FWD * NORM_SLOTS; }

}  // namespace cgs
