// Edge-map visibility check of the extraction step: for every edge (a Bezier's 4 control points or a line's 2 end
// points), the number of frames in which its projected points fall on the 2D edge detector's response.  Replaces the
// (edge, frame) Python double loop of the reference's compute_visibility (edge_extraction/extract_para_edge.py:145-197).
//
// Per (edge, frame) cell: each point X is projected as x = K (R X + T) in float64 and divided by x[2] (no z > 0 test: a
// point behind the camera projects mirrored; z = 0 gives inf / NaN and the point is dropped), rounded half to even
// (np.round), and kept if 0 <= u < width and 0 <= v < height.  With no kept point the cell is 0; otherwise it is
// mean(values) > 0.1 && max(values) > 0.5, where value = u8 / 255.0 (PidiNet) or 1 - u8 / 255.0 (DexiNed, `invert`).
//
// Exactness: contraction into FMAs is off in the kernel, divisions are IEEE, rounding is rint; every dot product is
// ((a0*b0 + a1*b1) + a2*b2) + t and the mean is (((v0 + v1) + v2) + v3) / n, the order np.mean takes over <= 4 values.
//
// Shape: lanes over edges (256 per workgroup), grid.y over slices of consecutive frames, so a frame's camera is
// wave-uniform (scalar loads) and the workgroups of one slice gather from the same few maps, which stay in L2.  A lane
// counts its cells over the slice in a register and adds the count with one integer atomicAdd per (edge, slice):
// integer sums do not depend on arrival order, so the counts are deterministic.  Map offsets are 64-bit.
//
// The depth gate (include/curvegs.h, cgs_edge_visibility_depth): k_edge_visibility is a template over GATED.  false is
// cgs_edge_visibility as it always was -- depth, slack and the second counter are not touched.  true drops a kept point
// that the frame's depth plane hides, exactly as an out-of-image point is dropped.  The rule, float64, no contraction:
//   raw coordinates ur = x0 / x2, vr = x1 / x2; the camera depth is c2, the third row of w2c X (not x2);
//   a point kept by rounding is HIDDEN iff ur >= 0 && vr >= 0 && nv_hidden(plane_f, width, ur, vr, c2, slack)
//   (point_projection.h: c2 > float64(plane_f[floor(vr)][floor(ur)]) + slack).
// Two pixel conventions meet here: the edge map is read at the ROUNDED pixel, as the reference reads it; the plane at the
// FLOORED one, the convention the planes are drawn in (a pixel centre is (j + 0.5, i + 0.5)).  A point kept by rounding
// with ur or vr in [-0.5, 0) has no plane pixel and is never hidden; rint(ur) <= W - 1 implies floor(ur) <= W - 1, so there
// is no upper test.  A mirrored point (c2 <= 0) is never hidden by a positive plane; a NaN plane entry hides nothing.  A
// hidden point enters neither the sum, the maximum nor nv; a cell whose points are all hidden is 0.  The gated kernel
// counts, per edge, the visible frames and the frames in which the gate dropped at least one of its points: two register
// counters, at most two integer atomicAdds per (edge, slice).
#include "kernels.h"
#include "point_projection.h"

namespace cgs {

constexpr int VIS_BLOCK = 256;         // edges per workgroup
constexpr int VIS_TARGET_WGS = 2048;   // ~8 workgroups per CU on 256 CUs before the frames are sliced further

// Zeroes the counts with a kernel, not hipMemsetAsync (see zero_async in api.hip: a captured memset node clears once).
__global__ void __launch_bounds__(VIS_BLOCK) k_edge_visibility_init(int n, int* __restrict__ counts) {
    const int i = blockIdx.x * VIS_BLOCK + threadIdx.x;
    if (i < n) counts[i] = 0;
}

template <bool GATED>
__global__ void __launch_bounds__(VIS_BLOCK) k_edge_visibility(int n_curves, const double* __restrict__ curves,
                                                              int n_lines, const double* __restrict__ lines,
                                                              int n_frames, int per_slice,
                                                              const double* __restrict__ K,
                                                              const double* __restrict__ w2c, int height, int width,
                                                              const unsigned char* __restrict__ maps, int invert,
                                                              int* __restrict__ counts,
                                                              const float* __restrict__ depth, double slack) {
#pragma clang fp contract(off)
    const int e = blockIdx.x * VIS_BLOCK + threadIdx.x;
    if (e >= n_curves + n_lines) return;
    double P[4][3];
    int np;
    if (e < n_curves) {
        np = 4;
        const double* c = curves + 12 * (size_t)e;
#pragma unroll
        for (int k = 0; k < 12; k++) P[k / 3][k % 3] = c[k];
    } else {
        np = 2;
        const double* l = lines + 6 * (size_t)(e - n_curves);
#pragma unroll
        for (int k = 0; k < 6; k++) P[k / 3][k % 3] = l[k];
#pragma unroll
        for (int k = 6; k < 12; k++) P[k / 3][k % 3] = 0.0;
    }
    const size_t plane = (size_t)height * (size_t)width;
    const double wd = (double)width, hd = (double)height;
    const int f0 = blockIdx.y * per_slice;
    const int f1 = min(n_frames, f0 + per_slice);
    int cnt = 0, touched = 0;   // touched: GATED only
    for (int f = f0; f < f1; f++) {
        const double* k = K + 9 * (size_t)f;
        const double* m = w2c + 12 * (size_t)f;
        const unsigned char* map = maps + (size_t)f * plane;
        const float* __restrict__ dplane = GATED ? depth + (size_t)f * plane : nullptr;
        double sum = 0.0, mx = 0.0;
        int nv = 0;
        bool dropped = false;
        for (int p = 0; p < np; p++) {
            const double X = P[p][0], Y = P[p][1], Z = P[p][2];
            const double c0 = ((m[0] * X + m[1] * Y) + m[2] * Z) + m[3];
            const double c1 = ((m[4] * X + m[5] * Y) + m[6] * Z) + m[7];
            const double c2 = ((m[8] * X + m[9] * Y) + m[10] * Z) + m[11];
            const double x0 = (k[0] * c0 + k[1] * c1) + k[2] * c2;
            const double x1 = (k[3] * c0 + k[4] * c1) + k[5] * c2;
            const double x2 = (k[6] * c0 + k[7] * c1) + k[8] * c2;
            const double ur = x0 / x2;
            const double vr = x1 / x2;
            const double u = rint(ur);
            const double v = rint(vr);
            // NaN and +-inf fail these tests, as does anything np.int32 would turn into INT_MIN; -0.0 is pixel 0
            if (u >= 0.0 && u < wd && v >= 0.0 && v < hd) {
                if constexpr (GATED) {
                    // 0 <= ur, rint(ur) <= W - 1, so 0 <= floor(ur) <= W - 1 (likewise vr): inside the frame's plane
                    if (ur >= 0.0 && vr >= 0.0 && nv_hidden(dplane, width, ur, vr, c2, slack)) {
                        dropped = true;
                        continue;
                    }
                }
                const double raw = (double)map[(size_t)v * (size_t)width + (size_t)u] / 255.0;
                const double val = invert ? 1.0 - raw : raw;
                sum = sum + val;
                mx = nv == 0 ? val : fmax(mx, val);
                nv++;
            }
        }
        if (nv > 0 && sum / (double)nv > 0.1 && mx > 0.5) cnt++;
        if (GATED && dropped) touched++;
    }
    if constexpr (GATED) {   // counts is [E,2]: visible frames, frames the gate touched
        if (cnt) atomicAdd(&counts[2 * (size_t)e], cnt);
        if (touched) atomicAdd(&counts[2 * (size_t)e + 1], touched);
    } else {
        if (cnt) atomicAdd(&counts[e], cnt);
    }
}

// Frames per slice: enough slices to bring the grid to ~VIS_TARGET_WGS workgroups, never more slices than frames.
static int visibility_per_slice(int n_edges, int n_frames) {
    const int eblocks = (n_edges + VIS_BLOCK - 1) / VIS_BLOCK;
    int slices = (VIS_TARGET_WGS + eblocks - 1) / eblocks;
    slices = max(1, min(slices, n_frames));
    return (n_frames + slices - 1) / slices;
}

template <bool GATED>
static void edge_visibility_launches(hipStream_t s, int n_curves, const double* curves, int n_lines, const double* lines,
                                     int n_frames, const double* K, const double* w2c, int height, int width,
                                     const unsigned char* maps, int invert, int* counts, DepthGate gate) {
    const int n_edges = n_curves + n_lines;
    const int eblocks = (n_edges + VIS_BLOCK - 1) / VIS_BLOCK;
    const int n_out = GATED ? 2 * n_edges : n_edges;   // n_edges <= 2^30: 2 n_edges - 1 + VIS_BLOCK fits an int
    hipLaunchKernelGGL(k_edge_visibility_init, dim3((n_out - 1) / VIS_BLOCK + 1), dim3(VIS_BLOCK), 0, s, n_out, counts);
    if (n_frames == 0) return;
    const int per = visibility_per_slice(n_edges, n_frames);
    const int slices = (n_frames + per - 1) / per;
    ProfScope p(GATED ? "edge_visibility_depth" : "edge_visibility", s);
    hipLaunchKernelGGL(k_edge_visibility<GATED>, dim3(eblocks, slices), dim3(VIS_BLOCK), 0, s, n_curves, curves, n_lines,
                       lines, n_frames, per, K, w2c, height, width, maps, invert, counts, gate.depth, gate.slack);
}

void launch_edge_visibility(hipStream_t s, int n_curves, const double* curves, int n_lines, const double* lines,
                            int n_frames, const double* K, const double* w2c, int height, int width,
                            const unsigned char* maps, int invert, const DepthGate* gate, int* counts) {
    if (gate)
        edge_visibility_launches<true>(s, n_curves, curves, n_lines, lines, n_frames, K, w2c, height, width, maps, invert,
                                       counts, *gate);
    else
        edge_visibility_launches<false>(s, n_curves, curves, n_lines, lines, n_frames, K, w2c, height, width, maps, invert,
                                        counts, DepthGate{nullptr, 0.0});
}

}  // namespace cgs
