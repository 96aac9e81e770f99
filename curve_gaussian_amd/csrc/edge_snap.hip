// Per-sample normal equations of "move me onto the nearest detected edge in every image" (include/curvegs.h,
// cgs_sample_snap_terms; ops/edge_snap.py solves them per sample on the host and refits the edges' control points).
//   k_sample_snap_terms   the shape of k_sample_support (edge_trim.hip): one thread per sample, the view loop inside the
//                         thread, so the view index is wave-uniform and the 16 doubles of a camera are scalar loads; a wave's
//                         64 consecutive samples -- neighbours on their edge -- gather neighbouring 2 x 2 footprints of one
//                         plane of the distance transform.  The point is projected with nv_project_xyz (point_projection.h),
//                         so no entry disagrees on a boundary point; the camera-space point it divides is formed again by the
//                         same expressions (the compiler shares them).  The distances are sqrt(k) of the integer transform,
//                         looked up in a table of at most 65 doubles that the host computed: the kernel takes no square root,
//                         so both back ends read the same bits.  The table is staged in LDS once per workgroup -- a per-lane
//                         index is a gather either way, and LDS answers it without a trip to the vector cache -- which makes
//                         this the one barrier of the kernel: every thread reaches it, a thread without a sample leaves after.
//                         The thread loads its own row of 10 doubles and its view count FIRST, adds view by view in view
//                         order and stores them: one owner per row, no atomics, and the same floating-point sequence however
//                         the views are cut into calls.  Everything is float64, one rounded operation at a time (contraction
//                         off, IEEE division), in the order frozen in the header.
//                         A template over GATED: false is cgs_sample_snap_terms as it always was; true is
//                         cgs_sample_snap_terms_depth -- nv_verdict (point_projection.h) drops a view whose depth plane hides
//                         the sample right after the projection's verdict, before the footprint test: no term, no view, and
//                         for every other view the floating-point sequence of the ungated kernel.
#include "kernels.h"
#include "point_projection.h"

namespace cgs {

constexpr int SNAP_THREADS = 256;
static_assert(CGS_SNAP_TERMS == 10, "Axx Axy Axz Ayy Ayz Azz bx by bz rr");

template <bool GATED>
__global__ void __launch_bounds__(SNAP_THREADS) k_sample_snap_terms(int P, const float* __restrict__ pts, int V,
                                                                    const double* __restrict__ intr,
                                                                    const double* __restrict__ w2c, int height, int width,
                                                                    const int* __restrict__ d2, int cap2,
                                                                    const double* __restrict__ dist_lut,
                                                                    double* __restrict__ terms, int* __restrict__ views,
                                                                    const float* __restrict__ depth, double slack,
                                                                    int* __restrict__ hidden) {
#pragma clang fp contract(off)
    __shared__ double lut[CGS_SNAP_MAX_CAP2 + 1];
    for (int k = threadIdx.x; k <= cap2; k += SNAP_THREADS) lut[k] = dist_lut[k];   // cap2 <= CGS_SNAP_MAX_CAP2 (the entry)
    __syncthreads();
    const long long i = (long long)blockIdx.x * SNAP_THREADS + threadIdx.x;
    if (i >= P) return;   // after the one barrier
    double* __restrict__ row = terms + (size_t)i * CGS_SNAP_TERMS;   // the thread's own row: a plain read-modify-write
    double Axx = row[0], Axy = row[1], Axz = row[2], Ayy = row[3], Ayz = row[4], Azz = row[5];
    double bx = row[6], by = row[7], bz = row[8], rr = row[9];
    int n = views[i], hid = 0;
    const double X = (double)pts[3 * i + 0], Y = (double)pts[3 * i + 1], Z = (double)pts[3 * i + 2];
    const double wd = (double)width, hd = (double)height;
    const size_t plane = (size_t)height * (size_t)width;
    for (int view = 0; view < V; view++) {   // wave-uniform
        NvCam c;
        nv_load_cam(c, intr, w2c, view);
        // the camera-space point of nv_project_xyz, by its expressions and ahead of it, so that the compiler keeps one copy
        // of the two divisions (a quotient by c2 <= 0 is formed and never used)
        const double c0 = ((c.m[0] * X + c.m[1] * Y) + c.m[2] * Z) + c.m[3];
        const double c1 = ((c.m[4] * X + c.m[5] * Y) + c.m[6] * Z) + c.m[7];
        const double c2 = ((c.m[8] * X + c.m[9] * Y) + c.m[10] * Z) + c.m[11];
        const double x = c0 / c2, y = c1 / c2;
        double u, v;
        const NvVerdict verdict = nv_verdict<GATED>(c, X, Y, Z, wd, hd, GATED ? depth + (size_t)view * plane : nullptr, width,
                                                    slack, u, v);
        if (verdict == NV_OUT) continue;
        if (GATED && verdict == NV_HIDDEN) {   // no term, no view
            hid++;
            continue;
        }
        // the footprint: the four pixel centres around (u, v); 0 <= u < W <= 16384, so the floors fit an int
        const double a = u - 0.5, b = v - 0.5;
        const double fj = floor(a), fi = floor(b);
        const int j0 = (int)fj, i0 = (int)fi;
        if (j0 < 0 || j0 + 1 > width - 1 || i0 < 0 || i0 + 1 > height - 1) continue;   // nothing is read outside the plane
        const int* __restrict__ q = d2 + (size_t)view * plane + (size_t)i0 * (size_t)width + (size_t)j0;
        const int k00 = q[0], k01 = q[1], k10 = q[width], k11 = q[(size_t)width + 1];
        // the capture, BEFORE the table is indexed: CGS_EDT_INF of an empty mask is far past its end
        if (k00 < 0 || k00 > cap2 || k01 < 0 || k01 > cap2 || k10 < 0 || k10 > cap2 || k11 < 0 || k11 > cap2) continue;
        const double d00 = lut[k00], d01 = lut[k01], d10 = lut[k10], d11 = lut[k11];
        const double fa = a - fj, fb = b - fi;
        const double ga = 1.0 - fa, gb = 1.0 - fb;
        const double r = gb * (ga * d00 + fa * d01) + fb * (ga * d10 + fa * d11);
        const double gu = gb * (d01 - d00) + fb * (d11 - d10);
        const double gv = ga * (d10 - d00) + fa * (d11 - d01);
        const double su = (gu * c.f[0]) / c2, sv = (gv * c.f[1]) / c2;
        const double gc = -(su * x + sv * y);
        const double gx = (c.m[0] * su + c.m[4] * sv) + c.m[8] * gc;
        const double gy = (c.m[1] * su + c.m[5] * sv) + c.m[9] * gc;
        const double gz = (c.m[2] * su + c.m[6] * sv) + c.m[10] * gc;
        Axx += gx * gx;
        Axy += gx * gy;
        Axz += gx * gz;
        Ayy += gy * gy;
        Ayz += gy * gz;
        Azz += gz * gz;
        bx += gx * r;
        by += gy * r;
        bz += gz * r;
        rr += r * r;
        n++;
    }
    row[0] = Axx, row[1] = Axy, row[2] = Axz, row[3] = Ayy, row[4] = Ayz, row[5] = Azz;
    row[6] = bx, row[7] = by, row[8] = bz, row[9] = rr;
    views[i] = n;
    if (GATED && hidden) hidden[i] += hid;   // added, like the sums: the thread's own word
}

template <bool GATED>
static void sample_snap_terms_launch(hipStream_t s, int P, const float* points, int V, const double* intr, const double* w2c,
                                     int height, int width, const int* d2, int cap2, const double* dist_lut, double* terms,
                                     int* views, DepthGate gate, int* hidden) {
    const unsigned blocks = (unsigned)(((long long)P + SNAP_THREADS - 1) / SNAP_THREADS);   // at most 2^23: one grid dimension
    ProfScope p(GATED ? "sample_snap_terms_depth" : "sample_snap_terms", s);
    hipLaunchKernelGGL(k_sample_snap_terms<GATED>, dim3(blocks), dim3(SNAP_THREADS), 0, s, P, points, V, intr, w2c, height,
                       width, d2, cap2, dist_lut, terms, views, gate.depth, gate.slack, hidden);
}

void launch_sample_snap_terms(hipStream_t s, int P, const float* points, int V, const double* intr, const double* w2c,
                              int height, int width, const int* d2, int cap2, const double* dist_lut, const DepthGate* gate,
                              double* terms, int* views, int* hidden) {
    if (gate)
        sample_snap_terms_launch<true>(s, P, points, V, intr, w2c, height, width, d2, cap2, dist_lut, terms, views, *gate,
                                       hidden);
    else
        sample_snap_terms_launch<false>(s, P, points, V, intr, w2c, height, width, d2, cap2, dist_lut, terms, views,
                                        DepthGate{nullptr, 0.0}, nullptr);
}

}  // namespace cgs
