// Line fitting and merging of the curve model (GaussianCurveModel.fit_curve_to_line / merge_curves, reference
// scene/gaussian_curve_model.py:459-632 over edge_extraction/fitting.py and merging.py; scene/topology.py here): the three
// data-parallel parts of the two edits as kernels, the greedy pairing and the model surgery stay on the host.
//   k_curve_straightness     is_curve_straight for every curve at once: one wave per curve
//   k_segment_adjacency      the close-and-parallel predicate of every pair of straight segments as an n x ceil(n/64) bit matrix
//   k_segment_components     connected components of that matrix (smallest member index as the label): one workgroup
//   k_pair_consensus_fit     per pair of Bezier curves: exhaustive two-point line consensus, line through the inliers,
//                            ordering along it, least-squares cubic Bezier: one workgroup per pair
// All arithmetic is float64 on float32 inputs.  Every result is deterministic: no floating-point atomics, wave reductions
// are xor butterflies (one fixed tree), block reductions run in a fixed order; the only atomics are integer minima whose
// result does not depend on their order.  None of the kernels is memory-bound or tuned: B and K are in the hundreds to
// thousands, the cost is latency and (for the consensus) float64 arithmetic: ~15 operations x N (N - 1) / 2 candidate lines
// x N points per pair, 60 MFLOP at N = 200.
#include <algorithm>

#include "kernels.h"

namespace cgs {

constexpr int CF_WAVE = 64;
constexpr int CF_STRAIGHT_THREADS = 256;   // 4 waves = 4 curves per workgroup
constexpr int CF_ADJ_THREADS = 256;        // 4 waves = 4 words of the bit matrix per workgroup
constexpr int CF_CC_THREADS = 1024;        // 16 waves share the rows of the bit matrix
constexpr int CF_PAIR_THREADS = 256;
constexpr int CF_PAIR_WAVES = CF_PAIR_THREADS / CF_WAVE;
constexpr int CF_PAIR_MAX_POINTS = 2 * CGS_CURVE_FIT_MAX_SAMPLES;

__device__ __forceinline__ double wsum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, CF_WAVE);
    return v;
}
__device__ __forceinline__ double wmin(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmin(v, __shfl_xor(v, off, CF_WAVE));
    return v;
}
__device__ __forceinline__ double wmax(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off, CF_WAVE));
    return v;
}

// orders one wave's LDS writes before its later LDS reads (the lanes run in lockstep; only the compiler has to be held)
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// cubic Bernstein weights at t
__device__ __forceinline__ void bernstein(double t, double w[4]) {
    const double s = 1.0 - t;
    w[0] = s * s * s;
    w[1] = 3.0 * s * s * t;
    w[2] = 3.0 * s * t * t;
    w[3] = t * t * t;
}

// Unit eigenvector of the largest eigenvalue of the symmetric matrix [[a00 a01 a02] [a01 a11 a12] [a02 a12 a22]]: cyclic
// Jacobi rotations (each one exactly orthogonal up to rounding, so the vector's error is eps / relative eigengap).  A zero
// matrix returns the first axis; nothing here divides by a quantity that can be zero.
__device__ void principal_axis(double a00, double a01, double a02, double a11, double a12, double a22, double dir[3]) {
    double A[3][3] = {{a00, a01, a02}, {a01, a11, a12}, {a02, a12, a22}};
    double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int sweep = 0; sweep < 16; sweep++) {
        const double off = fabs(A[0][1]) + fabs(A[0][2]) + fabs(A[1][2]);
        const double diag = fabs(A[0][0]) + fabs(A[1][1]) + fabs(A[2][2]);
        if (off <= 1e-300 || off <= 1e-19 * diag) break;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int p = k == 2 ? 1 : 0, q = k == 0 ? 1 : 2;   // (0,1) (0,2) (1,2)
            const double apq = A[p][q];
            if (apq == 0.0) continue;
            const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
            // the smaller root of t^2 + 2 theta t - 1 = 0; an infinite theta gives t = 0
            const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
            const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
            A[p][p] -= t * apq;
            A[q][q] += t * apq;
            A[p][q] = A[q][p] = 0.0;
            const int r = 3 - p - q;
            const double arp = A[r][p], arq = A[r][q];
            A[r][p] = A[p][r] = c * arp - s * arq;
            A[r][q] = A[q][r] = s * arp + c * arq;
#pragma unroll
            for (int i = 0; i < 3; i++) {
                const double vip = V[i][p], viq = V[i][q];
                V[i][p] = c * vip - s * viq;
                V[i][q] = s * vip + c * viq;
            }
        }
    }
    int m = 0;
    if (A[1][1] > A[m][m]) m = 1;
    if (A[2][2] > A[m][m]) m = 2;
    double d0 = V[0][m], d1 = V[1][m], d2 = V[2][m];
    const double n = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
    if (n > 0.0) { d0 /= n; d1 /= n; d2 /= n; } else { d0 = 1.0; d1 = d2 = 0.0; }
    dir[0] = d0; dir[1] = d1; dir[2] = d2;
}

// ------------------------------------------------------------------------------------------------ straightness
__global__ void __launch_bounds__(CF_STRAIGHT_THREADS) k_curve_straightness(int B, const float* __restrict__ cp,
                                                                            const uint8_t* __restrict__ is_bezier, int n,
                                                                            double thr, double thr_max,
                                                                            double* __restrict__ mean_dist,
                                                                            double* __restrict__ max_dist,
                                                                            uint8_t* __restrict__ straight) {
    const int lane = threadIdx.x & (CF_WAVE - 1);
    const int b = blockIdx.x * (CF_STRAIGHT_THREADS / CF_WAVE) + (threadIdx.x >> 6);
    if (b >= B) return;    // whole waves leave: the shuffles below always see 64 lanes
    double P[4][3];
#pragma unroll
    for (int k = 0; k < 12; k++) P[k / 3][k % 3] = (double)cp[(size_t)b * 12 + k];
    // the samples of this lane (i = lane, lane + 64, ...), at most CGS_CURVE_FIT_MAX_SAMPLES / 64 of them, recomputed per pass
    constexpr int PER = CGS_CURVE_FIT_MAX_SAMPLES / CF_WAVE;
    const double inv = 1.0 / (double)(n - 1), dn = (double)n;
    auto sample = [&](int i, double x[3]) {
        double w[4];
        bernstein((double)i * inv, w);
#pragma unroll
        for (int c = 0; c < 3; c++) x[c] = w[0] * P[0][c] + w[1] * P[1][c] + w[2] * P[2][c] + w[3] * P[3][c];
    };
    double s[3] = {0, 0, 0};
    for (int k = 0; k < PER; k++) {
        const int i = lane + k * CF_WAVE;
        if (i < n) {
            double x[3];
            sample(i, x);
            s[0] += x[0]; s[1] += x[1]; s[2] += x[2];
        }
    }
    const double m[3] = {wsum(s[0]) / dn, wsum(s[1]) / dn, wsum(s[2]) / dn};
    double c6[6] = {0, 0, 0, 0, 0, 0};
    for (int k = 0; k < PER; k++) {
        const int i = lane + k * CF_WAVE;
        if (i < n) {
            double x[3];
            sample(i, x);
            const double a = x[0] - m[0], bb = x[1] - m[1], c = x[2] - m[2];
            c6[0] += a * a; c6[1] += a * bb; c6[2] += a * c; c6[3] += bb * bb; c6[4] += bb * c; c6[5] += c * c;
        }
    }
#pragma unroll
    for (int k = 0; k < 6; k++) c6[k] = wsum(c6[k]) / dn;
    double d[3];
    principal_axis(c6[0], c6[1], c6[2], c6[3], c6[4], c6[5], d);
    double tmin = INFINITY, tmax = -INFINITY;
    for (int k = 0; k < PER; k++) {
        const int i = lane + k * CF_WAVE;
        if (i < n) {
            double x[3];
            sample(i, x);
            const double t = (x[0] - m[0]) * d[0] + (x[1] - m[1]) * d[1] + (x[2] - m[2]) * d[2];
            tmin = fmin(tmin, t);
            tmax = fmax(tmax, t);
        }
    }
    tmin = wmin(tmin);
    tmax = wmax(tmax);
    double dsum = 0.0, dmax = 0.0;
    for (int k = 0; k < PER; k++) {
        const int i = lane + k * CF_WAVE;
        if (i < n) {
            double x[3];
            sample(i, x);
            double t = (x[0] - m[0]) * d[0] + (x[1] - m[1]) * d[1] + (x[2] - m[2]) * d[2];
            t = fmin(fmax(t, tmin), tmax);
            const double e0 = x[0] - (m[0] + t * d[0]), e1 = x[1] - (m[1] + t * d[1]), e2 = x[2] - (m[2] + t * d[2]);
            const double dist = sqrt(e0 * e0 + e1 * e1 + e2 * e2);
            dsum += dist;
            dmax = fmax(dmax, dist);
        }
    }
    const double mean = wsum(dsum) / dn;
    dmax = wmax(dmax);
    if (lane == 0) {
        mean_dist[b] = mean;
        max_dist[b] = dmax;
        straight[b] = (is_bezier[b] != 0 && mean < thr && dmax < thr_max) ? 1 : 0;
    }
}

void launch_curve_straightness(hipStream_t s, int B, const float* cp, const uint8_t* is_bezier, int sample_num,
                               double thr, double thr_max, double* mean_dist, double* max_dist, uint8_t* straight) {
    ProfScope pr("curve_straightness", s);
    const int per = CF_STRAIGHT_THREADS / CF_WAVE;
    hipLaunchKernelGGL(k_curve_straightness, dim3((B + per - 1) / per), dim3(CF_STRAIGHT_THREADS), 0, s, B, cp, is_bezier,
                       sample_num, thr, thr_max, mean_dist, max_dist, straight);
}

// ------------------------------------------------------------------------------------------------ segment merge labels
// distance of point q to the segment p + u d, u in [0, 1] (dd = d . d > 0)
__device__ __forceinline__ double point_segment(const double p[3], const double d[3], double dd, const double q[3]) {
    const double r0 = q[0] - p[0], r1 = q[1] - p[1], r2 = q[2] - p[2];
    double u = (r0 * d[0] + r1 * d[1] + r2 * d[2]) / dd;
    u = fmin(fmax(u, 0.0), 1.0);
    const double e0 = p[0] + u * d[0] - q[0], e1 = p[1] + u * d[1] - q[1], e2 = p[2] + u * d[2] - q[2];
    return sqrt(e0 * e0 + e1 * e1 + e2 * e2);
}

// One wave per 64-bit word (row i, columns 64 w .. 64 w + 63) of the bit matrix: lane l decides the pair (i, 64 w + l), the
// ballot is the word.  For a < b the edge is  |cos(dir a, dir b)| >= sim_thr  &&  min(dist(b.start, a), dist(b.end, a)) <=
// dist_thr; the pair (i, j) is evaluated as (min, max), so the matrix is symmetric by construction.  A segment of zero
// length has no edge.  Every word is written, the bits past column n - 1 as zeros: the workspace needs no initialisation.
__global__ void __launch_bounds__(CF_ADJ_THREADS) k_segment_adjacency(int n, int W, const float* __restrict__ seg,
                                                                      double dist_thr, double sim_thr,
                                                                      unsigned long long* __restrict__ bits) {
    const int lane = threadIdx.x & (CF_WAVE - 1);
    const long long word = (long long)blockIdx.x * (CF_ADJ_THREADS / CF_WAVE) + (threadIdx.x >> 6);
    if (word >= (long long)n * W) return;
    const int i = (int)(word / W), w = (int)(word % W);
    const int j = w * CF_WAVE + lane;
    bool edge = false;
    if (j < n && j != i) {
        const int a = min(i, j), b = max(i, j);
        double pa[3], da[3], qs[3], qe[3], db[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            pa[c] = (double)seg[(size_t)a * 6 + c];
            da[c] = (double)seg[(size_t)a * 6 + 3 + c] - pa[c];
            qs[c] = (double)seg[(size_t)b * 6 + c];
            qe[c] = (double)seg[(size_t)b * 6 + 3 + c];
            db[c] = qe[c] - qs[c];
        }
        const double daa = da[0] * da[0] + da[1] * da[1] + da[2] * da[2];
        const double dbb = db[0] * db[0] + db[1] * db[1] + db[2] * db[2];
        if (daa > 0.0 && dbb > 0.0) {
            const double na = sqrt(daa), nb = sqrt(dbb);
            const double cs = fabs((da[0] / na) * (db[0] / nb) + (da[1] / na) * (db[1] / nb) + (da[2] / na) * (db[2] / nb));
            const double dist = fmin(point_segment(pa, da, daa, qs), point_segment(pa, da, daa, qe));
            edge = cs >= sim_thr && dist <= dist_thr;
        }
    }
    const unsigned long long m = __ballot(edge);
    if (lane == 0) bits[word] = m;
}

// Connected components of the bit matrix, one workgroup, labels in LDS.  lab[i] is always the index of a member of i's
// component and never grows; the fixed point (a round that changes nothing) is lab[i] = the smallest member, whatever order
// the waves ran in.  A round is (1) hook: row i takes the smallest label among its neighbours and hands it to its previous
// root as well (integer atomicMin), (2) compress: every node follows lab[] to a root.  Step (1) alone is min-label
// propagation, which reaches the fixed point within (longest shortest path) <= n - 1 rounds, so the cap of n rounds is never
// what ends the loop; with (2) a chain of 8192 takes a handful of rounds.
__global__ void __launch_bounds__(CF_CC_THREADS) k_segment_components(int n, int W,
                                                                      const unsigned long long* __restrict__ bits,
                                                                      int* __restrict__ labels, int* __restrict__ n_components) {
    extern __shared__ int lab[];       // [n]
    __shared__ int changed, count;
    const int tid = threadIdx.x, lane = tid & (CF_WAVE - 1), wave = tid >> 6;
    constexpr int WAVES = CF_CC_THREADS / CF_WAVE;
    for (int i = tid; i < n; i += CF_CC_THREADS) lab[i] = i;
    if (tid == 0) { changed = 0; count = 0; }
    __syncthreads();
    for (int round = 0; round < n; round++) {
        for (int i = wave; i < n; i += WAVES) {
            int m = n;
            for (int w = lane; w < W; w += CF_WAVE) {
                unsigned long long word = bits[(size_t)i * W + w];
                while (word) {
                    const int bit = __ffsll((long long)word) - 1;
                    word &= word - 1;
                    m = min(m, lab[w * CF_WAVE + bit]);
                }
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) m = min(m, __shfl_xor(m, off, CF_WAVE));
            if (lane == 0) {
                const int old = lab[i];
                if (m < old) {
                    atomicMin(&lab[i], m);
                    atomicMin(&lab[old], m);
                    changed = 1;
                }
            }
        }
        __syncthreads();
        for (int i = tid; i < n; i += CF_CC_THREADS) {
            int l = lab[i];
            for (int hop = 0; hop < n; hop++) {     // labels strictly decrease along the path: at most n hops
                const int up = lab[l];
                if (up == l) break;
                l = up;
            }
            if (l < lab[i]) atomicMin(&lab[i], l);
        }
        __syncthreads();
        const bool again = changed != 0;
        __syncthreads();
        if (!again) break;
        if (tid == 0) changed = 0;
        __syncthreads();
    }
    int roots = 0;
    for (int i = tid; i < n; i += CF_CC_THREADS) {
        const int l = lab[i];
        labels[i] = l;
        roots += l == i;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) roots += __shfl_xor(roots, off, CF_WAVE);
    if (lane == 0) atomicAdd(&count, roots);
    __syncthreads();
    if (tid == 0) *n_components = count;
}

size_t segment_merge_workspace_bytes(int n) {
    const size_t W = ((size_t)std::max(n, 0) + 63) / 64;
    return std::max<size_t>((size_t)std::max(n, 0) * W * sizeof(unsigned long long), 16);
}

void launch_segment_merge_labels(hipStream_t s, int n, const float* seg, double dist_thr, double sim_thr, void* workspace,
                                 int* labels, int* n_components) {
    ProfScope pr("segment_merge_labels", s);
    const int W = (n + 63) / 64;
    const long long words = (long long)n * W;
    const int per = CF_ADJ_THREADS / CF_WAVE;
    unsigned long long* bits = (unsigned long long*)workspace;
    hipLaunchKernelGGL(k_segment_adjacency, dim3((unsigned)((words + per - 1) / per)), dim3(CF_ADJ_THREADS), 0, s, n, W, seg,
                       dist_thr, sim_thr, bits);
    hipLaunchKernelGGL(k_segment_components, dim3(1), dim3(CF_CC_THREADS), (size_t)n * sizeof(int), s, n, W, bits, labels,
                       n_components);
}

// ------------------------------------------------------------------------------------------------ pair consensus fit
// Solves the symmetric positive definite 4 x 4 system G X = R (three right-hand sides) by Gaussian elimination with partial
// pivoting; false when a pivot vanishes.
__device__ bool solve4(double G[4][4], double R[4][3]) {
    for (int c = 0; c < 4; c++) {
        int p = c;
        for (int r = c + 1; r < 4; r++)
            if (fabs(G[r][c]) > fabs(G[p][c])) p = r;
        if (G[p][c] == 0.0) return false;
        if (p != c) {
            for (int k = 0; k < 4; k++) { const double t = G[c][k]; G[c][k] = G[p][k]; G[p][k] = t; }
            for (int k = 0; k < 3; k++) { const double t = R[c][k]; R[c][k] = R[p][k]; R[p][k] = t; }
        }
        for (int r = c + 1; r < 4; r++) {
            const double f = G[r][c] / G[c][c];
            for (int k = c; k < 4; k++) G[r][k] -= f * G[c][k];
            for (int k = 0; k < 3; k++) R[r][k] -= f * R[c][k];
        }
    }
    for (int c = 3; c >= 0; c--)
        for (int k = 0; k < 3; k++) {
            double v = R[c][k];
            for (int j = c + 1; j < 4; j++) v -= G[c][j] * R[j][k];
            R[c][k] = v / G[c][c];
        }
    return true;
}

// (count, residual sum, candidate index): more inliers, then the smaller sum of squared residuals, then the earlier (i, j)
__device__ __forceinline__ bool better(int c1, double r1, int i1, int c2, double r2, int i2) {
    if (c1 != c2) return c1 > c2;
    if (r1 != r2) return r1 < r2;
    return i1 < i2;
}

__global__ void __launch_bounds__(CF_PAIR_THREADS) k_pair_consensus_fit(int K, const float* __restrict__ cp,
                                                                        const int* __restrict__ pairs, int sample_num,
                                                                        double ransac_thr, double err_thr,
                                                                        float* __restrict__ ctrl, double* __restrict__ rmse,
                                                                        int* __restrict__ inliers, uint8_t* __restrict__ ok) {
    __shared__ double px[CF_PAIR_MAX_POINTS], py[CF_PAIR_MAX_POINTS], pz[CF_PAIR_MAX_POINTS];
    __shared__ double key[CF_PAIR_MAX_POINTS];
    __shared__ uint8_t inl[CF_PAIR_MAX_POINTS];
    __shared__ int best_cnt[CF_PAIR_WAVES], best_idx[CF_PAIR_WAVES];
    __shared__ double best_rs[CF_PAIR_WAVES];
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & (CF_WAVE - 1), wave = tid >> 6;
    const int N = 2 * sample_num;
    // ---- the N points: the samples of the first curve, then of the second
    const double inv = 1.0 / (double)(sample_num - 1);
    for (int p = tid; p < N; p += CF_PAIR_THREADS) {
        const int which = p >= sample_num, i = p - which * sample_num;
        const float* c = cp + (size_t)pairs[2 * k + which] * 12;
        double w[4];
        bernstein((double)i * inv, w);
        px[p] = w[0] * (double)c[0] + w[1] * (double)c[3] + w[2] * (double)c[6] + w[3] * (double)c[9];
        py[p] = w[0] * (double)c[1] + w[1] * (double)c[4] + w[2] * (double)c[7] + w[3] * (double)c[10];
        pz[p] = w[0] * (double)c[2] + w[1] * (double)c[5] + w[2] * (double)c[8] + w[3] * (double)c[11];
    }
    __syncthreads();
    // ---- exhaustive consensus: candidate c = (i, j), i < j, in row-major order; a thread visits its candidates in ascending
    // order and replaces its best only on a strict improvement, so the earliest of equals survives
    const int M = N * (N - 1) / 2;
    const double thr2 = ransac_thr * ransac_thr;
    int bc = 0, bi = M;
    double brs = INFINITY;
    for (int c = tid; c < M; c += CF_PAIR_THREADS) {
        // row i starts at candidate i (2N - i - 1) / 2
        int i = (int)(((double)(2 * N - 1) - sqrt((double)(2 * N - 1) * (double)(2 * N - 1) - 8.0 * (double)c)) * 0.5);
        i = max(0, min(i, N - 2));
        while (i > 0 && i * (2 * N - i - 1) / 2 > c) i--;
        while (i < N - 2 && (i + 1) * (2 * N - i - 2) / 2 <= c) i++;
        const int j = i + 1 + (c - i * (2 * N - i - 1) / 2);
        const double ox = px[i], oy = py[i], oz = pz[i];
        double dx = px[j] - ox, dy = py[j] - oy, dz = pz[j] - oz;
        const double nd = sqrt(dx * dx + dy * dy + dz * dz);
        if (!(nd > 0.0)) continue;
        dx /= nd; dy /= nd; dz /= nd;
        int cnt = 0;
        double rs = 0.0;
        for (int p = 0; p < N; p++) {
            const double rx = px[p] - ox, ry = py[p] - oy, rz = pz[p] - oz;
            const double t = rx * dx + ry * dy + rz * dz;
            const double ex = rx - t * dx, ey = ry - t * dy, ez = rz - t * dz;
            const double r2 = ex * ex + ey * ey + ez * ez;
            cnt += r2 < thr2;
            rs += r2;
        }
        if (better(cnt, rs, c, bc, brs, bi)) { bc = cnt; brs = rs; bi = c; }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const int oc = __shfl_xor(bc, off, CF_WAVE), oi = __shfl_xor(bi, off, CF_WAVE);
        const double ors = __shfl_xor(brs, off, CF_WAVE);
        if (better(oc, ors, oi, bc, brs, bi)) { bc = oc; brs = ors; bi = oi; }
    }
    if (lane == 0) { best_cnt[wave] = bc; best_rs[wave] = brs; best_idx[wave] = bi; }
    __syncthreads();
    if (wave != 0) return;            // the rest is one wave's work; no barrier follows
    bc = best_cnt[0]; brs = best_rs[0]; bi = best_idx[0];
    for (int w = 1; w < CF_PAIR_WAVES; w++)
        if (better(best_cnt[w], best_rs[w], best_idx[w], bc, brs, bi)) { bc = best_cnt[w]; brs = best_rs[w]; bi = best_idx[w]; }
    auto fail = [&](int count) {
        for (int q = lane; q < 12; q += CF_WAVE) ctrl[(size_t)k * 12 + q] = 0.f;
        if (lane == 0) { rmse[k] = 0.0; inliers[k] = count; ok[k] = 0; }
    };
    if (bc < 2) { fail(bc); return; }
    constexpr int PER = CF_PAIR_MAX_POINTS / CF_WAVE;
    // ---- the winner's inlier mask; line through the inliers: centroid, principal direction, extent of the projections
    {
        int i = 0;
        while (i < N - 2 && (i + 1) * (2 * N - i - 2) / 2 <= bi) i++;
        const int j = i + 1 + (bi - i * (2 * N - i - 1) / 2);
        const double ox = px[i], oy = py[i], oz = pz[i];
        double dx = px[j] - ox, dy = py[j] - oy, dz = pz[j] - oz;
        const double nd = sqrt(dx * dx + dy * dy + dz * dz);
        dx /= nd; dy /= nd; dz /= nd;
        for (int p = lane; p < N; p += CF_WAVE) {
            const double rx = px[p] - ox, ry = py[p] - oy, rz = pz[p] - oz;
            const double t = rx * dx + ry * dy + rz * dz;
            const double ex = rx - t * dx, ey = ry - t * dy, ez = rz - t * dz;
            inl[p] = (ex * ex + ey * ey + ez * ez) < thr2;
        }
    }
    wave_lds_sync();
    double s[3] = {0, 0, 0};
    for (int q = 0; q < PER; q++) {
        const int p = lane + q * CF_WAVE;
        if (p < N && inl[p]) { s[0] += px[p]; s[1] += py[p]; s[2] += pz[p]; }
    }
    const double cnt = (double)bc;
    const double ctr[3] = {wsum(s[0]) / cnt, wsum(s[1]) / cnt, wsum(s[2]) / cnt};
    double c6[6] = {0, 0, 0, 0, 0, 0};
    for (int q = 0; q < PER; q++) {
        const int p = lane + q * CF_WAVE;
        if (p < N && inl[p]) {
            const double a = px[p] - ctr[0], b = py[p] - ctr[1], c = pz[p] - ctr[2];
            c6[0] += a * a; c6[1] += a * b; c6[2] += a * c; c6[3] += b * b; c6[4] += b * c; c6[5] += c * c;
        }
    }
#pragma unroll
    for (int q = 0; q < 6; q++) c6[q] = wsum(c6[q]);
    double d[3];
    principal_axis(c6[0], c6[1], c6[2], c6[3], c6[4], c6[5], d);
    double tmin = INFINITY, tmax = -INFINITY;
    for (int q = 0; q < PER; q++) {
        const int p = lane + q * CF_WAVE;
        if (p < N && inl[p]) {
            const double t = (px[p] - ctr[0]) * d[0] + (py[p] - ctr[1]) * d[1] + (pz[p] - ctr[2]) * d[2];
            tmin = fmin(tmin, t);
            tmax = fmax(tmax, t);
        }
    }
    tmin = wmin(tmin);
    tmax = wmax(tmax);
    // the line's end points, and from them the direction and the midpoint the points are ordered by (topology.py)
    double st[3], en[3], mainv[3], mid[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        st[c] = ctr[c] + d[c] * tmin;
        en[c] = ctr[c] + d[c] * tmax;
        mainv[c] = en[c] - st[c];
        mid[c] = (en[c] + st[c]) / 2.0;
    }
    const double mn = sqrt(mainv[0] * mainv[0] + mainv[1] * mainv[1] + mainv[2] * mainv[2]);
    if (!(mn > 0.0)) { fail(bc); return; }
#pragma unroll
    for (int c = 0; c < 3; c++) mainv[c] /= mn;
    for (int p = lane; p < N; p += CF_WAVE)
        key[p] = (px[p] - mid[0]) * mainv[0] + (py[p] - mid[1]) * mainv[1] + (pz[p] - mid[2]) * mainv[2];
    wave_lds_sync();
    // ---- stable rank of every point (ties by original index), t = rank / (N - 1); normal equations of the cubic Bezier
    const double invn = 1.0 / (double)(N - 1);
    double g[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, r[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    int rank[PER];
#pragma unroll
    for (int q = 0; q < PER; q++) {
        const int p = lane + q * CF_WAVE;
        rank[q] = 0;
        if (p < N) {
            const double kp = key[p];
            int rk = 0;
            for (int o = 0; o < N; o++) {
                const double ko = key[o];
                rk += (ko < kp) || (ko == kp && o < p);
            }
            rank[q] = rk;
            double w[4];
            bernstein((double)rk * invn, w);
            int e = 0;
#pragma unroll
            for (int a = 0; a < 4; a++) {
#pragma unroll
                for (int b = a; b < 4; b++) g[e++] += w[a] * w[b];
                r[a * 3 + 0] += w[a] * px[p];
                r[a * 3 + 1] += w[a] * py[p];
                r[a * 3 + 2] += w[a] * pz[p];
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 10; q++) g[q] = wsum(g[q]);
#pragma unroll
    for (int q = 0; q < 12; q++) r[q] = wsum(r[q]);
    double G[4][4], R[4][3];
    {
        int e = 0;
        for (int a = 0; a < 4; a++)
            for (int b = a; b < 4; b++) { G[a][b] = G[b][a] = g[e++]; }
        for (int a = 0; a < 4; a++)
            for (int c = 0; c < 3; c++) R[a][c] = r[a * 3 + c];
    }
    if (!solve4(G, R)) { fail(bc); return; }
    double se = 0.0;
#pragma unroll
    for (int q = 0; q < PER; q++) {
        const int p = lane + q * CF_WAVE;
        if (p < N) {
            double w[4];
            bernstein((double)rank[q] * invn, w);
            const double ex = px[p] - (w[0] * R[0][0] + w[1] * R[1][0] + w[2] * R[2][0] + w[3] * R[3][0]);
            const double ey = py[p] - (w[0] * R[0][1] + w[1] * R[1][1] + w[2] * R[2][1] + w[3] * R[3][1]);
            const double ez = pz[p] - (w[0] * R[0][2] + w[1] * R[1][2] + w[2] * R[2][2] + w[3] * R[3][2]);
            se += ex * ex + ey * ey + ez * ez;
        }
    }
    const double e = sqrt(wsum(se) / (double)N);
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < 12; q++) ctrl[(size_t)k * 12 + q] = (float)R[q / 3][q % 3];
        rmse[k] = e;
        inliers[k] = bc;
        ok[k] = e <= err_thr ? 1 : 0;
    }
}

void launch_pair_consensus_fit(hipStream_t s, int K, const float* cp, const int* pairs, int sample_num, double ransac_thr,
                               double err_thr, float* ctrl, double* rmse, int* inliers, uint8_t* ok) {
    ProfScope pr("pair_consensus_fit", s);
    hipLaunchKernelGGL(k_pair_consensus_fit, dim3(K), dim3(CF_PAIR_THREADS), 0, s, K, cp, pairs, sample_num, ransac_thr,
                       err_thr, ctrl, rmse, inliers, ok);
}

}  // namespace cgs
