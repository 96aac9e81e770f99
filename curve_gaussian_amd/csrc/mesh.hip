// Ellipsoid mesh of the splats, written as the binary body of a PLY file: the reference's GaussianCurveModel.draw_ellipsoids
// (scene/gaussian_curve_model.py:634-709) builds one Open3D sphere per splat in a Python loop, scales, rotates and moves it,
// paints it one colour and concatenates the meshes.  Here every splat's copy of a host-made sphere template is expanded
// directly into the bytes of Open3D's binary little-endian PLY records:
//
//   vertex record, 27 B: double x, y, z; uchar red, green, blue
//   face record,   13 B: uchar 3; int a, b, c
//
// Arithmetic (exact; a float64 numpy restatement matches bit for bit): template vertex (tx, ty, tz), float64, radius
// applied on the host; p_k = t_k * (double)s_k; R = Eigen's Quaternion::toRotationMatrix of (double)(w, x, y, z) as given;
// every row ((r0*p0 + r1*p1) + r2*p2) + (double)xyz_k.  Contraction into FMAs is off.  Colour: Open3D's ColorToUint8,
// uint8(round(min(1, max(0, (double)c)) * 255)), round half away from zero.  Face indices: template + (first + i) * V0.
//
// Stores: a workgroup expands 256 consecutive records into LDS (byte writes at 27 t or 13 t), then stores its span of the
// chunk as aligned 16-byte words (256 records = 432 vertex words or 208 face words, so every workgroup starts on a word).
// Every word of the chunk, the zero-padded last one included, is written once by one non-temporal dwordx4 store: the
// output is far larger than L2 and is never read back on the device.  Byte offsets inside the chunk are 64-bit.  The
// bytes of a record depend only on its splat and template entry, so every chunking gives the same file.
#include "kernels.h"

namespace cgs {

constexpr int MESH_BLOCK = 256;                    // records per workgroup, one per thread
constexpr int MESH_VTX_BYTES = 27;
constexpr int MESH_FACE_BYTES = 13;
constexpr int MESH_VTX_WORDS = MESH_BLOCK * MESH_VTX_BYTES / 16;    // 432
constexpr int MESH_FACE_WORDS = MESH_BLOCK * MESH_FACE_BYTES / 16;  // 208
static_assert(MESH_BLOCK * MESH_VTX_BYTES % 16 == 0 && MESH_BLOCK * MESH_FACE_BYTES % 16 == 0, "word-aligned workgroups");

typedef unsigned int mesh_u32x4 __attribute__((ext_vector_type(4)));

__device__ inline void mesh_put_bytes(unsigned char* dst, const void* src, int n) {
    const unsigned char* s = (const unsigned char*)src;
    for (int b = 0; b < n; b++) dst[b] = s[b];
}

__device__ inline unsigned char mesh_color_u8(float c) {
    // std::round(std::min(1., std::max(0., c)) * 255.): std::max(0., NaN) is 0
    double x = (double)c;
    x = (0.0 < x) ? x : 0.0;
    x = (x < 1.0) ? x : 1.0;
    return (unsigned char)round(x * 255.0);
}

// Store the workgroup's nwords staged words; called after the records were written and a barrier.
__device__ inline void mesh_store_words(const mesh_u32x4* __restrict__ lds, mesh_u32x4* __restrict__ out, size_t word0,
                                        int nwords) {
    for (int w = threadIdx.x; w < nwords; w += MESH_BLOCK) __builtin_nontemporal_store(lds[w], out + word0 + w);
}

// The last workgroup: zero its staged dwords from the one holding byte `valid_bytes` on, so the padding of the last word
// is zero.  Called before the records are written.
__device__ inline void mesh_zero_tail(unsigned int* lds32, int valid_bytes, int nwords) {
    for (int d = valid_bytes / 4 + threadIdx.x; d < nwords * 4; d += MESH_BLOCK) lds32[d] = 0u;
}

__global__ void __launch_bounds__(MESH_BLOCK) k_mesh_vertices(long long n, int first, const float* __restrict__ xyz,
                                                              const float* __restrict__ rot, const float* __restrict__ scale,
                                                              const float* __restrict__ rgb, int V0,
                                                              const double* __restrict__ tv, mesh_u32x4* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ mesh_u32x4 stage[MESH_VTX_WORDS];
    unsigned char* bytes = (unsigned char*)stage;
    const long long r0 = (long long)blockIdx.x * MESH_BLOCK;
    const int nrec = (int)min((long long)MESH_BLOCK, n - r0);
    const int nwords = (int)((nrec * MESH_VTX_BYTES + 15) / 16);
    if (nrec < MESH_BLOCK) {
        mesh_zero_tail((unsigned int*)stage, nrec * MESH_VTX_BYTES, nwords);
        __syncthreads();
    }
    const int t = threadIdx.x;
    if (t < nrec) {
        const long long r = r0 + t;
        const long long i = (long long)first + r / V0;
        const int k = (int)(r % V0);
        const double p0 = tv[3 * k + 0] * (double)scale[3 * i + 0];
        const double p1 = tv[3 * k + 1] * (double)scale[3 * i + 1];
        const double p2 = tv[3 * k + 2] * (double)scale[3 * i + 2];
        const double w = (double)rot[4 * i + 0], x = (double)rot[4 * i + 1], y = (double)rot[4 * i + 2],
                     z = (double)rot[4 * i + 3];
        // Eigen::QuaternionBase::toRotationMatrix
        const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
        const double twx = tx * w, twy = ty * w, twz = tz * w;
        const double txx = tx * x, txy = ty * x, txz = tz * x;
        const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
        const double m00 = 1.0 - (tyy + tzz), m01 = txy - twz, m02 = txz + twy;
        const double m10 = txy + twz, m11 = 1.0 - (txx + tzz), m12 = tyz - twx;
        const double m20 = txz - twy, m21 = tyz + twx, m22 = 1.0 - (txx + tyy);
        double v[3];
        v[0] = ((m00 * p0 + m01 * p1) + m02 * p2) + (double)xyz[3 * i + 0];
        v[1] = ((m10 * p0 + m11 * p1) + m12 * p2) + (double)xyz[3 * i + 1];
        v[2] = ((m20 * p0 + m21 * p1) + m22 * p2) + (double)xyz[3 * i + 2];
        unsigned char c[3];
        for (int j = 0; j < 3; j++) c[j] = mesh_color_u8(rgb[3 * i + j]);
        unsigned char* dst = bytes + MESH_VTX_BYTES * t;
        mesh_put_bytes(dst, v, 24);
        mesh_put_bytes(dst + 24, c, 3);
    }
    __syncthreads();
    mesh_store_words(stage, out, (size_t)blockIdx.x * MESH_VTX_WORDS, nwords);
}

__global__ void __launch_bounds__(MESH_BLOCK) k_mesh_faces(long long n, int first, int V0, int F0,
                                                           const int* __restrict__ tf, mesh_u32x4* __restrict__ out) {
    __shared__ mesh_u32x4 stage[MESH_FACE_WORDS];
    unsigned char* bytes = (unsigned char*)stage;
    const long long r0 = (long long)blockIdx.x * MESH_BLOCK;
    const int nrec = (int)min((long long)MESH_BLOCK, n - r0);
    const int nwords = (int)((nrec * MESH_FACE_BYTES + 15) / 16);
    if (nrec < MESH_BLOCK) {
        mesh_zero_tail((unsigned int*)stage, nrec * MESH_FACE_BYTES, nwords);
        __syncthreads();
    }
    const int t = threadIdx.x;
    if (t < nrec) {
        const long long r = r0 + t;
        const int base = (int)(((long long)first + r / F0) * V0);   // the host checked (first + count) * V0 <= 2^31
        const int k = (int)(r % F0);
        const int f[3] = {tf[3 * k + 0] + base, tf[3 * k + 1] + base, tf[3 * k + 2] + base};
        unsigned char* dst = bytes + MESH_FACE_BYTES * t;
        dst[0] = 3;
        mesh_put_bytes(dst + 1, f, 12);
    }
    __syncthreads();
    mesh_store_words(stage, out, (size_t)blockIdx.x * MESH_FACE_WORDS, nwords);
}

void launch_ellipsoid_vertices(hipStream_t s, int first, int count, const float* xyz, const float* rot, const float* scale,
                               const float* rgb, int V0, const double* template_vertices, void* out) {
    const long long n = (long long)count * V0;
    if (n <= 0) return;
    const unsigned int blocks = (unsigned int)((n + MESH_BLOCK - 1) / MESH_BLOCK);
    hipLaunchKernelGGL(k_mesh_vertices, dim3(blocks), dim3(MESH_BLOCK), 0, s, n, first, xyz, rot, scale, rgb, V0,
                       template_vertices, (mesh_u32x4*)out);
}

void launch_ellipsoid_faces(hipStream_t s, int first, int count, int V0, int F0, const int* template_faces, void* out) {
    const long long n = (long long)count * F0;
    if (n <= 0) return;
    const unsigned int blocks = (unsigned int)((n + MESH_BLOCK - 1) / MESH_BLOCK);
    hipLaunchKernelGGL(k_mesh_faces, dim3(blocks), dim3(MESH_BLOCK), 0, s, n, first, V0, F0, template_faces,
                       (mesh_u32x4*)out);
}

}  // namespace cgs
