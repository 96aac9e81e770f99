// The subset of GLM the reference rasterizer uses, written from GLM's documented semantics (OpenGL conventions):
//
//   * mat3 is COLUMN-major: mat3(a0, a1, a2, b0, b1, b2, c0, c1, c2) has columns (a0, a1, a2), (b0, b1, b2), (c0, c1, c2),
//     and m[i] is column i, so m[i][j] is row j of column i.  mat3(s) is s times the identity.
//   * mat * vec treats vec as a column, vec * mat as a row: (M v)_r = sum_k M[k][r] v[k], (v M)_c = dot(v, M[c]).
//   * (A B)[c] = A * B[c]; every sum runs over k = 0, 1, 2 left to right, like GLM's own expansions.
//   * scalar overloads dot(x, y) = x * y and max(x, y) = (x < y) ? y : x.
//
// A row-major slip here would silently turn the oracle into another rasterizer: tests/test_ref_raster_cpu.py checks every
// operator against float64 numpy through the host-only exports of ref_raster_api.cpp.  Test infrastructure only.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define GLM_SHIM_FUNC __host__ __device__ inline
#else
#define GLM_SHIM_FUNC inline
#endif

namespace glm {

struct vec3 {
    float x, y, z;
    GLM_SHIM_FUNC vec3() : x(0.0f), y(0.0f), z(0.0f) {}
    GLM_SHIM_FUNC explicit vec3(float s) : x(s), y(s), z(s) {}
    GLM_SHIM_FUNC vec3(float a, float b, float c) : x(a), y(b), z(c) {}
    GLM_SHIM_FUNC float& operator[](int i) { return i == 0 ? x : (i == 1 ? y : z); }
    GLM_SHIM_FUNC const float& operator[](int i) const { return i == 0 ? x : (i == 1 ? y : z); }
    GLM_SHIM_FUNC vec3& operator+=(const vec3& o) { x += o.x; y += o.y; z += o.z; return *this; }
    GLM_SHIM_FUNC vec3& operator-=(const vec3& o) { x -= o.x; y -= o.y; z -= o.z; return *this; }
    GLM_SHIM_FUNC vec3& operator*=(float s) { x *= s; y *= s; z *= s; return *this; }
};

struct vec4 {
    float x, y, z, w;
    GLM_SHIM_FUNC vec4() : x(0.0f), y(0.0f), z(0.0f), w(0.0f) {}
    GLM_SHIM_FUNC vec4(float a, float b, float c, float d) : x(a), y(b), z(c), w(d) {}
};

// The reference reinterprets float arrays as glm::vec3* / glm::vec4* (scales, rotations, campos, gradients).
static_assert(sizeof(vec3) == 12, "glm::vec3 must be three packed floats");
static_assert(sizeof(vec4) == 16, "glm::vec4 must be four packed floats");

GLM_SHIM_FUNC vec3 operator+(const vec3& a, const vec3& b) { return vec3(a.x + b.x, a.y + b.y, a.z + b.z); }
GLM_SHIM_FUNC vec3 operator-(const vec3& a, const vec3& b) { return vec3(a.x - b.x, a.y - b.y, a.z - b.z); }
GLM_SHIM_FUNC vec3 operator*(const vec3& a, const vec3& b) { return vec3(a.x * b.x, a.y * b.y, a.z * b.z); }
GLM_SHIM_FUNC vec3 operator*(const vec3& v, float s) { return vec3(v.x * s, v.y * s, v.z * s); }
GLM_SHIM_FUNC vec3 operator*(float s, const vec3& v) { return vec3(s * v.x, s * v.y, s * v.z); }
GLM_SHIM_FUNC vec3 operator/(const vec3& v, float s) { return vec3(v.x / s, v.y / s, v.z / s); }

GLM_SHIM_FUNC float dot(float a, float b) { return a * b; }
GLM_SHIM_FUNC float dot(const vec3& a, const vec3& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
GLM_SHIM_FUNC float length(const vec3& v) { return sqrtf(dot(v, v)); }
GLM_SHIM_FUNC float max(float a, float b) { return (a < b) ? b : a; }

struct mat3 {
    vec3 c[3];   // columns
    GLM_SHIM_FUNC mat3() : mat3(1.0f) {}
    GLM_SHIM_FUNC explicit mat3(float s) { c[0] = vec3(s, 0.0f, 0.0f); c[1] = vec3(0.0f, s, 0.0f); c[2] = vec3(0.0f, 0.0f, s); }
    GLM_SHIM_FUNC mat3(float x0, float y0, float z0, float x1, float y1, float z1, float x2, float y2, float z2) {
        c[0] = vec3(x0, y0, z0);
        c[1] = vec3(x1, y1, z1);
        c[2] = vec3(x2, y2, z2);
    }
    GLM_SHIM_FUNC vec3& operator[](int i) { return c[i]; }
    GLM_SHIM_FUNC const vec3& operator[](int i) const { return c[i]; }
};

GLM_SHIM_FUNC vec3 operator*(const mat3& m, const vec3& v) {
    return vec3(m[0][0] * v.x + m[1][0] * v.y + m[2][0] * v.z,
                m[0][1] * v.x + m[1][1] * v.y + m[2][1] * v.z,
                m[0][2] * v.x + m[1][2] * v.y + m[2][2] * v.z);
}

GLM_SHIM_FUNC vec3 operator*(const vec3& v, const mat3& m) {
    return vec3(m[0][0] * v.x + m[0][1] * v.y + m[0][2] * v.z,
                m[1][0] * v.x + m[1][1] * v.y + m[1][2] * v.z,
                m[2][0] * v.x + m[2][1] * v.y + m[2][2] * v.z);
}

GLM_SHIM_FUNC mat3 operator*(const mat3& a, const mat3& b) {
    mat3 r;
    for (int i = 0; i < 3; ++i) r[i] = a * b[i];
    return r;
}

GLM_SHIM_FUNC mat3 operator*(float s, const mat3& m) {
    mat3 r;
    for (int i = 0; i < 3; ++i) r[i] = s * m[i];
    return r;
}

GLM_SHIM_FUNC mat3 operator*(const mat3& m, float s) {
    mat3 r;
    for (int i = 0; i < 3; ++i) r[i] = m[i] * s;
    return r;
}

GLM_SHIM_FUNC mat3 transpose(const mat3& m) {
    return mat3(m[0][0], m[1][0], m[2][0],
                m[0][1], m[1][1], m[2][1],
                m[0][2], m[1][2], m[2][2]);
}

}  // namespace glm
