// Host-only exports that run the GLM shim's operators (shim/glm/glm.hpp) on caller-given arrays, for
// tests/test_ref_raster_cpu.py.  Needs no reference source: built on its own into oracle/_ref/libglm_check.so (so the shim
// is checked on every machine that has hipcc) and linked into libref_raster.so (the same object the reference was built
// with).  Test infrastructure only.
#include <glm/glm.hpp>

extern "C" {

// Matrices cross the ABI as m[i][j] in row i*3+j, i.e. column i, row j -- exactly GLM's indexing.
static void store(const glm::mat3& m, float* out) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) out[3 * i + j] = m[i][j];
}

static glm::mat3 load(const float* a) { return glm::mat3(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8]); }

// mat3(9 scalars) then m[i][j]; mat3(s) then m[i][j]
void ref_glm_construct(const float* nine, float s, float* out_m, float* out_diag) {
    store(load(nine), out_m);
    store(glm::mat3(s), out_diag);
}

void ref_glm_transpose(const float* a, float* out) { store(glm::transpose(load(a)), out); }

void ref_glm_mat_vec(const float* a, const float* v, float* out_mv, float* out_vm) {
    const glm::vec3 x(v[0], v[1], v[2]);
    const glm::vec3 mv = load(a) * x, vm = x * load(a);
    for (int i = 0; i < 3; ++i) {
        out_mv[i] = mv[i];
        out_vm[i] = vm[i];
    }
}

void ref_glm_mat_mat(const float* a, const float* b, float s, float* out_ab, float* out_sa) {
    store(load(a) * load(b), out_ab);
    store(s * load(a), out_sa);
}

// computeCov2D's shape: transpose(T) * transpose(Vrk) * T
void ref_glm_cov2d_shape(const float* t, const float* vrk, float* out) {
    const glm::mat3 T = load(t), V = load(vrk);
    store(glm::transpose(T) * glm::transpose(V) * T, out);
}

// vec3 arithmetic (+, -, *, scalar * vec, vec / scalar, +=, *= scalar, dot, length) and the scalar dot / max overloads
void ref_glm_vec_ops(const float* a, const float* b, float s, float* out) {
    const glm::vec3 x(a[0], a[1], a[2]), y(b[0], b[1], b[2]);
    glm::vec3 acc = x;
    acc += y;
    glm::vec3 sc = x;
    sc *= s;
    const glm::vec3 r[6] = {x + y, x - y, s * x, x / s, acc, sc};
    for (int k = 0; k < 6; ++k)
        for (int i = 0; i < 3; ++i) out[3 * k + i] = r[k][i];
    out[18] = glm::dot(x, y);
    out[19] = glm::length(x);
    out[20] = glm::dot(a[0], b[0]);
    out[21] = glm::max(a[0], b[0]);
    out[22] = glm::max(b[0], a[0]);
}

}  // extern "C"
