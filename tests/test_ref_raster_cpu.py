"""The reference-rasterizer oracle without a GPU: the artefact oracle.build() makes, and the GLM subset it is compiled against.

oracle/_ref/libref_raster.so is the reference's own cuda_rasterizer/ built for gfx950 against our shims
(oracle/ref_raster/).  GLM is the one shim with arithmetic in it: a row-major slip (or a wrong summation order) there would
turn the "reference" into another rasterizer while every GPU comparison against it still ran.  So every GLM operator the
reference uses is run here through the library's host-only exports and checked against float64 numpy, on inputs whose
products and sums are exact in float32 (small integers): the results must be equal, not close."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle

F = C.POINTER(C.c_float)


@pytest.fixture(scope="module")
def L():
    """The GLM shim's host-only checks, built from our sources alone: present on every machine with hipcc."""
    so = oracle.build_ref_raster()
    import oracle.ref_raster as R   # (imports torch first: one HIP runtime per process)
    G = R.glm_check_lib()
    if so is not None:   # the library the reference was compiled into carries the same exports
        assert all(hasattr(R.lib(), n) for n in GLM_EXPORTS)
    return G


GLM_EXPORTS = ("ref_glm_construct", "ref_glm_transpose", "ref_glm_mat_vec", "ref_glm_mat_mat", "ref_glm_cov2d_shape",
               "ref_glm_vec_ops")


def _built_reference():
    """oracle/_ref/libref_raster.so after oracle.build(); None only where no reference checkout is readable and no build
    of it arrived (the GPU suite's reference pins then fail with a clear message -- the pin needs the checkout once)."""
    so = oracle.build_ref_raster()
    if so is None:
        assert oracle.ref_raster_src() is None, "a readable reference checkout must be built"
        pytest.skip("no reference checkout readable on this machine (REF_RASTER_SRC) and no oracle/_ref/libref_raster.so")
    return so


def _p(a):
    return a.ctypes.data_as(F)


def _f32(a):
    return np.ascontiguousarray(np.asarray(a, np.float32))


def _glm_mat(cols):
    """numpy [3,3] matrix whose COLUMN i is cols[i] -- GLM's m[i] (mat3(9 scalars) fills column by column)."""
    return np.asarray(cols, np.float64).reshape(3, 3).T


def _as_glm(M):
    """numpy matrix -> the 9 numbers in GLM's m[i][j] order (column i, row j)."""
    return _f32(np.asarray(M).T.reshape(9))


RNG = np.random.default_rng(5)


def _ints(*shape, lo=-6, hi=7):
    return RNG.integers(lo, hi, size=shape).astype(np.float64)


def test_the_artefact_exists_after_build_and_exports_the_wrapper_abi():
    so = _built_reference()
    assert os.path.exists(so) and so == oracle.REF_RASTER_SO
    import oracle.ref_raster as R
    L = R.lib()
    for name in ("ref_forward", "ref_backward", "ref_mark_visible", "ref_num_rendered", "ref_copy_state", "ref_free",
                 "ref_last_error") + GLM_EXPORTS:
        assert hasattr(L, name), name
    # ... and the reference's own entry points are linked into the same library (CudaRasterizer::Rasterizer::*)
    for mangled in ("_ZN14CudaRasterizer10Rasterizer7forwardE", "_ZN14CudaRasterizer10Rasterizer8backwardE",
                    "_ZN14CudaRasterizer10Rasterizer11markVisibleE"):
        assert mangled.encode() in open(so, "rb").read(), mangled
    L.ref_num_channels.restype = C.c_int
    L.ref_num_all_map.restype = C.c_int
    assert L.ref_num_channels() == 1 and L.ref_num_all_map() == 4   # the reference's config.h


def test_a_second_build_is_a_no_op():
    so = _built_reference()
    t, tg = os.path.getmtime(so), os.path.getmtime(oracle.GLM_CHECK_SO)
    assert oracle.build_ref_raster() == so and os.path.getmtime(so) == t and os.path.getmtime(oracle.GLM_CHECK_SO) == tg


def test_the_glm_check_library_needs_no_reference_source(tmp_path, monkeypatch):
    """Where no reference checkout is readable, oracle.build() still builds the GLM checks and raises nothing."""
    monkeypatch.setenv("REF_RASTER_SRC", str(tmp_path / "absent"))
    assert oracle.ref_raster_src() is None
    so = oracle.build_ref_raster()
    assert os.path.exists(oracle.GLM_CHECK_SO)
    assert so is None or so == oracle.REF_RASTER_SO


def test_glm_mat3_is_column_major_and_mat3_of_s_is_the_identity(L):
    nine = _f32(np.arange(1, 10))
    m, diag = np.zeros(9, np.float32), np.zeros(9, np.float32)
    L.ref_glm_construct(_p(nine), C.c_float(2.5), _p(m), _p(diag))
    # mat3(1..9): column 0 = (1, 2, 3), so m[0][1] (column 0, row 1) = 2 and m[1][0] (column 1, row 0) = 4
    np.testing.assert_array_equal(m, nine)
    assert m[0 * 3 + 1] == 2.0 and m[1 * 3 + 0] == 4.0
    np.testing.assert_array_equal(diag.reshape(3, 3), 2.5 * np.eye(3))


def test_glm_transpose(L):
    for _ in range(4):
        A = _ints(3, 3)
        out = np.zeros(9, np.float32)
        L.ref_glm_transpose(_p(_as_glm(A)), _p(out))
        np.testing.assert_array_equal(out, _as_glm(A.T))


def test_glm_mat_times_vec_and_vec_times_mat(L):
    differ = 0
    for _ in range(6):
        A, v = _ints(3, 3), _ints(3)
        mv, vm = np.zeros(3, np.float32), np.zeros(3, np.float32)
        L.ref_glm_mat_vec(_p(_as_glm(A)), _p(_f32(v)), _p(mv), _p(vm))
        np.testing.assert_array_equal(mv, A @ v)      # column vector
        np.testing.assert_array_equal(vm, v @ A)      # row vector = transpose(A) * v
        differ += not np.array_equal(mv, vm)
    assert differ, "the cases must tell mat * vec from vec * mat"


def test_glm_mat_times_mat_and_scalar_times_mat(L):
    for _ in range(6):
        A, B = _ints(3, 3), _ints(3, 3)
        ab, sa = np.zeros(9, np.float32), np.zeros(9, np.float32)
        L.ref_glm_mat_mat(_p(_as_glm(A)), _p(_as_glm(B)), C.c_float(2.0), _p(ab), _p(sa))
        np.testing.assert_array_equal(ab, _as_glm(A @ B))
        np.testing.assert_array_equal(sa, _as_glm(2.0 * A))


def test_glm_cov2d_shape_transpose_T_transpose_Vrk_T(L):
    """computeCov2D (forward.cu / backward.cu): T = W * J, cov = transpose(T) * transpose(Vrk) * T.  Built the way the
    reference builds them -- W from a row-major view matrix's upper 3x3 passed row by row, so GLM sees its transpose, and a
    J whose third column is zero -- and compared with the float64 product of the same column-major reading."""
    for _ in range(6):
        view = _ints(4, 4)                   # viewmatrix[] as the reference indexes it (column-major 4x4 in memory)
        vm = view.reshape(-1)
        Wm = _glm_mat([vm[0], vm[4], vm[8], vm[1], vm[5], vm[9], vm[2], vm[6], vm[10]])
        fx, fy, a, b = _ints(4, lo=1, hi=5)
        J = _glm_mat([fx, 0.0, -a, 0.0, fy, -b, 0.0, 0.0, 0.0])
        c = _ints(6, lo=-3, hi=4)
        Vrk = _glm_mat([c[0], c[1], c[2], c[1], c[3], c[4], c[2], c[4], c[5]])
        T = Wm @ J
        out = np.zeros(9, np.float32)
        L.ref_glm_cov2d_shape(_p(_as_glm(T)), _p(_as_glm(Vrk)), _p(out))
        want = T.T @ Vrk.T @ T
        assert np.abs(want).max() < 2 ** 24      # every partial sum exact in float32
        np.testing.assert_array_equal(out, _as_glm(want))
        # the three numbers computeCov2D returns: cov[0][0], cov[0][1], cov[1][1]
        assert (out[0], out[1], out[4]) == (want[0, 0], want[1, 0], want[1, 1])


def test_glm_vec3_arithmetic_and_scalar_overloads(L):
    for a, b, s in [((1, 2, 3), (4, -5, 6), 2.0), ((-3, 0, 4), (2, 2, -1), 4.0), ((0, 0, 0), (1, 1, 1), 0.5)]:
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        out = np.zeros(23, np.float32)
        L.ref_glm_vec_ops(_p(_f32(a)), _p(_f32(b)), C.c_float(s), _p(out))
        want = np.concatenate([a + b, a - b, s * a, a / s, a + b, a * s,
                               [a @ b, np.sqrt(a @ a), a[0] * b[0], max(a[0], b[0]), max(a[0], b[0])]])
        np.testing.assert_array_equal(out[:18], want[:18].astype(np.float32))
        assert out[18] == want[18] and out[20] == want[20] and out[21] == want[21] == out[22]
        assert out[19] == np.float32(np.sqrt(np.float32(a @ a)))   # length = correctly rounded sqrt(dot)
