"""CPU: the host back end of ops.undistort (the float64 restatement of COLMAP's camera models the kernel is held against),
``distortion_of``, and ``read_colmap(undistort=True)``."""
import os

import numpy as np
import pytest
import torch

import undistort_cases as UC
from curve_gaussian_amd.ops import undistort as U
from curve_gaussian_amd.scene import colmap_io as CIO


def test_hand_computed_pixel():
    """One OPENCV camera, one output pixel, every number a dyadic fraction, so the float64 arithmetic is exact.

    W = 8, H = 6, fx = fy = out_fx = out_fy = 4, cx = 4.5, cy = 2.75, k1 = 0.5, k2 = 0, p1 = 0.25, p2 = 0.125; pixel (i, j) = (5, 4):
      x  = (5 + 0.5 - 4) / 4 = 0.375          y = (4 + 0.5 - 3) / 4 = 0.375          r2 = 0.28125
      s  = 1 + 0.5 * 0.28125 = 1.140625       x s = y s = 0.427734375
      xd = 0.427734375 + 2 * 0.25 * 0.140625 + 0.125 * (0.28125 + 0.28125) = 0.427734375 + 0.0703125 + 0.0703125 = 0.568359375
      yd = 0.427734375 + 0.25 * (0.28125 + 0.28125) + 2 * 0.125 * 0.140625 = 0.427734375 + 0.140625 + 0.03515625 = 0.603515625
      u  = 4 * 0.568359375 + 4.5 - 0.5 = 6.2734375       x0 = 6, a = 0.2734375 = 35/128
      v  = 4 * 0.603515625 + 2.75 - 0.5 = 4.6640625      y0 = 4, b = 0.6640625 = 85/128
      weights of the taps (6,4), (7,4), (6,5), (7,5):  (93 * 43, 35 * 43, 93 * 85, 35 * 85) / 16384
                                                    = (3999, 1505, 7905, 2975) / 16384, which add up to 1."""
    W, H = 8, 6
    rng = np.random.default_rng(3)
    img = rng.random((2, H, W)).astype(np.float32)
    out, blank = U.undistort_host_f64(img, 4, (4.0, 4.0, 4.5, 2.75), (0.5, 0.0, 0.25, 0.125), (4.0, 4.0), fill=0.0)
    u, v = U.source_positions(H, W, 4, (4.0, 4.0, 4.5, 2.75), (0.5, 0.0, 0.25, 0.125), (4.0, 4.0))
    assert u[4, 5] == 6.2734375 and v[4, 5] == 4.6640625
    src = img.astype(np.float64)
    want = (3999 * src[:, 4, 6] + 1505 * src[:, 4, 7] + 7905 * src[:, 5, 6] + 2975 * src[:, 5, 7]) / 16384
    assert out.dtype == np.float64
    assert np.abs(out[:, 4, 5] - want).max() <= 1e-12
    # and the public entry rounds that value to float32 once
    outs, counts = U.undistort_images([torch.from_numpy(img)], [4], [(4.0, 4.0, 4.5, 2.75)], [(0.5, 0.0, 0.25, 0.125)],
                                      [(4.0, 4.0)], backend="host")
    assert outs[0].dtype == torch.float32 and np.array_equal(outs[0].numpy(), out.astype(np.float32))
    assert int(counts[0]) == blank


# ------------------------------------------------------------------------------------------------ direction
def _forward_model(x, y, k1, k2, p1, p2):
    """OPENCV's distortion and its derivatives (SIMPLE_RADIAL is k2 = p1 = p2 = 0), written for this test:
    (D, J, Hess) with D [2,...], J[m][n] = dD_m/dq_n and Hess[m][n][l] = d2 D_m / dq_n dq_l, q = (x, y)."""
    r2 = x * x + y * y
    s, s1, s2 = 1 + k1 * r2 + k2 * r2 * r2, k1 + 2 * k2 * r2, 2 * k2      # s, ds/dr2, d2s/dr2^2
    sx, sy = 2 * x * s1, 2 * y * s1
    sxx, syy, sxy = 2 * s1 + 4 * x * x * s2, 2 * s1 + 4 * y * y * s2, 4 * x * y * s2
    D = (x * s + 2 * p1 * x * y + p2 * (r2 + 2 * x * x), y * s + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y)
    J = ((s + x * sx + 2 * p1 * y + 6 * p2 * x, x * sy + 2 * p1 * x + 2 * p2 * y),
         (y * sx + 2 * p1 * x + 2 * p2 * y, s + y * sy + 6 * p1 * y + 2 * p2 * x))
    d1xx, d1xy, d1yy = 2 * sx + x * sxx + 6 * p2, sy + x * sxy + 2 * p1, x * syy + 2 * p2
    d2xx, d2xy, d2yy = y * sxx + 2 * p1, sx + y * sxy + 2 * p2, 2 * sy + y * syy + 6 * p1
    Hess = (((d1xx, d1xy), (d1xy, d1yy)), ((d2xx, d2xy), (d2xy, d2yy)))
    return D, J, Hess


def _invert(xd, yd, coef, iterations=30):
    """The ideal ray (x, y) with D(x, y) = (xd, yd): Newton iterations in float64 from (xd, yd)."""
    x, y = xd.copy(), yd.copy()
    for _ in range(iterations):
        D, J, _ = _forward_model(x, y, *coef)
        e0, e1 = D[0] - xd, D[1] - yd
        det = J[0][0] * J[1][1] - J[0][1] * J[1][0]
        x, y = x - (J[1][1] * e0 - J[0][1] * e1) / det, y - (J[0][0] * e1 - J[1][0] * e0) / det
    D, _, _ = _forward_model(x, y, *coef)
    assert max(np.abs(D[0] - xd).max(), np.abs(D[1] - yd).max()) < 1e-14
    return x, y


DIRECTION_A, DIRECTION_B = 3.0, 2.0
DIRECTION_CASES = {
    # model id: (its coefficients, the same as OPENCV's (k1, k2, p1, p2), (fx, fy, cx, cy)); H = 37, W = 53
    "SIMPLE_RADIAL": (2, (-0.15,), (-0.15, 0.0, 0.0, 0.0), (41.0, 41.0, 26.5, 18.5)),
    "OPENCV": (4, (-0.1, 0.02, 0.01, -0.015), (-0.1, 0.02, 0.01, -0.015), (41.0, 43.5, 27.8, 17.7)),
}


def _interpolation_bound(H, W, coef, fx, fy, cx, cy, a, b):
    """(1/8) (max |d2h/du2| + max |d2h/dv2|) for the source image h(u, v) = g(phi(u, v)), phi = D^-1((u + 0.5 - cx) / fx,
    (v + 0.5 - cy) / fy), over the source's pixel grid [0, W-1] x [0, H-1] sampled four times per pixel.
    With J = dD/dq at q = phi: dphi/du = J^-1 e1 / fx =: t, d2phi/du2 = -J^-1 Hess[t, t] =: c (differentiate D(phi) = affine
    twice), and d2h/du2 = t^T Hg t + grad g . c.  g = 0.5 + 0.5 sin(a x) cos(b y) has |g_x| <= a/2, |g_y| <= b/2,
    |g_xx| <= a^2/2, |g_xy| <= a b/2, |g_yy| <= b^2/2, hence |d2h/du2| <= (a |t_x| + b |t_y|)^2 / 2 + (a |c_x| + b |c_y|) / 2,
    whatever the phase; the same along v with e2 / fy."""
    us, vs = np.meshgrid(np.linspace(0, W - 1, 4 * (W - 1) + 1), np.linspace(0, H - 1, 4 * (H - 1) + 1))
    x, y = _invert((us + 0.5 - cx) / fx, (vs + 0.5 - cy) / fy, coef)
    _, J, Hs = _forward_model(x, y, *coef)
    det = J[0][0] * J[1][1] - J[0][1] * J[1][0]
    inv = ((J[1][1] / det, -J[0][1] / det), (-J[1][0] / det, J[0][0] / det))
    total = 0.0
    for axis, f in ((0, fx), (1, fy)):
        t = (inv[0][axis] / f, inv[1][axis] / f)
        q = [sum(Hs[m][n][l] * t[n] * t[l] for n in range(2) for l in range(2)) for m in range(2)]
        c = (-(inv[0][0] * q[0] + inv[0][1] * q[1]), -(inv[1][0] * q[0] + inv[1][1] * q[1]))
        second = 0.5 * (a * np.abs(t[0]) + b * np.abs(t[1])) ** 2 + 0.5 * (a * np.abs(c[0]) + b * np.abs(c[1]))
        total += float(second.max())
    return total / 8.0


@pytest.mark.parametrize("name", sorted(DIRECTION_CASES))
def test_direction(name):
    """The source image is the smooth pattern g(x, y) = 0.5 + 0.5 sin(3 x) cos(2 y) of the IDEAL ray of every source pixel
    (the model inverted by Newton iterations here); undistorting it must give g on the ideal pixel grid wherever all four
    taps are inside the source.

    Tolerance: the bilinear interpolation bound of the source image, (max |h_uu| + max |h_vv|) / 8, derived from a = 3,
    b = 2, the focal lengths and the Jacobian and Hessian of the distortion over the image (_interpolation_bound: 1.5e-3
    for SIMPLE_RADIAL, 9.4e-4 for OPENCV; the host back end is at 6.4e-4 and 6.1e-4).
    Applying the model in the wrong direction fails: with ops.undistort._distort replaced by its inverse (this file's
    _invert) the largest difference was 0.97 (SIMPLE_RADIAL) and 0.99 (OPENCV) -- checked once by hand."""
    model, params, coef, (fx, fy, cx, cy) = DIRECTION_CASES[name]
    H, W, a, b = 37, 53, DIRECTION_A, DIRECTION_B
    g = lambda x, y: 0.5 + 0.5 * np.sin(a * x) * np.cos(b * y)
    us, vs = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    sx, sy = _invert((us + 0.5 - cx) / fx, (vs + 0.5 - cy) / fy, coef)
    source = g(sx, sy).astype(np.float32)[None]
    outs, _ = U.undistort_images([torch.from_numpy(source)], [model], [(fx, fy, cx, cy)], [params], [(fx, fy)], backend="host")
    # the ideal grid, and where its pixels land in the source (this test's own forward model)
    x, y = (us + 0.5 - W / 2.0) / fx, (vs + 0.5 - H / 2.0) / fy
    D, _, _ = _forward_model(x, y, *coef)
    u, v = fx * D[0] + cx - 0.5, fy * D[1] + cy - 0.5
    inside = (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)
    assert inside.mean() > 0.8                                  # most of the frame is compared
    bound = _interpolation_bound(H, W, coef, fx, fy, cx, cy, a, b)
    assert 1e-4 < bound < 5e-3                                  # (a bound, not a blank cheque)
    err = np.abs(outs[0].numpy()[0].astype(np.float64) - g(x, y))[inside].max()
    print(f"{name}: max error {err:.3e}, bound {bound:.3e}")
    assert err <= bound


# ------------------------------------------------------------------------------------------------ identity and shift
@pytest.mark.parametrize("model", [0, 1])
def test_identity_and_pure_shift(model):
    """A pinhole camera with a centred principal point copies the image bit for bit.  A principal point off by (+3, -2)
    pixels samples the source 3 columns to the right and 2 rows up: out[j, i] = in[j - 2, i + 3], `fill` where that is
    outside, and exactly those pixels are blank.  (Focal length 64: a power of two keeps (p / f) * f exact.)"""
    H, W, f, fill = 37, 53, 64.0, 0.25
    img = torch.rand(2, H, W, generator=torch.Generator().manual_seed(1))
    outs, counts = U.undistort_images([img], [model], [(f, f, W / 2.0, H / 2.0)], [()], [(f, f)], fill=fill, backend="host")
    assert torch.equal(outs[0], img) and int(counts[0]) == 0
    outs, counts = U.undistort_images([img], [model], [(f, f, W / 2.0 + 3, H / 2.0 - 2)], [()], [(f, f)], fill=fill,
                                      backend="host")
    want = torch.full_like(img, fill)
    want[:, 2:, :W - 3] = img[:, :H - 2, 3:]
    assert torch.equal(outs[0], want)
    assert int(counts[0]) == H * W - (H - 2) * (W - 3)


def test_backend_and_argument_checks():
    img = torch.zeros(1, 4, 4)
    with pytest.raises(ValueError, match="unknown undistort backend 'cpu'"):
        U.undistort_images([img], [1], [(4.0, 4.0, 2.0, 2.0)], [()], [(4.0, 4.0)], backend="cpu")
    with pytest.raises(ValueError, match="1 images but 2 models"):
        U.undistort_images([img], [1, 1], [(4.0, 4.0, 2.0, 2.0)], [()], [(4.0, 4.0)], backend="host")
    with pytest.raises(ValueError, match="1..4 channels"):
        U.undistort_images([torch.zeros(5, 4, 4)], [1], [(4.0, 4.0, 2.0, 2.0)], [()], [(4.0, 4.0)], backend="host")
    with pytest.raises(ValueError, match="model id 5"):
        U.undistort_images([img], [5], [(4.0, 4.0, 2.0, 2.0)], [()], [(4.0, 4.0)], backend="host")


def test_c_abi_rejects_bad_calls_without_a_gpu():
    """The argument checks of cgs_undistort_images come before any device work, so they can be exercised here."""
    import ctypes as C
    from curve_gaussian_amd import _lib as L
    lib = L.load()
    assert C.sizeof(L.UndistortView) == 144

    def call(n, **kw):
        a = dict(src=16, dst=32, channels=1, model=4, fx=8.0, out_fx=8.0)
        a.update(kw)
        table = (L.UndistortView * 1)(L.UndistortView(a["src"], a["dst"], a["channels"], 8, 8, a["model"], a["fx"], 8.0, 4.0, 4.0,
                                                      a["out_fx"], 8.0, (C.c_double * 8)(0.1)))
        return lib.cgs_undistort_images(n, C.cast(table, C.c_void_p), 0.0, C.c_void_p(64), None)

    assert call(0) == 0
    for kw, word in ((dict(model=5), "camera model id 5"), (dict(fx=0.0), "fx=0"), (dict(out_fx=-1.0), "out_fx=-1"),
                     (dict(channels=5), "channels=5"), (dict(dst=16), "dst == src"), (dict(src=None), "NULL")):
        assert call(1, **kw) == -1 and word in L.last_error(), (kw, L.last_error())
    assert call(-1) == -1 and call(L.UNDISTORT_MAX_VIEWS + 1) == -1 and "at most 24" in L.last_error()


# ------------------------------------------------------------------------------------------------ distortion_of
def test_distortion_of_parameter_order_scaling_and_unsupported_models():
    cam = lambda model, params: CIO.ColmapCamera(1, model, 200, 100, np.array(params, np.float64))
    assert U.distortion_of(cam("SIMPLE_PINHOLE", [50, 101, 52]), 200, 100) == (0, (50, 50, 101, 52), (50, 50), ())
    assert U.distortion_of(cam("PINHOLE", [50, 60, 101, 52]), 200, 100) == (1, (50, 60, 101, 52), (50, 60), ())
    assert U.distortion_of(cam("SIMPLE_RADIAL", [50, 101, 52, -0.1]), 200, 100) == (2, (50, 50, 101, 52), (50, 50), (-0.1,))
    assert U.distortion_of(cam("RADIAL", [50, 101, 52, -0.1, 0.2]), 200, 100) == (3, (50, 50, 101, 52), (50, 50), (-0.1, 0.2))
    assert U.distortion_of(cam("OPENCV", [50, 60, 101, 52, 1, 2, 3, 4]), 200, 100) == (4, (50, 60, 101, 52), (50, 60), (1, 2, 3, 4))
    assert (U.distortion_of(cam("FULL_OPENCV", [50, 60, 101, 52, 1, 2, 3, 4, 5, 6, 7, 8]), 200, 100)
            == (6, (50, 60, 101, 52), (50, 60), (1, 2, 3, 4, 5, 6, 7, 8)))
    # loaded at 100 x 25: x by 1/2, y by 1/4; the coefficients act on normalised coordinates and stay
    assert U.distortion_of(cam("OPENCV", [50, 60, 101, 52, 1, 2, 3, 4]), 100, 25) == (4, (25, 15, 50.5, 13), (25, 15), (1, 2, 3, 4))
    for model, n in (("OPENCV_FISHEYE", 8), ("FOV", 5), ("SIMPLE_RADIAL_FISHEYE", 4), ("RADIAL_FISHEYE", 5),
                     ("THIN_PRISM_FISHEYE", 12)):
        with pytest.raises(ValueError, match=model):
            U.distortion_of(cam(model, [1.0] * n), 200, 100)


# ------------------------------------------------------------------------------------------------ loader
CAMERA_FIELDS = ("uid", "image_name", "R", "T", "K", "FoVx", "FoVy", "image_height", "image_width", "world_view_transform",
                 "full_proj_transform", "camera_center", "znear", "zfar")


def _same(a, b):
    if torch.is_tensor(a):
        return torch.equal(a, b)
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b)
    return a == b


def test_read_colmap_undistort_host(tmp_path):
    scan = UC.write_scan(str(tmp_path / "scan"))
    twin = UC.write_scan(str(tmp_path / "twin"), cameras=UC.TWIN_CAMERAS)
    # without the flag: today's behaviour, SIMPLE_RADIAL is refused
    with pytest.raises(ValueError, match="COLMAP camera model SIMPLE_RADIAL not handled: only undistorted datasets"):
        CIO.read_colmap(scan)
    train, test, pcd, extent = CIO.read_colmap(scan, undistort=True, undistort_backend="host")
    train_t, test_t, pcd_t, extent_t = CIO.read_colmap(twin)
    assert [c.image_name for c in train] == [n for n, _ in UC.SCAN_IMAGES] and test == [] and extent == extent_t
    assert np.array_equal(pcd.points, pcd_t.points)
    # the images: undistort_images of the plainly loaded maps
    cams, _ = CIO.read_model(os.path.join(scan, "sparse/0"))
    maps = [CIO.load_edge_image(CIO.edge_map_path(scan, None, name, "DexiNed"), -1) for name, _ in UC.SCAN_IMAGES]
    args = [U.distortion_of(cams[cid], UC.SCAN_W, UC.SCAN_H) for _, cid in UC.SCAN_IMAGES]
    want, blank = U.undistort_images(maps, [a[0] for a in args], [a[1] for a in args], [a[3] for a in args],
                                     [a[2] for a in args], backend="host")
    assert int(blank.max()) < 0.25 * UC.SCAN_W * UC.SCAN_H
    for cam, cam_t, w, plain in zip(train, train_t, want, maps):
        assert torch.equal(cam.original_image, w.clamp(0.0, 1.0)) and cam.original_image.dtype == torch.float32
        assert not torch.equal(cam.original_image, plain)                     # (the pass did something)
        assert torch.equal(cam_t.original_image, plain)
        for field in CAMERA_FIELDS:
            assert _same(getattr(cam, field), getattr(cam_t, field)), field
    # and in numbers: image 1 is the OPENCV camera (fx, fy = 42, 39), image 0 the SIMPLE_RADIAL one (f = 40)
    assert np.array_equal(train[1].K, [[42.0, 0, 24.0], [0, 39.0, 18.0], [0, 0, 1]])
    assert np.array_equal(train[0].K, [[40.0, 0, 24.0], [0, 40.0, 18.0], [0, 0, 1]])
    assert train[1].FoVx == 2 * np.arctan(48 / 84.0) and train[1].FoVy == 2 * np.arctan(36 / 78.0)
    with pytest.raises(ValueError, match="unknown undistort backend"):
        CIO.read_colmap(scan, undistort=True, undistort_backend="numpy")


def test_read_colmap_undistort_resized_and_blank_warning(tmp_path):
    """-r 2 halves the maps before the pass, and the intrinsics follow; a principal point far outside the frame leaves more
    than a quarter of the image blank, which is reported."""
    scan = UC.write_scan(str(tmp_path / "scan"))
    train, _, _, _ = CIO.read_colmap(scan, resolution=2, undistort=True, undistort_backend="host")
    assert tuple(train[0].original_image.shape) == (1, UC.SCAN_H // 2, UC.SCAN_W // 2)
    cams, _ = CIO.read_model(os.path.join(scan, "sparse/0"))
    assert U.distortion_of(cams[1], UC.SCAN_W // 2, UC.SCAN_H // 2)[1] == (20.0, 20.0, 12.65, 8.55)
    far = UC.write_scan(str(tmp_path / "far"), cameras={1: ("PINHOLE", [40.0, 40.0, 60.0, 18.0]),
                                                        2: ("PINHOLE", [40.0, 40.0, 24.0, 18.0])})
    with pytest.warns(UserWarning, match="00000.png are blank"):
        CIO.read_colmap(far, undistort=True, undistort_backend="host")


def test_driver_accepts_undistort(tmp_path):
    from curve_gaussian_amd import train as T
    dataset, _, args = T.parse_args(["-s", str(tmp_path), "-m", str(tmp_path / "out"), "--undistort"])
    assert args.undistort is True and dataset.undistort is True
    dataset, _, _ = T.parse_args(["-s", str(tmp_path), "-m", str(tmp_path / "out")])
    assert dataset.undistort is False and T.ModelParams().undistort is False
