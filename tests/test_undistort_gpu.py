"""GPU: cgs_undistort_images (csrc/undistort.hip) against the float64 host back end of ops.undistort, its chunking and
argument checks, and the loader that feeds it."""
import ctypes as C

import numpy as np
import pytest
import torch

import undistort_cases as UC
from curve_gaussian_amd import _lib as L
from curve_gaussian_amd.ops import undistort as U
from curve_gaussian_amd.scene import colmap_io as CIO

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def test_parity_with_the_host_back_end():
    """One call, every supported model plus a second OPENCV view, the sizes 37x53 (C=1), 53x37 (C=3), 1x1, 64x64 and 70x130
    (C=1): odd sizes, several channels, a partial last workgroup, a view smaller than a workgroup, and views that look
    past their source (fill taps, blank pixels).  Images are uniform in [0, 1].

    Bound 1e-6 on the largest difference: the coordinates are float64 on both sides; the kernel's blend is four float32
    products of values in [0, 1] and three additions, a few ulps of 1.0 (about 5e-7); bilinear interpolation is continuous
    across a tap boundary, so a last-bit difference in `floor` changes nothing.  The blank counts must be EQUAL: the
    coefficients are chosen so that no tap position lies within 1e-9 of an integer (asserted here on the host)."""
    images, models, intr, coefs, focals = UC.parity_inputs()
    assert len(images) <= L.UNDISTORT_MAX_VIEWS and sorted(set(models)) == [0, 1, 2, 3, 4, 6] and models.count(4) == 2
    for im, m, k, c, f in zip(images, models, intr, coefs, focals):
        u, v = U.source_positions(im.shape[1], im.shape[2], m, k, c, f)
        assert min(np.abs(u - np.round(u)).min(), np.abs(v - np.round(v)).min()) > 1e-9
    want, want_blank = U.undistort_images(images, models, intr, coefs, focals, fill=0.375, backend="host")
    got, blank = U.undistort_images(images, models, intr, coefs, focals, fill=0.375, backend="gpu")
    assert blank.is_cuda and blank.dtype == torch.int32
    worst = 0.0
    for g, w, im in zip(got, want, images):
        assert g.is_cuda and g.dtype == torch.float32 and g.shape == im.shape
        worst = max(worst, float((g.cpu().double() - w.double()).abs().max()))
    print(f"largest difference {worst:.3e}; blank pixels {want_blank.tolist()}")
    assert worst <= 1e-6
    assert blank.cpu().tolist() == want_blank.tolist()
    assert int(want_blank.sum()) > 0 and int((want_blank == 0).sum()) > 0       # both kinds of view occur
    # images that are already on the device are read where they are
    again, _ = U.undistort_images([im.to(DEV) for im in images], models, intr, coefs, focals, fill=0.375, backend="gpu")
    assert all(torch.equal(a, g) for a, g in zip(again, got))


def test_identity_and_shift_are_exact_on_the_device():
    H, W, f, fill = 37, 53, 64.0, 0.25
    img = torch.rand(2, H, W, generator=torch.Generator().manual_seed(1))
    outs, counts = U.undistort_images([img, img], [1, 0], [(f, f, W / 2.0, H / 2.0), (f, f, W / 2.0 + 3, H / 2.0 - 2)], [(), ()],
                                      [(f, f), (f, f)], fill=fill)
    want = torch.full_like(img, fill)
    want[:, 2:, :W - 3] = img[:, :H - 2, 3:]
    assert torch.equal(outs[0].cpu(), img) and torch.equal(outs[1].cpu(), want)
    assert counts.cpu().tolist() == [0, H * W - (H - 2) * (W - 3)]


def test_chunking_equals_per_view_calls():
    n = 2 * L.UNDISTORT_MAX_VIEWS + 1
    g = torch.Generator().manual_seed(2)
    images = [torch.rand(1, 8, 8, generator=g) for _ in range(n)]
    models = [(0, 1, 2, 3, 4, 6)[v % 6] for v in range(n)]
    intr = [(7.3 + 0.1 * v, 6.9 + 0.07 * v, 3.1 + 0.11 * v, 4.7 - 0.09 * v) for v in range(n)]
    coefs = [((), (), (-0.2,), (-0.2, 0.1), (0.1, 0.02, 0.03, -0.01), (0.1, 0.02, 0.03, -0.01, 0.01, 0.05, 0.01, 0.002))[v % 6]
             for v in range(n)]
    focals = [(k[0], k[1]) for k in intr]
    outs, blank = U.undistort_images(images, models, intr, coefs, focals)
    assert len(outs) == n and blank.shape == (n,)
    for v in range(n):
        one, b = U.undistort_images(images[v:v + 1], models[v:v + 1], intr[v:v + 1], coefs[v:v + 1], focals[v:v + 1])
        assert torch.equal(one[0], outs[v]) and int(b[0]) == int(blank[v]), v
    assert int(blank.sum()) > 0


def _view(src, dst, model=4, channels=1, fx=8.0, out_fx=8.0):
    return L.UndistortView(src.data_ptr(), dst.data_ptr(), channels, 8, 8, model, fx, 8.0, 4.0, 4.0, out_fx, 8.0,
                           (C.c_double * 8)(0.1, 0.0, 0.0, 0.0))


def test_degenerate_and_bad_calls_launch_nothing():
    lib = L.load()
    src = torch.rand(4, 8, 8, device=DEV)
    dst = torch.full_like(src, -1.0)
    blank = torch.zeros(2, dtype=torch.int32, device=DEV)
    stream = L.raw_stream(DEV)

    def call(n, *views):
        table = (L.UndistortView * max(len(views), 1))(*views)
        return lib.cgs_undistort_images(n, C.cast(table, C.c_void_p), 0.0, L.ptr(blank), stream)

    lib.cgs_prof_reset()
    lib.cgs_prof_enable(1)
    try:
        assert call(0) == 0 and lib.cgs_undistort_images(0, None, 0.0, None, stream) == 0
        for views, word in (((_view(src, dst, model=5),), "model id 5"), ((_view(src, dst, model=-1),), "model id -1"),
                            ((_view(src, dst, fx=0.0),), "fx=0"), ((_view(src, dst, out_fx=0.0),), "out_fx=0"),
                            ((_view(src, dst, channels=5),), "channels=5"), ((_view(src, dst, channels=0),), "channels=0"),
                            ((_view(src, src),), "dst == src"),
                            ((_view(src, dst), _view(src, dst, model=9)), "view 1: camera model id 9")):
            assert call(len(views), *views) == -1, word
            assert "cgs_undistort_images: invalid argument" in L.last_error() and word in L.last_error(), L.last_error()
        assert call(-1) == -1 and "n_views=-1" in L.last_error()
        assert call(L.UNDISTORT_MAX_VIEWS + 1) == -1 and "at most" in L.last_error()
        assert lib.cgs_undistort_images(1, None, 0.0, L.ptr(blank), stream) == -1 and "NULL" in L.last_error()
        table = (L.UndistortView * 1)(_view(src, dst))
        assert lib.cgs_undistort_images(1, C.cast(table, C.c_void_p), 0.0, None, stream) == -1 and "NULL" in L.last_error()
        assert "undistort_images" not in L.prof_collect()                     # nothing was launched ...
        torch.cuda.synchronize()
        assert float(dst.min()) == -1.0 and float(dst.max()) == -1.0 and blank.cpu().tolist() == [0, 0]
        assert call(1, _view(src, dst)) == 0
        assert L.prof_collect()["undistort_images"][1] == 1                    # ... and a good call is one launch
    finally:
        lib.cgs_prof_enable(0)
        lib.cgs_prof_reset()
    with pytest.raises(ValueError, match="model id 7"):                        # the op refuses it like the host back end
        U.undistort_images([src[:1].cpu()], [7], [(8.0, 8.0, 4.0, 4.0)], [()], [(8.0, 8.0)])


def test_loader_on_the_device(tmp_path):
    from curve_gaussian_amd.scene import GaussianCurveModel, Scene
    scan = UC.write_scan(str(tmp_path / "scan"))
    host, _, _, _ = CIO.read_colmap(scan, undistort=True, undistort_backend="host")
    train, _, _, _ = CIO.read_colmap(scan, undistort=True)
    gm = GaussianCurveModel(0, 12, device=DEV)
    scene = Scene(scan, gm, undistort=True, device="cuda")
    for cams in (train, scene.getTrainCameras()):
        assert len(cams) == len(host)
        for cam, ref in zip(cams, host):
            assert cam.original_image.is_cuda and cam.image_name == ref.image_name
            assert float((cam.original_image.cpu() - ref.original_image).abs().max()) <= 1e-6
    assert scene.getTrainCameras()[0].world_view_transform.is_cuda
    assert gm._curve_points.is_cuda and gm._curve_points.shape[0] > 0          # create_from_pcd ran
    with pytest.raises(ValueError, match="SIMPLE_RADIAL not handled"):
        Scene(scan, GaussianCurveModel(0, 12, device=DEV), device="cuda")
