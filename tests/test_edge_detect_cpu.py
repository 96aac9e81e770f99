"""CPU: the host back end of ops.edge_detect (what the kernels of csrc/edge_detect.hip are held against), the argument checks of
the ops and of the C ABI, and the tool ``python -m curve_gaussian_amd.edge_detect`` on two tiny scans."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import edge_detect_cases as EC
from curve_gaussian_amd import _lib as L
from curve_gaussian_amd import edge_detect as TOOL
from curve_gaussian_amd.ops import edge_detect as E


# ------------------------------------------------------------------------------------------------ gradients
@pytest.mark.parametrize("name, views, sigma", [("small", EC.small_views, EC.SIGMA), ("degenerate", EC.degenerate_views, EC.DEGENERATE_SIGMA),
                                                ("unsmoothed", EC.degenerate_views, 0.0)])
def test_host_gradients_match_plain_loops(name, views, sigma):
    """Both sides are float64 and differ only in the order of their sums: 1e-12 on values of at most 1, and the result is
    that value rounded to float32 once."""
    images = views()
    gx, gy, m = E.edge_gradients(images, sigma, backend="host")
    assert len(gx) == len(gy) == len(m) == len(images)
    for v, im in enumerate(images):
        want = EC.gradients_loop_f64(im, sigma)
        got64 = E.gradients_host_f64(im, sigma)
        for w, g64, g in zip(want, got64, (gx[v], gy[v], m[v])):
            assert g.dtype == torch.float32 and tuple(g.shape) == im.shape[:2] == w.shape
            assert np.abs(g64 - w).max() <= 1e-12
            assert np.array_equal(g.numpy(), g64.astype(np.float32))


def test_taps_step_and_alpha():
    taps, r = E.gaussian_taps(1.4)
    assert r == 5 and taps.dtype == np.float32 and len(taps) == 11 and abs(float(taps.astype(np.float64).sum()) - 1) < 1e-6
    assert np.array_equal(taps, taps[::-1]) and E.gaussian_taps(4.0)[1] == 12 and E.gaussian_taps(0.0)[1] == 0
    # a full black-to-white step without smoothing has magnitude 1
    step = np.zeros((5, 6), np.uint8)
    step[:, 3:] = 255
    gx, gy, m = E.edge_gradients([step], 0.0, backend="host")
    assert float(m[0].max()) == 1.0 and float(gx[0][2, 2]) == 1.0 and float(gy[0].abs().max()) == 0.0
    assert float(E.edge_gradients([step.T.copy()], 0.0, backend="host")[1][0][2, 2]) == 1.0   # gy grows downwards
    # alpha is ignored
    rgba = EC.small_views()[2]
    a = E.edge_gradients([rgba], backend="host")
    b = E.edge_gradients([np.ascontiguousarray(rgba[:, :, :3])], backend="host")
    assert all(torch.equal(x[0], y[0]) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ tracing
@pytest.mark.parametrize("case", EC.trace_cases(), ids=lambda c: c.name)
def test_host_hysteresis_matches_hand_written_sets(case):
    m = torch.from_numpy(case.m)
    e = E.trace_edges([m], [torch.zeros_like(m)], [m], EC.LOW, EC.HIGH, thin=False, backend="host")[0]
    assert e.dtype == torch.float32 and tuple(e.shape) == (1,) + case.m.shape
    assert np.array_equal(e[0].numpy() > 0, case.kept)
    want = np.where(case.kept, np.minimum(case.m / np.float32(EC.HIGH), np.float32(1)), np.float32(0))
    assert np.array_equal(e[0].numpy(), want)


def test_inclusive_threshold_values():
    case = EC.inclusive_thresholds()
    m = torch.from_numpy(case.m)
    e = E.trace_edges([m], [torch.zeros_like(m)], [m], EC.LOW, EC.HIGH, thin=False, backend="host")[0][0].numpy()
    assert e[1, 3] == 1.0 and e[1, 2] == np.float32(EC.LOW) / np.float32(EC.HIGH) and e[3, 2] == 0 and e[1, 8] == 0 and e[1, 9] == 0


@pytest.mark.parametrize("case", EC.thin_cases(), ids=lambda c: c.name)
def test_host_thinning_matches_hand_written_sets(case):
    gx, gy, m = (torch.from_numpy(a) for a in (case.gx, case.gy, case.m))
    e = E.trace_edges([gx], [gy], [m], EC.LOW, EC.HIGH, thin=True, backend="host")[0][0].numpy()
    assert np.array_equal(e > 0, case.kept), (case.name, np.argwhere(e > 0).tolist())
    assert np.array_equal(e, case.kept.astype(np.float32))           # every value is strong: the response saturates
    plain = E.trace_edges([gx], [gy], [m], EC.LOW, EC.HIGH, thin=False, backend="host")[0][0].numpy()
    assert np.array_equal(plain > 0, case.m > 0)                     # without thinning every pixel stays


def test_disc_on_the_host():
    check_disc(E.detect_edges([EC.disc_image()], backend="host")[0])


def check_disc(e):
    """Every kept pixel within 1.5 px of the circle, 95 % of 360 samples of the circle with a kept pixel within 1.5 px, and
    the noise-only corners exactly 0 (shared with the GPU test)."""
    e = e.detach().cpu().numpy()[0]
    ys, xs = np.nonzero(e > 0)
    assert len(ys) > 100
    assert np.abs(np.hypot(xs - EC.DISC_CX, ys - EC.DISC_CY) - EC.DISC_R).max() <= 1.5
    ang = np.deg2rad(np.arange(360))
    px, py = EC.DISC_CX + EC.DISC_R * np.cos(ang), EC.DISC_CY + EC.DISC_R * np.sin(ang)
    near = np.hypot(px[:, None] - xs[None, :], py[:, None] - ys[None, :]).min(1) <= 1.5
    print(f"disc: {len(ys)} kept pixels, {int(near.sum())} of 360 samples covered")
    assert near.mean() >= 0.95
    for cy, cx in ((slice(0, 10), slice(0, 10)), (slice(0, 10), slice(-10, None)), (slice(-10, None), slice(0, 10)),
                   (slice(-10, None), slice(-10, None))):
        assert float(np.abs(e[cy, cx]).max()) == 0.0
    assert e.min() >= 0.0 and e.max() <= 1.0


# ------------------------------------------------------------------------------------------------ arguments
def test_argument_errors():
    img = np.zeros((4, 5, 3), np.uint8)
    f = torch.zeros(4, 5)
    for fn, args in ((E.edge_gradients, ([img],)), (E.trace_edges, ([f], [f], [f])), (E.detect_edges, ([img],))):
        with pytest.raises(ValueError, match="unknown edge detection backend 'cpu'"):
            fn(*args, backend="cpu")
    for bad in (np.zeros((4, 5, 3), np.float32), np.zeros((4, 5, 2), np.uint8), np.zeros((4, 5, 3, 1), np.uint8),
                np.zeros((0, 5, 3), np.uint8), np.zeros(5, np.uint8), "x"):
        with pytest.raises(ValueError, match=r"images\[0\]"):
            E.edge_gradients([bad], backend="host")
        with pytest.raises(ValueError, match=r"images\[0\]"):
            E.detect_edges([bad], backend="host")
    for sigma in (-0.1, 4.5, float("nan")):
        with pytest.raises(ValueError, match="sigma"):
            E.edge_gradients([img], sigma, backend="host")
    for low, high in ((0.0, 0.1), (-1.0, 0.1), (0.2, 0.1), (float("nan"), 0.1), (0.1, float("nan")), (0.1, float("inf"))):
        with pytest.raises(ValueError, match="0 < low <= high"):
            E.trace_edges([f], [f], [f], low, high, backend="host")
        with pytest.raises(ValueError, match="0 < low <= high"):
            E.detect_edges([img], low=low, high=high, backend="host")
    with pytest.raises(ValueError, match="differ in shape"):
        E.trace_edges([f], [torch.zeros(5, 4)], [f], backend="host")
    with pytest.raises(ValueError, match="float32"):
        E.trace_edges([f.double()], [f], [f], backend="host")
    assert E.trace_edges([f], [f], [f], 0.1, 0.1, backend="host")[0].shape == (1, 4, 5)      # low == high is allowed
    assert E.detect_edges([], backend="host") == []
    if not torch.cuda.is_available():
        for fn, args in ((E.edge_gradients, ([img],)), (E.trace_edges, ([f], [f], [f])), (E.detect_edges, ([img],))):
            with pytest.raises(L.CurveGSError, match="backend='host'"):
                fn(*args)


def test_c_abi_rejects_bad_calls_without_a_gpu():
    """The argument checks of both entry points come before any device work."""
    lib = L.load()
    assert C.sizeof(L.EdgeGradientView) == 48 and C.sizeof(L.EdgeTraceView) == 48
    taps = (C.c_float * 25)(*([0.04] * 25))

    def grad(n, radius=1, taps=taps, **kw):
        a = dict(pixels=16, gx=32, gy=48, m=64, height=8, width=8, channels=3)
        a.update(kw)
        table = (L.EdgeGradientView * 1)(L.EdgeGradientView(a["pixels"], a["gx"], a["gy"], a["m"], a["height"], a["width"],
                                                            a["channels"], 0))
        return lib.cgs_edge_gradients(n, C.cast(table, C.c_void_p), C.cast(taps, C.c_void_p) if taps else None, radius, None)

    for kw, word in ((dict(radius=13), "radius=13"), (dict(radius=-1), "radius=-1"), (dict(pixels=None), "NULL"),
                     (dict(m=None), "NULL"), (dict(taps=None), "NULL"), (dict(height=0), "height=0"), (dict(width=-3), "width=-3"),
                     (dict(channels=2), "channels=2")):
        assert grad(1, **kw) == -1 and "cgs_edge_gradients: invalid argument" in L.last_error() and word in L.last_error(), kw
    assert grad(0) == -1 and "n_views=0" in L.last_error()
    assert grad(L.EDGE_MAX_VIEWS + 1) == -1 and "1..24" in L.last_error()
    assert lib.cgs_edge_gradients(1, None, C.cast(taps, C.c_void_p), 1, None) == -1 and "NULL" in L.last_error()

    def trace(n, low=0.05, high=0.15, flag=128, **kw):
        a = dict(gx=16, gy=32, m=48, e=64, state=80, height=8, width=8)
        a.update(kw)
        table = (L.EdgeTraceView * 1)(L.EdgeTraceView(a["gx"], a["gy"], a["m"], a["e"], a["state"], a["height"], a["width"]))
        return lib.cgs_edge_trace(n, C.cast(table, C.c_void_p), low, high, 1, flag, None)

    for kw, word in ((dict(low=0.0), "low=0"), (dict(low=-0.5), "low=-0.5"), (dict(low=0.2, high=0.1), "low=0.2"),
                     (dict(low=float("nan")), "low=nan"), (dict(high=float("nan")), "high=nan"), (dict(flag=None), "NULL"),
                     (dict(state=None), "NULL"), (dict(e=None), "NULL"), (dict(height=0), "height=0"), (dict(width=0), "width=0")):
        assert trace(1, **kw) == -1 and "cgs_edge_trace: invalid argument" in L.last_error() and word in L.last_error(), kw
    assert trace(0) == -1 and trace(-1) == -1 and trace(L.EDGE_MAX_VIEWS + 1) == -1 and "1..24" in L.last_error()
    assert lib.cgs_edge_trace(1, None, 0.05, 0.15, 1, 128, None) == -1 and "NULL" in L.last_error()


# ------------------------------------------------------------------------------------------------ the tool
def _png(path):
    from PIL import Image
    with Image.open(path) as im:
        assert im.mode == "L"
        return np.array(im)


def _expected_maps():
    e = E.detect_edges(EC.scan_photographs(), backend="host")
    return [torch.round(m[0] * 255.0).numpy().astype(np.uint8) for m in e], e


def rounding_margin_fraction(e):
    """The share of pixels whose 255 e lies within 0.01 of a rounding boundary k + 0.5 (shared with the GPU test)."""
    t = 255.0 * torch.cat([m.flatten() for m in e]).double().numpy()
    return float((np.abs(t - np.floor(t) - 0.5) < 0.01).mean())


def test_tool_on_an_emap_scan(tmp_path, capsys):
    from curve_gaussian_amd.scene import dataset_io as IO
    scan = EC.write_emap_scan(str(tmp_path / "emap"))
    with pytest.raises(FileNotFoundError):
        IO.read_emap(scan, detector="PidiNet")                        # photographs and poses only: nothing to train on
    assert TOOL.main(["--scan", scan, "--backend", "host"]) == 0
    assert "wrote 3 edge maps" in capsys.readouterr().out
    want, e = _expected_maps()
    assert rounding_margin_fraction(e) <= 0.01                        # the cap the GPU test's exception list is held to
    cams = IO.read_emap(scan, detector="PidiNet")
    assert len(cams) == EC.SCAN_VIEWS
    for k, (cam, w) in enumerate(zip(cams, want)):
        assert int((w > 0).sum()) > 20                                # there are edges
        assert np.array_equal(_png(os.path.join(scan, "edge_PidiNet", f"{k}_colors.png")), w)
        assert tuple(cam.original_image.shape) == (3, EC.SCAN_H, EC.SCAN_W)
        assert torch.equal(cam.original_image[0], torch.from_numpy(w) / 255.0)
    meta = json.load(open(os.path.join(scan, "edge_PidiNet", "detector.json")))
    assert (meta["sigma"], meta["low"], meta["high"], meta["thin"], meta["backend"], meta["views"]) == (1.4, 0.05, 0.15, True, "host", 3)
    # an existing folder is left alone ...
    before = _png(os.path.join(scan, "edge_PidiNet", "0_colors.png"))
    with pytest.raises(FileExistsError, match="--overwrite"):
        TOOL.main(["--scan", scan, "--backend", "host", "--sigma", "0", "--no_thin"])
    assert np.array_equal(_png(os.path.join(scan, "edge_PidiNet", "0_colors.png")), before)
    # ... unless asked, and the parameters arrive
    assert TOOL.main(["--scan", scan, "--backend", "host", "--sigma", "0", "--low", "0.1", "--high", "0.3", "--no_thin", "--overwrite"]) == 0
    other = E.detect_edges(EC.scan_photographs()[:1], 0.0, 0.1, 0.3, False, backend="host")[0]
    after = _png(os.path.join(scan, "edge_PidiNet", "0_colors.png"))
    assert np.array_equal(after, torch.round(other[0] * 255.0).numpy().astype(np.uint8)) and not np.array_equal(after, before)
    assert json.load(open(os.path.join(scan, "edge_PidiNet", "detector.json")))["thin"] is False
    # detect_scan is the function behind it
    written = TOOL.detect_scan(scan, backend="host", overwrite=True)
    assert [os.path.basename(p) for p in written] == [f"{k}_colors.png" for k in range(3)]
    assert np.array_equal(_png(written[0]), before)


def test_tool_refuses_an_emap_name_that_is_not_png(tmp_path):
    scan = EC.write_emap_scan(str(tmp_path / "emap"))
    meta_path = os.path.join(scan, "meta_data.json")
    meta = json.load(open(meta_path))
    meta["frames"][1]["rgb_path"] = "1_colors.jpg"
    json.dump(meta, open(meta_path, "w"))
    with pytest.raises(ValueError, match=r"'1_colors.jpg' does not end in \.png"):
        TOOL.main(["--scan", scan, "--backend", "host"])
    assert not os.path.exists(os.path.join(scan, "edge_PidiNet"))


def test_tool_on_a_colmap_scan(tmp_path):
    from curve_gaussian_amd.scene import colmap_io as CIO
    scan = EC.write_colmap_scan(str(tmp_path / "colmap"))
    assert TOOL.main(["--scan", scan, "--backend", "host"]) == 0
    want, _ = _expected_maps()
    train, _, _, _ = CIO.read_colmap(scan, detector="PidiNet")
    assert [c.image_name for c in train] == [f"{k:05d}.png" for k in range(EC.SCAN_VIEWS)]
    for k, (cam, w) in enumerate(zip(train, want)):
        assert CIO.edge_map_path(scan, None, f"{k:05d}.png", "PidiNet") == os.path.join(scan, "edge_PidiNet", f"{k:05d}.png")
        assert np.array_equal(_png(os.path.join(scan, "edge_PidiNet", f"{k:05d}.png")), w)
        assert tuple(cam.original_image.shape) == (1, EC.SCAN_H, EC.SCAN_W)
        assert torch.equal(cam.original_image[0], torch.from_numpy(w) / 255.0)
    assert os.path.exists(os.path.join(scan, "edge_PidiNet", "detector.json"))
    with pytest.raises(FileExistsError, match="--overwrite"):
        TOOL.main(["--scan", scan, "--backend", "host"])
    # an image folder whose name the path rule cannot rewrite would be overwritten by its own edge maps: refused
    os.rename(os.path.join(scan, "images"), os.path.join(scan, "input"))
    with pytest.raises(ValueError, match="replace the photograph"):
        TOOL.main(["--scan", scan, "--images", "input", "--backend", "host", "--overwrite"])
