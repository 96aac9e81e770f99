"""GPU: cgs_edge_gradients / cgs_edge_trace (csrc/edge_detect.hip) against the host back end of ops.edge_detect, the chunking
of the ops, a disc whose edge is known, and the tool ``python -m curve_gaussian_amd.edge_detect`` on the device."""
import functools
import os

import numpy as np
import pytest
import torch

import edge_detect_cases as EC
from curve_gaussian_amd import _lib as L
from curve_gaussian_amd import edge_detect as TOOL
from curve_gaussian_amd.ops import edge_detect as E
from test_edge_detect_cpu import check_disc, rounding_margin_fraction

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _small_on_gpu():
    """The views of (a) and their gradients on the device, computed once."""
    views = EC.small_views()
    return views, E.edge_gradients(views, EC.SIGMA, backend="gpu")


@pytest.mark.parametrize("name, views, sigma", [("small", EC.small_views, EC.SIGMA), ("degenerate", EC.degenerate_views, EC.DEGENERATE_SIGMA),
                                                ("batch", EC.batch_views, EC.SIGMA), ("unsmoothed", EC.small_views, 0.0),
                                                ("widest", EC.small_views, 4.0)])
def test_gradients_against_float64(name, views, sigma):
    """gx, gy and m within 2e-5 of the float64 host result.  Inputs are at most 1 and each blur pass sums at most 25 weighted
    terms of total weight 1: about (n + 1) 2^-24 = 1.6e-6 per pass, the same again for Sobel over 4, and the square root
    keeps relative error; 2e-5 leaves a factor of about 4."""
    images = views()
    assert name != "batch" or len(images) > L.EDGE_MAX_VIEWS
    got = E.edge_gradients(images, sigma, backend="gpu")
    worst = 0.0
    for v, im in enumerate(images):
        want = E.gradients_host_f64(im, sigma)
        for g, w in zip((got[0][v], got[1][v], got[2][v]), want):
            assert g.is_cuda and g.dtype == torch.float32 and tuple(g.shape) == w.shape
            worst = max(worst, float(np.abs(g.cpu().numpy().astype(np.float64) - w).max()))
    print(f"{name}: largest difference {worst:.3e}")
    assert worst <= 2e-5


def test_gradients_read_images_where_they_are_and_ignore_alpha():
    views, (gx, gy, m) = _small_on_gpu()
    again = E.edge_gradients([torch.from_numpy(v).to(DEV) for v in views], EC.SIGMA, backend="gpu")
    assert all(torch.equal(a, b) for a, b in zip(again[2], m)) and all(torch.equal(a, b) for a, b in zip(again[0], gx))
    rgb = E.edge_gradients([np.ascontiguousarray(views[2][:, :, :3])], EC.SIGMA, backend="gpu")
    assert views[2].shape[2] == 4 and torch.equal(rgb[0][0], gx[2]) and torch.equal(rgb[1][0], gy[2]) and torch.equal(rgb[2][0], m[2])


@pytest.mark.parametrize("thin", [True, False])
def test_tracing_is_bit_identical_to_the_host_on_gradients(thin):
    """trace_edges on the device's own gx, gy, m against the host rule on the same tensors: exact, no pixel excluded."""
    _, (gx, gy, m) = _small_on_gpu()
    stats = {}
    got = E.trace_edges(gx, gy, m, EC.LOW, EC.HIGH, thin, backend="gpu", stats=stats)
    want = E.trace_edges([t.cpu() for t in gx], [t.cpu() for t in gy], [t.cpu() for t in m], EC.LOW, EC.HIGH, thin, backend="host")
    assert stats["rounds"] and all(r >= 1 for r in stats["rounds"])
    for g, w in zip(got, want):
        assert g.is_cuda and g.dtype == torch.float32 and g.shape == w.shape and int((w > 0).sum()) > 50
        assert torch.equal(g.cpu(), w)


def test_tracing_is_bit_identical_to_the_host_on_hand_made_fields():
    """(d) and (e) in two calls (views of different sizes share a call), against the host rule and the hand-written sets."""
    cases = EC.trace_cases()
    m = [torch.from_numpy(c.m) for c in cases]
    zero = [torch.zeros_like(t) for t in m]
    stats = {}
    got = E.trace_edges(m, zero, m, EC.LOW, EC.HIGH, thin=False, backend="gpu", stats=stats)
    want = E.trace_edges(m, zero, m, EC.LOW, EC.HIGH, thin=False, backend="host")
    for c, g, w in zip(cases, got, want):
        assert torch.equal(g.cpu(), w), c.name
        assert np.array_equal(g.cpu().numpy()[0] > 0, c.kept), c.name
    print(f"propagation rounds: {stats['rounds']}")
    assert stats["rounds"][0] > 2            # the serpentine chain crosses tile borders: it cannot settle in one round
    alone = {}
    E.trace_edges(m[1:2], zero[1:2], m[1:2], EC.LOW, EC.HIGH, thin=False, backend="gpu", stats=alone)
    assert alone["rounds"] == [1]            # no strong pixel: the first round changes nothing
    thin = EC.thin_cases()
    f = [[torch.from_numpy(a) for a in (c.gx, c.gy, c.m)] for c in thin]
    args = ([t[0] for t in f], [t[1] for t in f], [t[2] for t in f])
    got = E.trace_edges(*args, EC.LOW, EC.HIGH, thin=True, backend="gpu")
    want = E.trace_edges(*args, EC.LOW, EC.HIGH, thin=True, backend="host")
    for c, g, w in zip(thin, got, want):
        assert torch.equal(g.cpu(), w), c.name
        assert np.array_equal(g.cpu().numpy()[0] > 0, c.kept), c.name


def test_composed_op_and_chunking():
    views, (gx, gy, m) = _small_on_gpu()
    whole = E.detect_edges(views, EC.SIGMA, EC.LOW, EC.HIGH, True, backend="gpu")
    parts = E.trace_edges(gx, gy, m, EC.LOW, EC.HIGH, True, backend="gpu")
    assert all(torch.equal(a, b) for a, b in zip(whole, parts))
    batch = EC.batch_views()
    assert len(batch) == 26 > L.EDGE_MAX_VIEWS
    together = E.detect_edges(batch, backend="gpu")
    assert len(together) == 26 and sum(int((t > 0).sum()) for t in together) > 100
    for v, im in enumerate(batch):
        assert torch.equal(E.detect_edges([im], backend="gpu")[0], together[v]), v


@pytest.mark.parametrize("backend", ["gpu", "host"])
def test_disc(backend):
    """Meaning, not parity: with the defaults the kept pixels are the circle."""
    check_disc(E.detect_edges([EC.disc_image()], backend=backend)[0])


def test_bad_calls_launch_nothing():
    lib = L.load()
    f = torch.full((8, 8), 0.2, device=DEV)
    e = torch.full((8, 8), -1.0, device=DEV)
    lib.cgs_prof_reset()
    lib.cgs_prof_enable(1)
    try:
        with pytest.raises(ValueError, match="0 < low <= high"):
            E.trace_edges([f], [f], [f], 0.2, 0.1)
        import ctypes as C
        table = (L.EdgeTraceView * 1)(L.EdgeTraceView(f.data_ptr(), f.data_ptr(), f.data_ptr(), e.data_ptr(), 0, 8, 8))
        assert lib.cgs_edge_trace(1, C.cast(table, C.c_void_p), 0.05, 0.15, 1, None, L.raw_stream(DEV)) == -1
        assert "NULL" in L.last_error()
        assert not any(k.startswith("edge_") for k in L.prof_collect())
        torch.cuda.synchronize()
        assert float(e.min()) == -1.0 and float(e.max()) == -1.0
        out = E.trace_edges([f], [f], [f], 0.05, 0.15, thin=False)
        prof = L.prof_collect()
        assert prof["edge_classify"][1] == 1 and prof["edge_propagate"][1] == 1 and prof["edge_response"][1] == 1
        assert float(out[0].min()) == 1.0
    finally:
        lib.cgs_prof_enable(0)
        lib.cgs_prof_reset()


def test_tool_on_the_device(tmp_path):
    """The files of --backend gpu equal those of --backend host except where 255 e lies within 0.01 of a rounding boundary
    (the gradients agree within 2e-5, 255 times that is 5.1e-3); at most 1 % of the pixels may be excepted."""
    from PIL import Image
    gpu = EC.write_emap_scan(str(tmp_path / "gpu"))
    host = EC.write_emap_scan(str(tmp_path / "host"))
    assert TOOL.main(["--scan", gpu, "--backend", "gpu"]) == 0
    assert TOOL.main(["--scan", host, "--backend", "host"]) == 0
    e = E.detect_edges(EC.scan_photographs(), backend="host")
    assert rounding_margin_fraction(e) <= 0.01
    excepted = total = 0
    for k, ref in enumerate(e):
        a = np.array(Image.open(os.path.join(gpu, "edge_PidiNet", f"{k}_colors.png")))
        b = np.array(Image.open(os.path.join(host, "edge_PidiNet", f"{k}_colors.png")))
        t = 255.0 * ref[0].double().numpy()
        near = np.abs(t - np.floor(t) - 0.5) < 0.01
        assert a.shape == b.shape == (EC.SCAN_H, EC.SCAN_W) and a.dtype == np.uint8 and int((b > 0).sum()) > 20
        assert np.array_equal(a[~near], b[~near]), k
        excepted += int(near.sum())
        total += near.size
    assert excepted <= 0.01 * total
