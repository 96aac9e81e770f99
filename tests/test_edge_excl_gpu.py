"""GPU: cgs_ray_claims / cgs_ray_wins against the host back end, bit for bit; list lengths, contention on one pixel,
accumulation, seed_points(exclusive=True) on both drawn scans, a Scene seeded through the claims, and the raw calls'
argument errors."""
import ctypes

import numpy as np
import pytest
import torch

import edge_dir_cases as DC
import edge_excl_cases as XC
import edge_seed_cases as SC
from curve_gaussian_amd.ops import edge_seed as SD

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENTINEL = 0xABCD


def _sentinel_words(n):
    return torch.from_numpy(np.full(n, SENTINEL, np.uint16)).to(DEV)


class _Raw:
    """The raw C calls on device copies of one case."""

    def __init__(self, bounds, dims, index, support, K, M, bits, H, W):
        from curve_gaussian_amd import _lib as L
        self.L, self.lib = L, L.load()
        lo, hi = (np.asarray(b, np.float64) for b in bounds)
        self.lo, self.step = (ctypes.c_double * 3)(*lo), (ctypes.c_double * 3)(*((hi - lo) / np.array(dims, np.float64)))
        self.dims, self.H, self.W, self.V, self.M = dims, H, W, len(K), len(index)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        self.index, self.support = dev(np.asarray(index, np.int32)), dev(np.asarray(support, np.uint16))
        self.K, self.Mx, self.bits = dev(np.asarray(K, np.float64)), dev(np.asarray(M, np.float64).reshape(-1, 12)), bits.to(DEV)

    def _head(self, **kw):
        L = self.L
        a = dict(nx=self.dims[0], ny=self.dims[1], nz=self.dims[2], lo=ctypes.cast(self.lo, ctypes.c_void_p),
                 step=ctypes.cast(self.step, ctypes.c_void_p), M=self.M, index=L.ptr(self.index), support=L.ptr(self.support),
                 V=self.V, intr=L.ptr(self.K), w2c=L.ptr(self.Mx), H=self.H, W=self.W, bits=L.ptr(self.bits))
        a.update(kw)
        return [a[k] for k in ("nx", "ny", "nz", "lo", "step", "M", "index", "support", "V", "intr", "w2c", "H", "W", "bits")]

    def claims(self, best, clear=1, **kw):
        best_p = kw.pop("best_ptr", self.L.ptr(best))
        return self.lib.cgs_ray_claims(*self._head(**kw), clear, best_p, self.L.raw_stream(DEV))

    def wins(self, best, out, window=1, margin=0, accumulate=0, **kw):
        best_p, out_p = kw.pop("best_ptr", self.L.ptr(best)), kw.pop("out_ptr", self.L.ptr(out))
        return self.lib.cgs_ray_wins(*self._head(**kw), best_p, window, margin, accumulate, out_p, self.L.raw_stream(DEV))


def _compare(bounds, dims, index, support, K, M, bits, H, W, windows=XC.WINDOWS, margins=XC.MARGINS):
    """best and wins of both back ends and of the raw calls into prefilled outputs, at every window and margin.  Returns the
    host's (best, {(window, margin): wins})."""
    want_best = SD.ray_claims(bounds, dims, index, support, K, M, bits, H, W, backend="host")
    bits_dev = bits.to(DEV)
    best = SD.ray_claims(bounds, dims, index, support, K, M, bits_dev, H, W, backend="gpu")
    assert best.is_cuda and best.dtype == torch.int32 and torch.equal(best.cpu(), want_best)
    raw = _Raw(bounds, dims, index, support, K, M, bits, H, W)
    raw_best = torch.full((len(K), H, W), SENTINEL, dtype=torch.int32, device=DEV)
    assert raw.claims(raw_best, clear=1) == 0 and torch.equal(raw_best.cpu(), want_best), "the clear reaches every pixel"
    assert raw.claims(raw_best, clear=0) == 0 and torch.equal(raw_best.cpu(), want_best), "claiming again changes nothing"
    all_wins = {}
    for window in windows:
        for margin in margins:
            want = SD.ray_wins(bounds, dims, index, support, K, M, bits, want_best, H, W, window=window, margin=margin,
                               backend="host")
            got = SD.ray_wins(bounds, dims, index, support, K, M, bits_dev, best, H, W, window=window, margin=margin,
                              backend="gpu")
            assert got.is_cuda and got.dtype == torch.uint16 and torch.equal(got.cpu(), want), (window, margin)
            out = _sentinel_words(len(index))
            assert raw.wins(raw_best, out, window, margin) == 0
            assert torch.equal(out.cpu(), want), ("every listed voxel's word is written", window, margin)
            all_wins[(window, margin)] = want
    return want_best, all_wins


@pytest.mark.parametrize("dims", SC.VOTE_GRIDS, ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("V", SC.VOTE_VIEWS)
def test_claims_and_wins_are_bit_identical_to_the_host(dims, V):
    K, M = SC.vote_cameras(V)
    bits = XC.vote_bits(V)
    for density in XC.DENSITIES:
        index, support = XC.random_list(dims, density)
        best, wins = _compare(SC.VOTE_BOUNDS, dims, index, support, K, M, bits, SC.MASK_H, SC.MASK_W)
        if dims[0] >= 63 and V >= 3 and density == 1.0:
            assert best.numpy().max() > 0 and wins[(0, 65535)].numpy().max() > 0, "the case must hold hits"
            assert not torch.equal(wins[(4, 0)], wins[(0, 65535)]), "and losses"
    empty = np.zeros(0, np.int32)
    best, wins = _compare(SC.VOTE_BOUNDS, dims, empty, empty.astype(np.uint16), K, M, bits, SC.MASK_H, SC.MASK_W, [1], [0])
    assert not best.numpy().any() and wins[(1, 0)].shape == (0,), "an empty list claims nothing"


@pytest.mark.parametrize("width", SC.BITS_WIDTHS)
def test_widths_around_the_word_boundaries(width):
    """Images of 1, 31, 32, 33 and 67 pixels a row: the near bit's word, the first and the last column, the window's clip."""
    bounds, dims, K, M, bits, index, support = XC.width_case(width)
    best, wins = _compare(bounds, dims, index, support, K, M, bits, XC.WIDTH_H, width)
    assert best.numpy()[:, 0, 0].min() > 0 and best.numpy()[:, -1, -1].min() > 0, "the corner pixels are claimed"
    assert wins[(0, 65535)].numpy().max() > 0


@pytest.mark.parametrize("count", XC.LIST_LENGTHS)
def test_list_lengths_and_partial_waves(count):
    dims, V = (257, 2, 1), 3
    K, M = SC.vote_cameras(V)
    index, support = XC.random_list(dims, 1.0)
    pick = np.sort(np.random.default_rng(count).permutation(index.size)[:count])
    _compare(SC.VOTE_BOUNDS, dims, index[pick], support[pick], K, M, XC.vote_bits(V), SC.MASK_H, SC.MASK_W, [1], [0])


def test_contention_on_one_pixel():
    """257 voxels, five waves in two blocks, on pixel (0, 0) of one view with distinct supports: best is the exact maximum
    and only its voxel wins."""
    K, M = XC.identity_camera()
    H, W = XC.HAND_H, XC.HAND_W
    bits = XC.ones_bits(1, H, W)
    index, support = np.arange(257, dtype=np.int32), XC.contention_support()
    best, wins = _compare(XC.CONTENTION_BOUNDS, XC.CONTENTION_DIMS, index, support, K, M, bits, H, W, [0, 4], [0, 6])
    assert best[0, 0, 0] == 1256 and best.sum() == 1256
    assert np.array_equal(wins[(0, 0)].numpy(), (support == 1256).astype(np.uint16)) and wins[(0, 0)].numpy().sum() == 1
    assert np.array_equal(wins[(4, 6)].numpy(), (support >= 1250).astype(np.uint16)) and wins[(4, 6)].numpy().sum() == 7


def test_accumulation_repeat_runs_and_a_reversed_list():
    dims, V = (65, 3, 2), 40
    K, M = SC.vote_cameras(V)
    bits = XC.vote_bits(V).to(DEV)
    index, support = XC.random_list(dims, 0.5)
    size = (SC.MASK_H, SC.MASK_W)
    run = lambda i, s: SD.ray_wins(SC.VOTE_BOUNDS, dims, i, s, K, M, bits,
                                   SD.ray_claims(SC.VOTE_BOUNDS, dims, i, s, K, M, bits, *size, backend="gpu"), *size,
                                   backend="gpu")
    one, again = run(index, support), run(index, support)
    assert torch.equal(one, again) and one.cpu().numpy().max() > 0
    back = run(index[::-1].copy(), support[::-1].copy())
    assert np.array_equal(back.cpu().numpy()[::-1], one.cpu().numpy()), "a voxel's wins do not depend on its thread"
    wins = None
    for v0 in range(0, V, 2):   # chunks of two views: best of the chunk, wins accumulated
        sl = slice(v0, v0 + 2)
        best = SD.ray_claims(SC.VOTE_BOUNDS, dims, index, support, K[sl], M[sl], bits[sl], *size, backend="gpu")
        first = wins
        wins = SD.ray_wins(SC.VOTE_BOUNDS, dims, index, support, K[sl], M[sl], bits[sl], best, *size, counts=wins, backend="gpu")
        assert first is None or wins is first
    assert torch.equal(wins, one)
    half = index.size // 2   # the list claimed in two pieces
    part = SD.ray_claims(SC.VOTE_BOUNDS, dims, index[:half], support[:half], K, M, bits, *size, backend="gpu")
    both = SD.ray_claims(SC.VOTE_BOUNDS, dims, index[half:], support[half:], K, M, bits, *size, best=part, backend="gpu")
    whole = SD.ray_claims(SC.VOTE_BOUNDS, dims, index, support, K, M, bits, *size, backend="gpu")
    assert both is part and torch.equal(both, whole)


def test_seed_points_exclusive_gpu_equals_host():
    for cases, bounds, cached, opts, (H, W) in [
            (DC.dir_novel_cameras(), DC.DIR_BOUNDS, XC.twelve_view_seeds, dict(DC.DIR_OPTIONS, directions=True), (DC.DIR_H, DC.DIR_W)),
            (SC.seed_novel_cameras(), SC.SEED_BOUNDS, XC.six_view_seeds, dict(SC.SEED_OPTIONS), (SC.SEED_H, SC.SEED_W))]:
        cams, maps = cases
        want, want_info = cached(True)
        got, info = SD.seed_points(cams, maps, "PidiNet", bounds, backend="gpu", device=DEV, exclusive=True, **opts)
        assert len(got) > 100 and got.dtype == np.float64 and np.array_equal(got, want)
        assert info["backend"] == "gpu" and XC.same_info(info, want_info)
        assert 0 < info["exclusive_voxels"] < info["kept_voxels"]
        budget = 2 * SD.BYTES_PER_PIXEL * H * W   # two views at a time in the first sweep, four in the second
        parts, info_p = SD.seed_points(cams, maps, "PidiNet", bounds, backend="gpu", device=DEV, exclusive=True,
                                       budget_bytes=budget, **opts)
        assert np.array_equal(parts, got) and XC.same_info(info_p, info)
        plain, plain_info = SD.seed_points(cams, maps, "PidiNet", bounds, backend="gpu", device=DEV, **opts)
        assert "exclusive_voxels" not in plain_info and XC.same_info(plain_info, cached(False)[1]) and len(plain) > len(got)


def test_scene_seeded_through_the_claims(tmp_path):
    """One curve per seed of the exclusive vote, and a finite, non-empty render."""
    from curve_gaussian_amd.edge_extraction.reprojection import scene_cameras
    from curve_gaussian_amd.gaussian_renderer import PipelineParams, render
    from curve_gaussian_amd.scene import GaussianCurveModel, Scene, default_seed_bounds
    scan = SC.write_seed_scan(tmp_path, "emap")
    gm = GaussianCurveModel(0, 12, device=DEV)
    options = dict(SC.SEED_OPTIONS, exclusive=True, excl_window=1)
    scene = Scene(scan, gm, device=DEV, init="edge_votes", init_options=options)
    cams, maps = scene_cameras(scene.getTrainCameras())
    want, info = SD.seed_points(cams, maps, "DexiNed", default_seed_bounds("emap", None), backend="host", **options)
    plain, _ = SD.seed_points(cams, maps, "DexiNed", default_seed_bounds("emap", None), backend="host", **SC.SEED_OPTIONS)
    cp = gm.get_curve_points.detach().double().cpu().numpy()
    assert 100 < info["seeds"] < len(plain) and cp.shape == (info["seeds"], 4, 3), "one curve per seed"
    assert np.array_equal(np.asarray(scene.point_cloud.points), want)
    gm.training_setup()
    with torch.no_grad():
        out = render(scene.getTrainCameras()[0], gm, PipelineParams(), torch.zeros(3, device=DEV))["render"]
    assert torch.isfinite(out).all() and out.abs().sum() > 0


def test_raw_argument_errors():
    bounds, dims = XC.hand_grid(1)
    K, M = XC.identity_camera()
    H, W = XC.HAND_H, XC.HAND_W
    raw = _Raw(bounds, dims, [0, 1, 2, 3], XC.HAND_SUPPORT, K, M, XC.ones_bits(1, H, W), H, W)
    best = torch.full((1, H, W), SENTINEL, dtype=torch.int32, device=DEV)
    out = _sentinel_words(4)
    nan, neg = (ctypes.c_double * 3)(0.0, float("nan"), 0.0), (ctypes.c_double * 3)(1.0, 1.0, -1.0)
    void = lambda a: ctypes.cast(a, ctypes.c_void_p)
    shared = [dict(M=-1), dict(V=-1), dict(V=65536), dict(nx=0), dict(ny=-1), dict(nz=0), dict(nx=65536, ny=65536, nz=1),
              dict(H=0), dict(W=16385), dict(lo=None), dict(step=None), dict(lo=void(nan)), dict(step=void(neg)),
              dict(index=None), dict(support=None), dict(intr=None), dict(w2c=None), dict(bits=None), dict(best_ptr=None)]
    for kw in shared:
        assert raw.claims(best, clear=1, **kw) == -1 and b"cgs_ray_claims: invalid argument" in raw.lib.cgs_last_error(), kw
        assert raw.wins(best, out, **kw) == -1 and b"cgs_ray_wins: invalid argument" in raw.lib.cgs_last_error(), kw
    for kw in [dict(window=-1), dict(window=5), dict(margin=-1), dict(margin=65536), dict(out_ptr=None)]:
        assert raw.wins(best, out, **kw) == -1 and b"cgs_ray_wins: invalid argument" in raw.lib.cgs_last_error(), kw
    torch.cuda.synchronize(DEV)
    untouched = lambda: (best.cpu().numpy() == SENTINEL).all() and (out.cpu().numpy() == SENTINEL).all()
    assert untouched(), "nothing was launched or cleared"
    for kw in [dict(M=0), dict(V=0)]:
        assert raw.claims(best, clear=0, **kw) == 0 and raw.wins(best, out, **kw) == 0
    assert untouched(), "no voxel or no view is a no-op"
    assert raw.claims(best, clear=1, M=0) == 0 and not best.cpu().numpy().any(), "apart from the requested clear"
    assert raw.claims(best, clear=0) == 0 and best.cpu().numpy()[0, 0, 0] == 30 and best.cpu().numpy().sum() == 30
    assert raw.wins(best, out) == 0 and out.cpu().tolist() == [0, 1, 1, 0]
    assert raw.wins(best, out, margin=10, accumulate=1) == 0 and out.cpu().tolist() == [0, 2, 2, 1]
