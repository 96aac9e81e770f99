"""The training-loss and Adam kernels against float64 references (tests/loss_ref64.py), at the shapes training runs at
and at the edges where the kernels' tiling, grids and hashing go wrong:

  fused SSIM (csrc/ssim.hip)            forward map and backward, tile-edge sizes, XCD tile-remap tails, 2048^2
  photometric loss (cgs_photometric_loss, ops.losses.photometric_loss)  clamp on / off, exact 0 and 1, edge-map extremes
  edge count / edge_aware_loss (csrc/loss.hip)
  curve regularisers (cgs_curve_regularizers)   B off the curves-per-block multiple, visibility extremes, device gate
  end-point connection loss (k_conn_*)  constructed geometry around the hash grid's cells
  flat Adam (k_adam_flat, k_adam_flat_dev)  3.2 M elements (second grid-stride trip), 16 segments, skip flag

Every bound is stated next to its assert.  Unless marked otherwise it comes from a rounding analysis of the kernel's
float32 arithmetic (eps = 2^-24 per rounding), not from measurement."""
import ctypes as C
import math
import struct
import types

import numpy as np
import pytest
import torch

import loss_ref64 as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = R.EPS32
THR32 = float(np.float32(0.1))


def _lib():
    from curve_gaussian_amd import _lib as L
    return L, L.load()


def _within(name, got, ref, bound):
    """|got - ref| <= bound elementwise (all float64 on one device); the message names the worst violation."""
    err = (got.double() - ref.double()).abs()
    bad = err > bound
    if bool(bad.any()):
        i = int(torch.argmax((err - bound).reshape(-1)))
        raise AssertionError(f"{name}: {int(bad.sum())} of {err.numel()} beyond the bound; worst at {i}: got "
                             f"{float(got.reshape(-1)[i]):.9g} ref {float(ref.reshape(-1)[i]):.9g} bound "
                             f"{float(bound.reshape(-1)[i]):.3g}")


# ---------------------------------------------------------------------------------------------------------------- SSIM
# 32 x 54 output tiles; T = tiles per plane.  T < 8 skips the XCD remap, T = 8q remaps every tile, T = 8q + r leaves a
# tail of r tiles in natural order.
SSIM_SHAPES = [(1, 1, 1, 1), (1, 1, 11, 11)] + [(1, 1, h, w) for w in (31, 32, 33, 65) for h in (53, 54, 55, 109)] + [
    (1, 1, 108, 64),      # T = 4
    (1, 1, 108, 128),     # T = 8
    (1, 1, 162, 160),     # T = 15 = 8 + 7
    (1, 1, 217, 289),     # T = 50 = 8 * 6 + 2, both sides off the tile edge
    (2, 3, 109, 65),
    (1, 1, 800, 800), (1, 1, 680, 1200), (1, 1, 1600, 1600), (1, 1, 2048, 2048)]


@pytest.mark.parametrize("shape", SSIM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fused_ssim_against_float64(shape):
    from curve_gaussian_amd.fused_ssim import FusedSSIMMap, SSIM_C1, SSIM_C2, fused_ssim
    g = torch.Generator(device=DEV).manual_seed(sum(shape) * 7 + shape[-1])
    a = torch.rand(*shape, generator=g, device=DEV)
    b = torch.rand(*shape, generator=g, device=DEV)
    dmap = torch.randn(*shape, generator=g, device=DEV)
    x = a.clone().requires_grad_(True)
    m = FusedSSIMMap.apply(SSIM_C1, SSIM_C2, x, b, "same", True)
    m.backward(dmap)
    ref_map = R.ssim_parts64(a, b)["map"]
    ref_grad = R.ssim_vjp64(a, b, dmap)
    map_bound, grad_bound = R.ssim_error_bounds(a, b, dmap)
    # per pixel: the first-order rounding bound of ssim_error_bounds (K = 64, derivation in its docstring)
    _within("ssim map", m.detach(), ref_map, map_bound)
    _within("ssim d/d img1", x.grad, ref_grad, grad_bound + 1e-30)
    # the mean (what fused_ssim returns): bound averaged, plus torch's float32 reduction (<= log2 N roundings)
    N = a.numel()
    val = fused_ssim(a, b)
    tol = float(map_bound.mean()) + math.ceil(math.log2(N) + 1) * EPS * float(ref_map.abs().mean())
    assert abs(float(val) - float(ref_map.mean())) <= tol


@pytest.mark.parametrize("shape", [(1, 1, 11, 11), (1, 1, 12, 30), (2, 3, 55, 33), (1, 1, 217, 289), (1, 1, 800, 800)],
                         ids=lambda s: "x".join(map(str, s)))
def test_fused_ssim_valid_padding_against_float64(shape):
    from curve_gaussian_amd.fused_ssim import fused_ssim
    g = torch.Generator(device=DEV).manual_seed(shape[-1])
    a = torch.rand(*shape, generator=g, device=DEV)
    b = torch.rand(*shape, generator=g, device=DEV)
    x = a.clone().requires_grad_(True)
    val = fused_ssim(x, b, padding="valid")
    val.backward()
    ref_m, ref_mean, ref_grad = R.ssim64(a, b, "valid")
    Nv = ref_m.numel()
    dmap = torch.zeros_like(a, dtype=torch.float64)
    dmap[..., 5:-5, 5:-5] = 1.0 / Nv
    map_bound, grad_bound = R.ssim_error_bounds(a, b, dmap)
    # same bounds as the "same" test, restricted to the cropped map
    tol = float(map_bound[..., 5:-5, 5:-5].mean()) + math.ceil(math.log2(Nv) + 1) * EPS * float(ref_m.abs().mean())
    assert abs(float(val) - float(ref_mean)) <= tol
    _within("ssim valid d/d img1", x.grad, ref_grad, grad_bound + 1e-30)


@pytest.mark.parametrize("hw", [(1, 1), (5, 7), (10, 10), (10, 40)])
def test_fused_ssim_valid_padding_on_tiny_images_is_the_empty_crop(hw):
    """<= 10 px: the reference's crop [5:-5] is empty, its mean NaN and the gradient zero; the drop-in does the same."""
    from curve_gaussian_amd.fused_ssim import fused_ssim
    a = torch.rand(1, 1, *hw, device=DEV)
    x = a.clone().requires_grad_(True)
    val = fused_ssim(x, torch.rand(1, 1, *hw, device=DEV), padding="valid")
    _, ref_mean, _ = R.ssim64(a, a, "valid")
    assert math.isnan(float(val)) and math.isnan(float(ref_mean))
    val.backward()
    assert x.grad is not None and not bool(x.grad.any())


# ------------------------------------------------------------------------------------------------- photometric loss
PHOTO_SHAPES = [(1, 1), (11, 11), (53, 31), (54, 33), (55, 65), (109, 32), (108, 64), (108, 128), (162, 160), (217, 289)]
PHOTO_LARGE = [(800, 800), (680, 1200), (1600, 1600), (2048, 2048)]


def _photo_inputs(H, W, gt_kind, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    img = torch.rand(1, H, W, generator=g, device=DEV) * 1.4 - 0.2           # about 14 % outside [0, 1] each side
    u = torch.rand(1, H, W, generator=g, device=DEV)
    img = torch.where(u < 0.02, torch.zeros_like(img), torch.where(u > 0.98, torch.ones_like(img), img))
    if gt_kind == "sparse":
        gt = (torch.rand(1, H, W, generator=g, device=DEV) > 0.85).float() * torch.rand(1, H, W, generator=g, device=DEV)
    elif gt_kind == "none":                                                  # n_pos = 0
        gt = torch.rand(1, H, W, generator=g, device=DEV) * 0.09
    elif gt_kind == "all":                                                   # n_pos = N
        gt = 0.11 + 0.89 * torch.rand(1, H, W, generator=g, device=DEV)
    else:                                                                    # values == float32(threshold): not edges
        v = torch.rand(1, H, W, generator=g, device=DEV)
        gt = torch.where(v < 0.5, torch.full_like(v, THR32), v)
    # where the render sits exactly on a clamp bound the gt differs, so the gradient there is not zero
    gt = torch.where((img == 0) & (gt == 0), torch.full_like(gt, 0.5), gt)
    gt = torch.where((img == 1) & (gt == 1), torch.full_like(gt, 0.5), gt)
    return img, gt


def _photo_bounds(img, gt, a, b, clamp):
    """Bounds on the fused kernel's value and d loss / d image (derivation: the SSIM part as in ssim_error_bounds with
    the constant dL/dmap = -b/N; the edge part's terms d^2 w and 2 a d w / N carry <= 4 roundings each and are summed in
    float32 per 512-thread block (<= 9 levels), in float64 across blocks: <= 16 eps of the sum of their magnitudes)."""
    x = img.double().clamp(0, 1) if clamp else img.double()
    N = x.numel()
    _, w, _ = R.edge_weights64(gt)
    d = x - gt.double()
    map_bound, grad_bound = R.ssim_error_bounds(x.unsqueeze(0), gt.unsqueeze(0), torch.full_like(x, b / N).unsqueeze(0))
    ref_map = R.ssim_parts64(x.unsqueeze(0), gt.double().unsqueeze(0))["map"]
    v_bound = (a * 16 * EPS * float((d * d * w).mean()) + b * (float(map_bound.mean()) + 16 * EPS * float(ref_map.abs().mean())))
    g_edge = (2 * a / N * d * w).abs()
    g_bound = grad_bound[0] + 8 * EPS * g_edge
    return v_bound, g_bound


def _check_photo(img, gt, clamp, val, grad, a=9.0, b=1.0):
    ref_v, ref_g = R.photometric64(img, gt, a, b, clamp=clamp)
    v_bound, g_bound = _photo_bounds(img, gt, a, b, clamp)
    assert abs(float(val) - float(ref_v)) <= v_bound + 2 * EPS * abs(float(ref_v)), (float(val), float(ref_v), v_bound)
    _within("photometric d/d image", grad, ref_g, g_bound + 4 * EPS * ref_g.abs() + 1e-30)
    if clamp:   # the clamp's mask is inclusive: exactly zero outside [0, 1], live on the bounds
        out = (img < 0) | (img > 1)
        assert not bool(grad[out].any())
        on = (img == 0) | (img == 1)
        if bool(on.any()):
            assert bool((grad[on] != 0).all())


@pytest.mark.parametrize("gt_kind", ["sparse", "none", "all", "at_threshold"])
@pytest.mark.parametrize("clamp", [False, True])
def test_photometric_loss_against_float64(clamp, gt_kind):
    from curve_gaussian_amd.ops.losses import edge_pixel_count, photometric_loss
    for i, (H, W) in enumerate(PHOTO_SHAPES):
        img, gt = _photo_inputs(H, W, gt_kind, 100 * i + len(gt_kind))
        n_ref = R.edge_weights64(gt)[2]
        assert int(edge_pixel_count(gt)) == n_ref
        if gt_kind == "none":
            assert n_ref == 0
        if gt_kind == "all":
            assert n_ref == H * W
        x = img.clone().requires_grad_(True)
        val = photometric_loss(x, gt, 10.0, 0.1, clamp=clamp)      # a = 9, b = 1
        val.backward()
        _check_photo(img, gt, clamp, val, x.grad)


@pytest.mark.parametrize("hw", PHOTO_LARGE, ids=lambda s: "x".join(map(str, s)))
def test_photometric_loss_at_training_resolutions(hw):
    from curve_gaussian_amd.ops.losses import photometric_loss
    for clamp in (False, True):
        img, gt = _photo_inputs(*hw, "sparse", hw[1] + clamp)
        x = img.clone().requires_grad_(True)
        val = photometric_loss(x, gt, 10.0, 0.1, clamp=clamp)
        val.backward()
        _check_photo(img, gt, clamp, val, x.grad)


def test_photometric_workspace_reused_across_image_sizes():
    """One zero-filled workspace, sized for the largest image, serves every smaller H x W in turn (the slots the value
    is reduced into sit at a fixed offset and are left zero by each call): same value and gradient as a fresh one."""
    from curve_gaussian_amd.ops.losses import edge_pixel_count
    L, lib = _lib()
    sizes = [(217, 289), (55, 65), (108, 128), (11, 11), (217, 289), (1, 1), (54, 33)]
    ws = torch.zeros(int(lib.cgs_photometric_workspace_bytes(217, 289)), dtype=torch.uint8, device=DEV)
    s = L.raw_stream(torch.device(DEV))
    for i, (H, W) in enumerate(sizes):
        img, gt = _photo_inputs(H, W, "sparse", 7 + i)
        n_pos = edge_pixel_count(gt)
        out = []
        for w in (ws, torch.zeros(int(lib.cgs_photometric_workspace_bytes(H, W)), dtype=torch.uint8, device=DEV)):
            grad = torch.empty_like(img)
            loss = torch.empty((), device=DEV)
            L.check(lib.cgs_photometric_loss(H, W, L.ptr(img), L.ptr(gt), C.c_float(0.1), L.ptr(n_pos), C.c_float(9.0),
                                             C.c_float(1.0), 1, L.ptr(w), L.ptr(grad), L.ptr(loss), s), "photometric_loss")
            out.append((loss, grad))
        assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]), (H, W)
        _check_photo(img, gt, True, out[0][0], out[0][1])


def test_photometric_loss_half_precision_render():
    """A float16 render gets a float16 gradient: the float32 one rounded (half a float16 ulp, or half the subnormal
    spacing 2^-24 below 2^-14)."""
    from curve_gaussian_amd.ops.losses import photometric_loss
    img, gt = _photo_inputs(40, 50, "sparse", 3)
    h = img.half().requires_grad_(True)
    f = h.detach().float().requires_grad_(True)
    vh = photometric_loss(h, gt, 10.0, 0.1, clamp=True)
    vf = photometric_loss(f, gt, 10.0, 0.1, clamp=True)
    vh.backward()
    vf.backward()
    assert h.grad.dtype == torch.float16
    assert float(vh) == float(vf)
    g32 = f.grad.double()
    assert bool(((h.grad.double() - g32).abs() <= 2.0 ** -11 * g32.abs() + 2.0 ** -25).all())


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs")
def test_photometric_loss_on_a_non_current_device():
    from curve_gaussian_amd.ops.losses import photometric_loss
    img, gt = _photo_inputs(70, 93, "sparse", 5)
    res = []
    for dev in ("cuda:0", "cuda:1"):
        x = img.to(dev).requires_grad_(True)
        val = photometric_loss(x, gt.to(dev), 10.0, 0.1, clamp=True)
        val.backward()
        res.append((val.detach().cpu(), x.grad.cpu()))
    assert torch.cuda.current_device() == 0
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


# ---------------------------------------------------------------------------------------- edge count / edge-aware loss
def test_edge_count_is_exact_at_2048():
    L, lib = _lib()
    g = torch.Generator(device=DEV).manual_seed(1)
    gt = torch.rand(1, 2048, 2048, generator=g, device=DEV) * 0.2
    gt.view(-1)[::7] = THR32                                              # equal to the threshold: not an edge
    gt.view(-1)[3::11] = float(np.nextafter(np.float32(THR32), np.float32(1)))   # one ulp above: an edge
    n = torch.empty(1, dtype=torch.int32, device=DEV)
    L.check(lib.cgs_edge_count(1, 2048, 2048, L.ptr(gt), C.c_float(0.1), L.ptr(n), L.raw_stream(torch.device(DEV))),
            "edge_count")
    assert int(n) == int((gt.double() > THR32).sum()) == R.edge_weights64(gt)[2]


@pytest.mark.parametrize("hw", [(37, 53), (680, 1200)])
def test_edge_aware_loss_three_channels_against_float64(hw):
    from curve_gaussian_amd.ops.losses import edge_aware_loss
    g = torch.Generator(device=DEV).manual_seed(hw[0])
    img = torch.rand(3, *hw, generator=g, device=DEV)
    gt = (torch.rand(3, *hw, generator=g, device=DEV) > 0.7).float() * torch.rand(3, *hw, generator=g, device=DEV)
    x = img.clone().requires_grad_(True)
    val = edge_aware_loss(x, gt)
    val.backward()
    ref_v, ref_g = R.edge_aware_loss64(img, gt)
    # terms d^2 w: <= 4 roundings each, summed in float64; the mean's division and the float32 result: 2 more
    assert abs(float(val) - float(ref_v)) <= 6 * EPS * float(ref_v)
    # 2 / (C N) * d * w: d 1, w 2, the scale 1, the two products 2 roundings
    _within("edge_aware_loss d/d image", x.grad, ref_g, 6 * EPS * ref_g.abs())


# ------------------------------------------------------------------------------------------------- curve regularisers
M = 12
CPB = 256 // M          # k_reg_main's curves_per_block


def _reg_inputs(B, vis, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    rot = torch.randn(B * M, 4, generator=g, device=DEV)
    op = torch.randn(B, 1, generator=g, device=DEV) * 2
    wl = math.log(0.005) + torch.randn(B, 1, generator=g, device=DEV)    # about half the curves above the threshold
    if vis == "random":
        radii = (torch.rand(B * M, generator=g, device=DEV) > 0.5).to(torch.int32) * 3
    elif vis == "one":
        radii = torch.zeros(B * M, dtype=torch.int32, device=DEV)
        radii[(B * M) // 2 + 1] = 2
    elif vis == "none":
        radii = torch.zeros(B * M, dtype=torch.int32, device=DEV)
    else:
        radii = torch.ones(B * M, dtype=torch.int32, device=DEV)
    return rot, op, wl, radii


@pytest.mark.parametrize("B", [1, CPB - 1, CPB + 1, 20000])
@pytest.mark.parametrize("vis", ["random", "one", "none", "all"])
def test_curve_regularizers_against_float64(B, vis):
    from curve_gaussian_amd.ops import regularizers as RG
    rot, op, wl, radii = _reg_inputs(B, vis, B + len(vis))
    for gate in (1.0, torch.ones((), device=DEV), 0.0, torch.zeros((), device=DEV), 0.5):
        leaves = [t.clone().requires_grad_(True) for t in (rot, op, wl)]
        gm = types.SimpleNamespace(_rotation=leaves[0], _opacity=leaves[1], _width=leaves[2], n_gaussians=M)
        val = RG.curve_regularizers(gm, radii, 0.01, gate, 0.1, 0.01)
        val.backward()
        ref = R.regularizers64(rot, op, wl, radii, M, 0.01, float(gate), 0.1, 0.01)
        # value: every term has <= ~16 roundings (expf / logf / sigmoid <= 2 ulp each, the cosine's products and
        # division); 1 - |cos| is bounded by 1 in magnitude and the terms are summed in float32 per block of 256 (8
        # levels), in float64 after: <= 32 eps of the summed magnitudes (w_op gate log 3, w_smo, w_w max width)
        scale = 0.01 * abs(float(gate)) * math.log(3) + 0.1 + 0.01 * float(torch.exp(wl).max())
        assert abs(float(val) - float(ref[0])) <= 32 * EPS * scale, (float(val), float(ref[0]))
        # gradients: the quaternion -> axis -> cosine chain is ~40 roundings of terms no larger than the tensor's largest
        # entry; 256 eps of that entry bounds it with room
        for name, leaf, r in zip(("rotation", "opacity", "width"), leaves, ref[1:]):
            _within(f"regularizer d/d {name} (B={B}, {vis}, gate={float(gate)})", leaf.grad, r,
                    torch.full_like(r, 256 * EPS * float(r.abs().max()) + 1e-30))
        if vis == "none":   # only the width term is left, whatever the gate
            assert not bool(leaves[0].grad.any()) and not bool(leaves[1].grad.any())


# ----------------------------------------------------------------------------------------------- connection loss
THR = 0.05
CELL = float(np.float32(THR) * np.float32(1.0001))


def _conn_check(cp, what, weight=0.1):
    """HIP value and gradient against connection64 (float64 brute force).  Bounds: each distance has <= 4 roundings;
    a point's sums run over its <= deg partners in float32 (deg roundings), the block sums add <= 10 levels:
    (deg + 16) eps relative for the positive sum of distances, (deg + 16) eps of the deg unit vectors for a gradient.
    An ordered pair within 4 ulp of the threshold may be counted either way: `amb` of them move the mean by at most
    amb (thr + mean) / (count - amb) and a gradient entry by amb 2 w / (count - amb) times (1 + deg)."""
    from curve_gaussian_amd.ops import regularizers as RG
    leaf = cp.clone().requires_grad_(True)
    val = RG.connection_loss(types.SimpleNamespace(_curve_points=leaf), weight, THR)
    val.backward()
    ref_v, ref_g, count, amb, deg = R.connection64(cp, THR, weight, chunk=1024)
    if count == 0:
        assert float(val) == 0.0 and not bool(leaf.grad.any()), what
        return 0
    flip_v = amb * weight * (THR + ref_v / weight) / max(count - amb, 1)
    v_bound = (deg + 16) * EPS * ref_v + flip_v
    assert abs(float(val) - ref_v) <= v_bound, (what, float(val), ref_v, count, amb)
    unit = 2 * weight / count
    g_bound = (deg + 16) * EPS * unit * deg + amb * 2 * weight / max(count - amb, 1) * (1 + deg)
    _within(what, leaf.grad, ref_g, torch.full_like(ref_g, g_bound))
    assert not bool(leaf.grad[:, 1:3].any())
    return count


def _pair_curves(pairs, far):
    """curve k: start = pairs[k][0]; curve k + n: end = pairs[k][1]; every other end point at its own far location."""
    n = len(pairs)
    cp = torch.zeros(2 * n, 4, 3, dtype=torch.float64)
    for k, (p, q) in enumerate(pairs):
        cp[k, 0] = torch.tensor(p)
        cp[n + k, 3] = torch.tensor(q)
        cp[k, 3] = torch.tensor([far + 4 * THR * k, far, far])
        cp[n + k, 0] = torch.tensor([far + 4 * THR * k, far + 1.0, far])
    cp[:, 1:3] = 0.5 * (cp[:, :1] + cp[:, 3:])
    return cp.float().to(DEV)


@pytest.mark.parametrize("origin", [0.0, -1000.0, 1000.0])
def test_connection_loss_across_every_neighbour_cell(origin):
    """Partners in each of the 26 neighbouring cells: the first point sits just inside its cell next to the shared face,
    edge or corner, the partner just across it, so only one of the 27 cells visited holds it.  Near the origin the cells
    straddle 0 (floorf vs the int cast); at +-1000 the float32 coordinates are 1/800 of a cell apart."""
    r = THR * (1 - 1e-3) if origin == 0.0 else THR * 0.98     # at |x| = 1000 one float32 ulp is 6e-5: keep a margin
    pairs = []
    d_list = [d for d in ((dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)) if d != (0, 0, 0)]
    for k, d in enumerate(d_list):
        nd = math.sqrt(sum(c * c for c in d))
        base = math.floor(origin / CELL) + 6 * (k - 13)        # cells of different pairs are >= 3 apart
        p, q = [], []
        for axis, c in enumerate(d):
            cell = base if axis == 0 else math.floor(origin / CELL)
            lo, hi = cell * CELL, (cell + 1) * CELL
            if c == 0:
                p.append((lo + hi) / 2)
            else:
                edge = hi if c > 0 else lo
                p.append(edge - c * 0.3 * r / nd)
            q.append(p[-1] + c * r / nd)
        pairs.append((p, q))
    cp = _pair_curves(pairs, origin + 500.0)
    count = _conn_check(cp, f"26 directions @ {origin}")
    assert count == 2 * 26                                   # every planted pair, in both orders, nothing else
    # partners really sit in the neighbouring cell the direction names (as the kernel computes cells)
    inv = np.float32(1.0) / np.float32(CELL)
    for k, (p, q) in enumerate(pairs):
        cpk = np.floor(np.float32(cp[k, 0].cpu().numpy()) * inv)
        cqk = np.floor(np.float32(cp[26 + k, 3].cpu().numpy()) * inv)
        assert np.count_nonzero(cpk != cqk) == sum(c != 0 for c in d_list[k]) and np.abs(cpk - cqk).max() == 1


def test_connection_loss_planted_pairs_at_the_threshold():
    inside, outside = THR * (1 - 1e-3), THR * (1 + 1e-3)
    pairs = []
    for k in range(40):
        x = -1.0 + 0.3 * k
        pairs.append(([x, 0.2, -0.1], [x + (inside if k % 2 == 0 else outside), 0.2, -0.1]))
    cp = _pair_curves(pairs, 300.0)
    assert _conn_check(cp, "thr (1 -+ 1e-3)") == 2 * 20


@pytest.mark.parametrize("case", ["centred", "minus1000", "plus1000", "dense_cell", "collisions", "coincident_closed"])
def test_connection_loss_constructed_clouds(case):
    g = torch.Generator().manual_seed(len(case))
    if case in ("centred", "minus1000", "plus1000"):
        B = 3000
        c = {"centred": 0.0, "minus1000": -1000.0, "plus1000": 1000.0}[case]
        cp = (torch.rand(B, 4, 3, generator=g, dtype=torch.float64) - 0.5) * 0.8 + c
    elif case == "dense_cell":                          # every end point in one grid cell: one long list per query
        B = 300
        cp = torch.rand(B, 4, 3, generator=g, dtype=torch.float64) * 0.3 * THR + 2 * CELL + 0.1 * THR
    elif case == "collisions":                          # 1200 points over ~10^4 cells, 4096 hash buckets
        B = 600
        cp = torch.rand(B, 4, 3, generator=g, dtype=torch.float64) * 22 * CELL - 11 * CELL
    else:
        B = 500
        cp = torch.rand(B, 4, 3, generator=g, dtype=torch.float64) * 0.4
        cp[10:20, 0] = cp[30:40, 3]                      # coincident end points of different curves
        cp[50:60, 3] = cp[50:60, 0]                      # closed curves: same-curve pairs excluded
        cp[70, 0] = cp[71, 0] = cp[72, 3]                # three end points at one place
    n = _conn_check(cp.float().to(DEV), case)
    assert n > 0
    if case == "dense_cell":
        assert n == 2 * B * (2 * B - 1) - 2 * B          # all ordered pairs but each curve's own start-end pair


def test_connection_loss_accumulate_into_a_gradient_buffer():
    L, lib = _lib()
    g = torch.Generator().manual_seed(2)
    B = 900
    cp = (torch.rand(B, 4, 3, generator=g) * 0.5).to(DEV)
    g0 = torch.randn(B, 4, 3, generator=g).to(DEV)
    s = L.raw_stream(torch.device(DEV))
    ws = torch.empty(int(lib.cgs_endpoint_connection_workspace_bytes(B)), dtype=torch.uint8, device=DEV)
    loss = torch.empty((), device=DEV)
    fresh = torch.full_like(g0, float("nan"))
    acc = g0.clone()
    for out, accumulate in ((fresh, 0), (acc, 1)):
        L.check(lib.cgs_endpoint_connection_loss(B, L.ptr(cp), C.c_float(THR), C.c_float(0.1), L.ptr(ws), L.ptr(loss),
                                                 L.ptr(out), accumulate, s), "endpoint_connection_loss")
    assert not bool(fresh[:, 1:3].any())
    assert torch.equal(acc[:, 1:3], g0[:, 1:3])                      # rows 1, 2 untouched
    # the per-point sums are float atomics (their order varies from call to call): the two calls' gradients agree within
    # the connection bound of _conn_check, the addition itself is one rounding of the sum
    _, ref_g, count, _, deg = R.connection64(cp, THR, 0.1)
    tol = 2 * (deg + 16) * EPS * (0.2 / count) * deg + EPS * (g0 + fresh).abs()
    _within("accumulate", acc[:, [0, 3]], g0[:, [0, 3]] + fresh[:, [0, 3]], tol[:, [0, 3]])
    _within("accumulate = 0", fresh, ref_g, torch.full_like(ref_g, (deg + 16) * EPS * (0.2 / count) * deg))


def test_connection_loss_at_100k_curves():
    """B = 100 000 (200 000 end points, ~4 partners each) in a box across the origin; reference: float64 brute force over
    all 4 * 10^10 ordered pairs (an algorithm independent of the hash grid), 1024 rows at a time."""
    g = torch.Generator(device=DEV).manual_seed(100)
    cp = (torch.rand(100000, 4, 3, generator=g, device=DEV) - 0.5) * 3.0
    assert _conn_check(cp, "B = 100000") > 100000


def test_connection_grid_coordinate_bound():
    """curvegs.h: end points must stay within |x| < 2^30 thr.  Up to 2^20 thr (a 52 km scene at the reference's 5 cm)
    the neighbour search is still exact: pairs there are found like anywhere else."""
    far = float(2 ** 20) * THR
    # one pair 0.6 thr apart (a float32 ulp there is 0.004 = thr / 13)
    pairs = [([far + 0.5, 3.0, -far], [far + 0.5 + 0.6 * THR, 3.0, -far])]
    cp = _pair_curves(pairs + [([0.0, 0.0, 0.0], [5.0, 5.0, 5.0])], 900.0)
    assert _conn_check(cp, "far") == 2


# ------------------------------------------------------------------------------------------------------- flat Adam
NADAM = 3_200_003
BETAS32 = (float(np.float32(0.9)), float(np.float32(0.999)))   # the kernel receives float betas


def _adam_segments():
    begins = [0, 1, 12_347, 12_348, 12_348, 600_001, 1_048_577, 1_048_833, 1_500_011, 2_000_003, 2_100_001, 2_500_009,
              2_800_001, 3_000_019, 3_100_007, 3_199_999]
    assert len(begins) == 16 and begins == sorted(begins)
    lens = [b - a for a, b in zip(begins, begins[1:] + [NADAM])]
    assert 0 in lens and 1 in lens
    lrs = [float(np.float32(1e-3 * 1.7 ** (s % 7) * (1 if s % 2 else 0.31))) for s in range(16)]
    return begins, lrs


def _pack(begins, lrs):
    return b"".join(struct.pack("<qff", b, lr, 0.0) for b, lr in zip(begins, lrs))


def _lr_per_element(begins, lrs, n):
    lr = torch.empty(n, dtype=torch.float64, device=DEV)
    for s, b in enumerate(begins):
        e = begins[s + 1] if s + 1 < len(begins) else n
        lr[b:e] = lrs[s]
    return lr


def _adam_grads(step):
    g = torch.Generator(device=DEV).manual_seed(50 + step)
    mag = 10.0 ** (torch.rand(NADAM, generator=g, device=DEV) * 11 - 8)            # 1e-8 .. 1e3
    return torch.randn(NADAM, generator=g, device=DEV) * mag


def test_flat_adam_against_float64_and_torch():
    """5 steps over 3.2 M elements (past the 2048 x 256 grid: the grid-stride loop's second trip), 16 segments with odd
    boundaries and segments of length 0 and 1, a learning-rate change at step 4, gradients from 1e-8 to 1e3."""
    L, lib = _lib()
    b1, b2 = BETAS32
    eps = 1e-15
    begins, lrs = _adam_segments()
    g0 = torch.Generator(device=DEV).manual_seed(0)
    p = torch.randn(NADAM, generator=g0, device=DEV)
    m, v, grad = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
    p64, m64, v64 = p.double(), torch.zeros_like(p, dtype=torch.float64), torch.zeros_like(p, dtype=torch.float64)
    budget = torch.zeros_like(p64)
    mabs = torch.zeros_like(p64)
    # torch.optim.Adam in float32 on the GPU, one group per segment, the same float betas and learning rates
    tp = p.clone()
    groups = []
    for s, b in enumerate(begins):
        e = begins[s + 1] if s + 1 < 16 else NADAM
        groups.append({"params": [torch.nn.Parameter(tp[b:e].clone())], "lr": lrs[s]})
    opt = torch.optim.Adam(groups, betas=(b1, b2), eps=eps)
    s = L.raw_stream(torch.device(DEV))
    for step in range(1, 6):
        if step == 4:
            lrs = [lr if k % 3 else float(np.float32(lr * 0.25)) for k, lr in enumerate(lrs)]
            for grp, lr in zip(opt.param_groups, lrs):
                grp["lr"] = lr
        gr = _adam_grads(step)
        grad.copy_(gr)
        L.check(lib.cgs_adam_step_flat(NADAM, L.ptr(p), L.ptr(grad), L.ptr(m), L.ptr(v), _pack(begins, lrs), 16,
                                       C.c_float(b1), C.c_float(b2), C.c_float(eps), step, step % 2, s), "adam_step_flat")
        assert (float(grad.abs().max()) == 0.0) == (step % 2 == 1)       # zero_grad folded in
        for grp, (b, e) in zip(opt.param_groups, zip(begins, begins[1:] + [NADAM])):
            grp["params"][0].grad = gr[b:e].clone()
        opt.step()
        lr = _lr_per_element(begins, lrs, NADAM)
        p64, m64, v64 = R.adam64_step(p64, gr, m64, v64, step, lr, b1, b2, eps)
        # budget: the update lr/bc1 * m / (sqrt(v / bc2) + eps) has <= 3 roundings per step in m (relative to
        # mabs = b1 mabs + (1 - b1) |g|, the magnitude of the terms m sums), <= 3 per step in v (non-negative terms), 4 in
        # the square root, divisions and the step size; 16 t covers t steps of accumulated state error.  Each new p adds one
        # rounding of |p|.
        mabs = b1 * mabs + (1 - b1) * gr.double().abs()
        den = (v64 / (1 - b2 ** step)).sqrt() + eps
        budget = budget + EPS * p64.abs() + 16 * step * EPS * (lr / (1 - b1 ** step)) * mabs / den
        _within(f"flat Adam p (step {step})", p, p64, budget)
    _within("flat Adam exp_avg", m, m64, 16 * 5 * EPS * mabs)
    _within("flat Adam exp_avg_sq", v, v64, 16 * 5 * EPS * v64)
    # torch's float32 Adam: also within the budget of the exact value, so within twice the budget of the kernel.  Not bit
    # for bit: torch rounds v * b2 in its own kernel before addcmul (the kernel contracts it into one fma) and takes lr /
    # bc1 in float64, the kernel in float32.
    tp = torch.cat([grp["params"][0].detach() for grp in opt.param_groups])
    _within("flat Adam vs torch.optim.Adam", p, tp, 2 * budget)


def _dev_state(begins, lrs, step, b1, b2):
    """cgs_adam_state_bytes() bytes: 16 x {int64 begin, float lr, float pad}, bc1, sqrt(bc2), 2 floats of padding --
    the scalars computed as cgs_adam_step_flat computes them (double, then rounded to float)."""
    bc1 = 1.0 - float(np.float64(np.float32(b1))) ** step
    sbc2 = math.sqrt(1.0 - float(np.float64(np.float32(b2))) ** step)
    blob = _pack(begins, lrs)
    blob += b"\0" * (16 * 16 - len(blob)) + struct.pack("<ffff", bc1, sbc2, 0.0, 0.0)
    return torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(DEV)


def test_flat_adam_dev_equals_host_table_and_honours_the_skip_flag():
    L, lib = _lib()
    assert int(lib.cgs_adam_state_bytes()) == 16 * 16 + 16
    b1, b2 = BETAS32
    begins, lrs = _adam_segments()
    s = L.raw_stream(torch.device(DEV))
    g0 = torch.Generator(device=DEV).manual_seed(1)
    A = [torch.randn(NADAM, generator=g0, device=DEV), torch.zeros(NADAM, device=DEV), torch.zeros(NADAM, device=DEV)]
    Bst = [t.clone() for t in A]
    ga, gb = torch.empty(NADAM, device=DEV), torch.empty(NADAM, device=DEV)
    for step in range(1, 6):
        gr = _adam_grads(step)
        ga.copy_(gr)
        gb.copy_(gr)
        L.check(lib.cgs_adam_step_flat(NADAM, L.ptr(A[0]), L.ptr(ga), L.ptr(A[1]), L.ptr(A[2]), _pack(begins, lrs), 16,
                                       C.c_float(b1), C.c_float(b2), C.c_float(1e-15), step, 1, s), "adam_step_flat")
        st = _dev_state(begins, lrs, step, b1, b2)
        L.check(lib.cgs_adam_step_flat_dev(NADAM, L.ptr(Bst[0]), L.ptr(gb), L.ptr(Bst[1]), L.ptr(Bst[2]), L.ptr(st), 16,
                                           C.c_float(b1), C.c_float(b2), C.c_float(1e-15), 1, None, s), "adam_step_flat_dev")
        for x, y in zip(A, Bst):
            assert torch.equal(x, y), step
        assert not bool(gb.any())
    # skip flag set: parameters and moments untouched, gradients cleared, the report ring records the skip
    seq = torch.zeros(1, dtype=torch.int32, device=DEV)
    ring = torch.full((4,), 7, dtype=torch.int32, device=DEV)
    flag = torch.ones(1, dtype=torch.int32, device=DEV)
    before = [t.clone() for t in Bst]
    gb.copy_(_adam_grads(9))
    st = _dev_state(begins, lrs, 6, b1, b2)
    args = (NADAM, L.ptr(Bst[0]), L.ptr(gb), L.ptr(Bst[1]), L.ptr(Bst[2]), L.ptr(st), 16, C.c_float(b1), C.c_float(b2),
            C.c_float(1e-15), 1)
    L.check(lib.cgs_adam_step_flat_dev_report(*args, L.ptr(flag), L.ptr(seq), L.ptr(ring), 4, s), "report")
    for x, y in zip(Bst, before):
        assert torch.equal(x, y)
    assert not bool(gb.any())
    assert int(seq) == 1 and ring.tolist() == [1, 7, 7, 7]
    flag.zero_()
    gb.copy_(_adam_grads(9))
    L.check(lib.cgs_adam_step_flat_dev_report(*args, L.ptr(flag), L.ptr(seq), L.ptr(ring), 4, s), "report")
    assert int(seq) == 2 and ring.tolist() == [1, 0, 7, 7]
    assert not torch.equal(Bst[0], before[0])


def test_flat_adam_argument_limits():
    L, lib = _lib()
    begins, lrs = _adam_segments()
    p = torch.randn(100, device=DEV)
    keep = p.clone()
    g, m, v = torch.ones_like(p), torch.zeros_like(p), torch.zeros_like(p)
    s = L.raw_stream(torch.device(DEV))
    segs17 = _pack(begins + [99], lrs + [1e-3])
    rc = lib.cgs_adam_step_flat(100, L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), segs17, 17, C.c_float(0.9),
                                C.c_float(0.999), C.c_float(1e-15), 1, 0, s)
    assert rc == -1                                                   # CGS_ERR_INVALID_ARGUMENT, nothing launched
    st = torch.zeros(int(lib.cgs_adam_state_bytes()), dtype=torch.uint8, device=DEV)
    rc = lib.cgs_adam_step_flat_dev(100, L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), L.ptr(st), 17, C.c_float(0.9),
                                    C.c_float(0.999), C.c_float(1e-15), 0, None, s)
    assert rc == -1
    rc = lib.cgs_adam_step_flat(0, L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), _pack(begins, lrs), 16, C.c_float(0.9),
                                C.c_float(0.999), C.c_float(1e-15), 1, 1, s)
    assert rc == 0                                                    # n = 0: a no-op
    torch.cuda.synchronize()
    assert torch.equal(p, keep) and bool((g == 1).all()) and not bool(m.any()) and not bool(v.any())
