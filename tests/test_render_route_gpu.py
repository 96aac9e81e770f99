"""GPU: the drop-in ``render()`` (gaussian_renderer/__init__.py:18-157 of the reference) reaches the headline kernels.

Under the reference's default pipeline flags ``render()`` is ONE autograd node over cgs_view_forward_checked /
cgs_view_backward (ops/view_render.py): the unit-colour forward with the in-kernel tile sort and the pair-major backward that
bench.py times -- through the call sequence of train.py:95-107.  Checked here: which route runs, that both routes agree,
the full-size result against the C oracle on identical inputs, and every switch of the reference's signature."""
import math

import numpy as np
import pytest
import torch

from oracle import raster as ORA
from oracle import torch_ref as TR
from util import S, assert_close, tanfov

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _model(curves, mask=None, device=None):
    from curve_gaussian_amd.scene import GaussianCurveModel
    return GaussianCurveModel(0, 12, device=device or DEV).create_from_curves(curves["curve_points"], curves["width"],
                                                                              curves["opacity"], mask, curves["is_bezier"])


def _small(B=300, seed=5, H=96, W=128):
    c = S.make_curves(B, seed)
    g = torch.Generator().manual_seed(seed)
    c["width"] = c["width"] + 0.8 + 0.3 * torch.randn(B, 1, generator=g)
    c["is_bezier"] = torch.rand(B, generator=g) > 0.25
    mask = torch.randn(B, 12, 1, generator=g) * 3
    cam = S.make_camera((0.5, -1.7, 0.9), (0.5, 0.5, 0.5), (0, 0, 1), H, W)
    return c, mask, cam


def _count_fused_calls(monkeypatch):
    from curve_gaussian_amd.ops import view_render as VR
    calls = []
    orig = VR.view_render
    monkeypatch.setattr(VR, "view_render", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    return calls


@pytest.mark.parametrize("use_mask", [False, True])
def test_default_render_takes_the_fused_route_and_equals_the_general_one(use_mask, monkeypatch):
    from curve_gaussian_amd.gaussian_renderer import PipelineParams, render
    c, mask, cam = _small()
    cam = cam.to(DEV)
    H, W = cam.image_height, cam.image_width
    bg = torch.zeros(3, device=DEV)
    dimg = torch.randn(1, H, W, generator=torch.Generator().manual_seed(1)).to(DEV)
    calls = _count_fused_calls(monkeypatch)
    out = {}
    ncalls = {}
    for route in (None, False):
        gm = _model(c, mask)
        before = len(calls)
        pkg = render(cam, gm, PipelineParams(), bg, use_mask=use_mask, mask_thr=0.3, fused=route)
        ncalls[route] = len(calls) - before
        (pkg["render"] * dimg).sum().backward()
        out[route] = (pkg, gm)
    # (more than one call: the first forward of a new workload shape may outgrow its buckets and is redone)
    assert ncalls[None] >= 1 and ncalls[False] == 0, "render() with default flags must run the fused view path (and fused=False must not)"
    (pf, gf), (pg, gg) = out[None], out[False]
    assert torch.equal(pf["radii"], pg["radii"]) and torch.equal(pf["visibility_filter"], pg["visibility_filter"])
    for k in ("render", "depth", "rend_dir", "rend_alpha"):
        assert_close(k, pf[k].detach().cpu().numpy(), pg[k].detach().cpu().numpy())
    assert_close("means2D grad", pf["viewspace_points"].grad.cpu().numpy(), pg["viewspace_points"].grad.cpu().numpy(), abs_floor=1e-6)
    names = ("_curve_points", "_width", "_opacity") + (("_mask",) if use_mask else ())
    for name in names:
        a, b = getattr(gf, name).grad, getattr(gg, name).grad
        rel = float((a - b).norm() / b.norm())
        assert rel < 2e-5, f"{name}: fused vs general route relative L2 {rel:.2e}"
    if not use_mask:
        assert gf._mask.grad is None


def test_stale_derived_tensors_send_render_down_the_general_route(monkeypatch):
    """The reference renders `pc.get_xyz` as it finds it; the fused route samples the curves itself, so it is only taken while
    the derived tensors belong to the current parameters."""
    from curve_gaussian_amd.gaussian_renderer import PipelineParams, render
    c, mask, cam = _small(B=60)
    cam = cam.to(DEV)
    gm = _model(c, mask)
    calls = _count_fused_calls(monkeypatch)
    bg = torch.zeros(3, device=DEV)
    render(cam, gm, PipelineParams(), bg)                      # (sizes the buckets of this shape)
    calls.clear()
    with torch.no_grad():
        gm._curve_points.add_(0.01)
    stale = render(cam, gm, PipelineParams(), bg)["render"]
    assert len(calls) == 0
    with pytest.raises(ValueError):
        render(cam, gm, PipelineParams(), bg, fused=True)
    gm.prepare_scaling_rot()
    fresh = render(cam, gm, PipelineParams(), bg)["render"]
    assert len(calls) == 1 and not torch.equal(stale, fresh)


@pytest.mark.parametrize("use_mask", [False, True])
def test_fused_route_serves_depth_and_normal_losses(use_mask):
    """A loss on depth / rend_dir / rend_alpha through the DEFAULT render() (the reference's rasterizer backward takes
    grad_out_depth and grad_out_all_map, diff_cur_rasterization/__init__.py:117-151): the fused node's backward re-renders the
    view through the general operator route and pulls every upstream gradient through it -- same gradients as fused=False,
    and a loss on `render` alone afterwards still takes the fast backward."""
    from curve_gaussian_amd.gaussian_renderer import PipelineParams, render
    c, mask, cam = _small(B=200)
    cam = cam.to(DEV)
    H, W = cam.image_height, cam.image_width
    bg = torch.zeros(3, device=DEV)
    g = torch.Generator().manual_seed(11)
    w_img, w_d, w_n, w_a = (torch.randn(s_, generator=g).to(DEV) for s_ in ((1, H, W), (1, H, W), (3, H, W), (1, H, W)))
    grads = {}
    for route in (None, False):
        gm = _model(c, mask)
        pkg = render(cam, gm, PipelineParams(), bg, use_mask=use_mask, mask_thr=0.3, fused=route)
        loss = ((pkg["render"] * w_img).sum() + (pkg["depth"] * w_d).sum() + (pkg["rend_dir"] * w_n).sum()
                + (pkg["rend_alpha"] * w_a).sum())
        loss.backward()
        names = ("_curve_points", "_width", "_opacity") + (("_mask",) if use_mask else ())
        grads[route] = {n: getattr(gm, n).grad.clone() for n in names}
        grads[route]["means2D"] = pkg["viewspace_points"].grad.clone()
    for n, a in grads[None].items():
        b = grads[False][n]
        assert float(b.abs().max()) > 0, n
        rel = float((a - b).norm() / b.norm())
        assert rel < 2e-5, f"{n}: fused-route backward (general recomputation) vs general route: relative L2 {rel:.2e}"
    # depth alone (no gradient at `render`)
    gm = _model(c, mask)
    pkg = render(cam, gm, PipelineParams(), bg)
    (pkg["depth"] * w_d).sum().backward()
    gm2 = _model(c, mask)
    pkg2 = render(cam, gm2, PipelineParams(), bg, fused=False)
    (pkg2["depth"] * w_d).sum().backward()
    rel = float((gm._curve_points.grad - gm2._curve_points.grad).norm() / gm2._curve_points.grad.norm())
    assert rel < 2e-5, rel


@pytest.mark.parametrize("use_mask", [False, True])
def test_grad_sinks_put_the_same_gradients_into_existing_grad_buffers(use_mask):
    """render(grad_sinks=True): the backward kernels add into the parameters' `.grad` (what TrainStep(fused=True) uses on its
    flat gradient buffer); same numbers as autograd's own accumulation, on top of what the buffers already held, and a loss
    that reaches the geometry maps (general backward) still lands in `.grad` the ordinary way."""
    from curve_gaussian_amd.gaussian_renderer import PipelineParams, render
    c, mask, cam = _small()
    cam = cam.to(DEV)
    H, W = cam.image_height, cam.image_width
    bg = torch.zeros(3, device=DEV)
    gen = torch.Generator().manual_seed(3)
    dimg = torch.randn(1, H, W, generator=gen).to(DEV)
    ddepth = torch.randn(1, H, W, generator=gen).to(DEV)
    names = ["_curve_points", "_width", "_opacity"] + (["_mask"] if use_mask else [])
    got = {}
    for sinks in (False, True):
        gm = _model(c, mask)
        prior = {}
        for i, n in enumerate(names):   # something already in the buffers: the sinks must add, not overwrite
            p = getattr(gm, n)
            p.grad = torch.full_like(p, 0.25 * (i + 1))
            prior[n] = p.grad
        pkg = render(cam, gm, PipelineParams(), bg, use_mask=use_mask, mask_thr=0.3, grad_sinks=sinks)
        ((pkg["render"] * dimg).sum() + 0.1 * gm._width.sum()).backward()      # (+ a term autograd accumulates itself)
        pkg = render(cam, gm, PipelineParams(), bg, use_mask=use_mask, mask_thr=0.3, grad_sinks=sinks)
        ((pkg["render"] * dimg).sum() + (pkg["depth"] * ddepth).sum()).backward()   # depth loss: the general backward
        for n in names:
            assert getattr(gm, n).grad is prior[n]          # still the caller's buffer
        got[sinks] = {n: getattr(gm, n).grad.detach().cpu() for n in names}
        got[sinks]["m2d"] = pkg["viewspace_points"].grad.detach().cpu()
    for n in got[False]:
        assert_close(n, got[True][n], got[False][n], rel=2e-4)
    if not use_mask:   # a parameter outside the call keeps its own .grad untouched
        assert gm._mask.grad is None or float(gm._mask.grad.abs().max()) == 0.0


def test_grad_sinks_replaced_between_forward_and_backward_fall_back_to_autograd():
    """the sinks are the `.grad` tensors of FORWARD time.  zero_grad(set_to_none=True) (or a rebound flat buffer)
    between forward and backward must not make the kernels add into an orphaned tensor: the node then returns its gradients and
    autograd accumulates them into whatever `.grad` is current."""
    from curve_gaussian_amd.gaussian_renderer import PipelineParams, render
    c, mask, cam = _small()
    cam = cam.to(DEV)
    bg = torch.zeros(3, device=DEV)
    dimg = torch.randn(1, cam.image_height, cam.image_width, generator=torch.Generator().manual_seed(3)).to(DEV)
    names = ["_curve_points", "_width", "_opacity"]
    ref = _model(c, mask)
    (render(cam, ref, PipelineParams(), bg)["render"] * dimg).sum().backward()
    gm = _model(c, mask)
    orphans = {}
    for n in names:
        p = getattr(gm, n)
        p.grad = torch.zeros_like(p)
        orphans[n] = p.grad
    pkg = render(cam, gm, PipelineParams(), bg, grad_sinks=True)
    for n in names:
        getattr(gm, n).grad = None                     # zero_grad(set_to_none=True)
    (pkg["render"] * dimg).sum().backward()
    for n in names:
        assert float(orphans[n].abs().max()) == 0.0, n            # nothing was added behind the caller's back
        assert_close(n, getattr(gm, n).grad.cpu(), getattr(ref, n).grad.cpu(), rel=2e-4)


def test_fused_route_and_loss_are_cpp_autograd_nodes_under_the_shim():
    """with the compiled shim the fused view route and the photometric loss are torch::autograd::Function nodes of
    _cgs_torch.so (their backward runs on the engine's device thread without the GIL); CGS_TORCH_SHIM=0 keeps the Python nodes."""
    from curve_gaussian_amd import _lib as L
    from curve_gaussian_amd.gaussian_renderer import PipelineParams, render
    from curve_gaussian_amd.ops.losses import photometric_loss
    if not L.use_shim():
        pytest.skip("ctypes bindings selected")
    c, mask, cam = _small()
    cam = cam.to(DEV)
    gm = _model(c, mask)
    pkg = render(cam, gm, PipelineParams(), torch.zeros(3, device=DEV), clamp=False)
    assert "ViewRenderFn" in pkg["render"].grad_fn.name(), pkg["render"].grad_fn.name()
    gt = (torch.rand(1, cam.image_height, cam.image_width, generator=torch.Generator().manual_seed(1)) > 0.9).float().to(DEV)
    loss = photometric_loss(pkg["render"], gt, 10.0, 0.1, clamp=True)
    assert "PhotometricLossFn" in loss.grad_fn.name(), loss.grad_fn.name()
    loss.backward()
    assert float(gm._curve_points.grad.abs().max()) > 0 and pkg["viewspace_points"].grad is not None


def _use_binding(monkeypatch, shim):
    """Select the fused node's binding: the compiled shim (ViewRenderFn, the default) or the ctypes bindings (_ViewRender,
    CGS_TORCH_SHIM=0).  The general route resolves its own binding once, so that choice is reset too."""
    from curve_gaussian_amd import diff_cur_rasterization as D
    if shim:
        monkeypatch.delenv("CGS_TORCH_SHIM", raising=False)
    else:
        monkeypatch.setenv("CGS_TORCH_SHIM", "0")
    monkeypatch.setattr(D._ExtProxy, "_impl", None)


def test_fused_route_backward_twice_over_one_forward(monkeypatch):
    """retain_graph + repeated backwards through one fused render(), under both bindings: the second and the third give the
    same gradients again (the grid-wide sums of the sampling backward are cleared by the forward once and by the node before
    any further backward -- without bumping the version of the saved buffer, which autograd checks at every unpack)."""
    from curve_gaussian_amd.gaussian_renderer import PipelineParams, render
    c, mask, cam = _small()
    cam = cam.to(DEV)
    dimg = torch.randn(1, cam.image_height, cam.image_width, generator=torch.Generator().manual_seed(5)).to(DEV)
    for shim in (True, False):
        _use_binding(monkeypatch, shim)
        gm = _model(c, mask)
        pkg = render(cam, gm, PipelineParams(), torch.zeros(3, device=DEV))
        wrt = [gm._curve_points, gm._width, gm._opacity]
        first = torch.autograd.grad(pkg["render"], wrt, dimg, retain_graph=True)
        for _ in range(2):
            again = torch.autograd.grad(pkg["render"], wrt, dimg, retain_graph=True)
            for a, b, n in zip(first, again, ("curve_points", "width", "opacity")):
                assert float(a.abs().max()) > 0
                assert_close(n, b.cpu(), a.cpu(), rel=2e-4)


def test_both_bindings_of_the_fused_node_agree(monkeypatch):
    """ViewRenderFn (compiled shim) and _ViewRender (ctypes bindings) make the same cgs_view_forward_render /
    cgs_view_backward_render calls: identical forward outputs and gradients equal to the rounding of the backward's atomics,
    for every switch the node takes (mask, clamp, direction map, eager / sync-free) and for a depth loss, which reaches the
    general backward."""
    from curve_gaussian_amd import _lib as L
    from curve_gaussian_amd.gaussian_renderer import PipelineParams, render
    from curve_gaussian_amd.ops import view_render as VR
    _use_binding(monkeypatch, True)
    if not L.use_shim():
        pytest.skip("CGS_LIB names an experiment build: the ctypes bindings are the only binding")
    c, mask, cam = _small()
    cam = cam.to(DEV)
    H, W = cam.image_height, cam.image_width
    bg = torch.zeros(3, device=DEV)
    gen = torch.Generator().manual_seed(7)
    dimg, ddepth = (torch.randn(1, H, W, generator=gen).to(DEV) for _ in range(2))
    render(cam, _model(c, mask), PipelineParams(), bg)              # (sizes the buckets of this shape)
    lib = L.load()
    cap = min(2 * VR._capacity(lib, torch.device(DEV), c["curve_points"].shape[0] * 12, W, H), int(lib.cgs_bucket_capacity_limit()))
    cases = [(use_mask, clamp, rend_dir, static, False) for use_mask in (False, True) for clamp in (False, True)
             for rend_dir in (False, True) for static in (False, True)]
    cases.append((True, True, True, False, True))
    for use_mask, clamp, rend_dir, static, depth_loss in cases:
        case = f"mask={use_mask} clamp={clamp} rend_dir={rend_dir} static={static} depth_loss={depth_loss}"
        got = {}
        for shim in (True, False):
            _use_binding(monkeypatch, shim)
            gm = _model(c, mask)
            sink = []
            pkg = render(cam, gm, PipelineParams(), bg, use_mask=use_mask, mask_thr=0.3, clamp=clamp, compute_rend_dir=rend_dir,
                         static_bucket_cap=cap if static else 0, status_sink=sink if static else None)
            node = pkg["render"].grad_fn.name()
            assert ("ViewRenderFn" in node) == shim and ("_ViewRender" in node) != shim, (case, node)
            if static:
                assert len(sink) == 1 and int(sink[0][2]) == 0, case        # (status word 2: a bucket overflowed)
            loss = (pkg["render"] * dimg).sum()
            if depth_loss:
                loss = loss + (pkg["depth"] * ddepth).sum()
            loss.backward()
            grads = {n: getattr(gm, n).grad for n in ("_curve_points", "_width", "_opacity", "_mask")}
            grads["viewspace_points"] = pkg["viewspace_points"].grad
            got[shim] = pkg, grads
        (ps, gs), (pc, gc) = got[True], got[False]
        for k in ("render", "depth", "rend_alpha", "rend_dir", "radii", "visibility_filter"):
            assert (ps[k] is None) == (pc[k] is None), (case, k)
            assert ps[k] is None or torch.equal(ps[k], pc[k]), (case, k)
        for n, a in gs.items():
            b = gc[n]
            assert (a is None) == (b is None), (case, n)
            if a is not None:
                assert float(a.abs().max()) > 0, (case, n)
                assert_close(f"{case} {n}", b.cpu(), a.cpu(), rel=2e-4)


def test_fused_route_resamples_with_the_eps_of_prepare_scaling_rot(monkeypatch):
    """prepare_scaling_rot(eps) stamps the eps it used; the fused route (which samples the curves itself) renders with it, so
    both routes draw the same splats for any eps."""
    from curve_gaussian_amd.gaussian_renderer import PipelineParams, render
    c, mask, cam = _small(B=120)
    cam = cam.to(DEV)
    bg = torch.zeros(3, device=DEV)
    gm = _model(c, mask)
    gm.prepare_scaling_rot(eps=0.5)      # (an absurd eps: changes rotations / scalings visibly)
    calls = _count_fused_calls(monkeypatch)
    a = render(cam, gm, PipelineParams(), bg)
    assert len(calls) >= 1
    b = render(cam, gm, PipelineParams(), bg, fused=False)
    assert torch.equal(a["radii"], b["radii"])
    assert_close("render", a["render"].detach().cpu().numpy(), b["render"].detach().cpu().numpy())
    gm.prepare_scaling_rot()
    d = render(cam, gm, PipelineParams(), bg)
    assert not torch.equal(a["render"], d["render"])


@pytest.mark.parametrize("B", [1, 37, 2000])
def test_visibility_filter_is_nonzero_of_radii_in_one_launch(B):
    """render()["visibility_filter"] == (radii > 0).nonzero() (gaussian_renderer/__init__.py:150): the fused route writes it with
    cgs_visible_indices from the per-chunk counts its checked forward left in the image buffer (no compare / nonzero kernels,
    no host sync); splat counts that do not divide into the 64 chunks, a camera that culls part of the cloud."""
    from curve_gaussian_amd.gaussian_renderer import PipelineParams, render
    c, mask, cam = _small(B=B, seed=9)
    cam = S.make_camera((0.5, 0.5, 0.5), (0.9, 0.2, 0.5), (0, 0, 1), 96, 128).to(DEV)     # inside the cloud: near culls
    gm = _model(c, mask)
    bg = torch.zeros(3, device=DEV)
    for fused in (None, False):
        pkg = render(cam, gm, PipelineParams(), bg, fused=fused)
        want = (pkg["radii"] > 0).nonzero()
        got = pkg["visibility_filter"]
        assert got.dtype == want.dtype and got.shape == want.shape and torch.equal(got, want), fused
        assert 0 < want.shape[0] < pkg["radii"].shape[0] or B == 1


def test_two_models_interleave_their_fused_forwards():
    """Pending forwards are carried by handle (cgs_view_forward_begin -> cgs_view_forward_wait(handle)): two view_render calls
    of different models / image sizes begun back to back and finished in the opposite order do not disturb each other."""
    from curve_gaussian_amd.gaussian_renderer import PipelineParams, render
    from curve_gaussian_amd.ops import view_render as VR
    c1, mask1, cam1 = _small(B=150, seed=5)
    c2, mask2, cam2 = _small(B=260, seed=6, H=64, W=80)
    gm1, gm2 = _model(c1, mask1), _model(c2, mask2)
    cam1, cam2 = cam1.to(DEV), cam2.to(DEV)
    bg = torch.zeros(3, device=DEV)
    ref1 = render(cam1, gm1, PipelineParams(), bg)["render"].clone()   # (also sizes the buckets of both shapes)
    ref2 = render(cam2, gm2, PipelineParams(), bg)["render"].clone()

    def begin(gm, cam):
        pend = []
        z = torch.zeros_like(gm.get_xyz, requires_grad=True)
        out = VR.view_render(gm._curve_points, gm._width, gm._opacity, None, z, gm.is_bezier, gm.n_gaussians, 0.01, bg, cam,
                             *tanfov(cam), 0, None, True, False, pend)
        return out[0], pend[0]
    img1, p1 = begin(gm1, cam1)
    img2, p2 = begin(gm2, cam2)
    ok2, n2 = VR.finish(p2)
    ok1, n1 = VR.finish(p1)
    assert ok1 and ok2
    assert n1 == int((render(cam1, gm1, PipelineParams(), bg)["radii"] > 0).sum())
    assert torch.equal(img1, ref1) and torch.equal(img2, ref2)
    assert VR.finish(p1) == (True, -1)                  # a finished handle is inert
    # a dropped Pending gives its slot back (no leak after many abandoned forwards)
    for _ in range(200):
        _img, p = begin(gm2, cam2)
        del p
    img2b, p2b = begin(gm2, cam2)
    assert VR.finish(p2b)[0] and torch.equal(img2b, ref2)


def _begin_view(gm, cam, bg):
    """A checked fused forward left outstanding: (image, Pending) -- its status slot is held until VR.finish()."""
    from curve_gaussian_amd.ops import view_render as VR
    pend = []
    z = torch.zeros_like(gm.get_xyz, requires_grad=True)
    out = VR.view_render(gm._curve_points, gm._width, gm._opacity, None, z, gm.is_bezier, gm.n_gaussians, 0.01, bg, cam,
                         *tanfov(cam), 0, None, True, False, pend)
    return out[0], pend[0]


def test_operator_forward_between_begin_and_wait_of_view_forwards():
    """The operator API (the general route) and the checked view forwards read their status back through one slot pool: an
    operator forward run while view forwards are outstanding takes a slot of its own and gives it back, and every image
    equals the one rendered alone."""
    from curve_gaussian_amd.gaussian_renderer import PipelineParams, render
    from curve_gaussian_amd.ops import view_render as VR
    c1, mask1, cam1 = _small(B=150, seed=5)
    c2, mask2, cam2 = _small(B=260, seed=6, H=64, W=80)
    gm1, gm2 = _model(c1, mask1), _model(c2, mask2)
    cam1, cam2 = cam1.to(DEV), cam2.to(DEV)
    bg = torch.zeros(3, device=DEV)
    ref1 = render(cam1, gm1, PipelineParams(), bg)["render"].clone()
    ref2 = render(cam2, gm2, PipelineParams(), bg)["render"].clone()
    for _ in range(2):   # (the first general forward takes the exact binning path, the second the bucket path)
        ref_op = render(cam1, gm1, PipelineParams(), bg, fused=False)["render"].clone()
    pending = [_begin_view(gm, cam, bg) for gm, cam in ((gm1, cam1), (gm2, cam2), (gm1, cam1))]
    op = render(cam1, gm1, PipelineParams(), bg, fused=False)["render"]
    assert [VR.finish(p)[0] for _img, p in pending] == [True] * 3
    assert torch.equal(op, ref_op)
    for (img, _p), ref in zip(pending, (ref1, ref2, ref1)):
        assert torch.equal(img, ref)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs")
def test_status_slots_move_to_another_device_once_idle():
    """Every slot of the pool bound to cuda:0 (64 checked forwards outstanding at once, then finished): a checked view
    forward and an operator-API forward on cuda:1 rebind idle slots and render what they render alone."""
    from curve_gaussian_amd.gaussian_renderer import PipelineParams, render
    from curve_gaussian_amd.ops import view_render as VR
    c1, mask1, cam1 = _small(B=150, seed=5)
    gm0, cam0 = _model(c1, mask1), cam1.to(DEV)
    bg0 = torch.zeros(3, device=DEV)
    pending = [_begin_view(gm0, cam0, bg0) for _ in range(64)]
    assert all(VR.finish(p)[0] for _img, p in pending)
    del pending
    dev = "cuda:1"
    with torch.cuda.device(dev):
        gm, cam, bg = _model(c1, mask1, device=dev), cam1.to(dev), torch.zeros(3, device=dev)
        view = render(cam, gm, PipelineParams(), bg)["render"].clone()
        op = render(cam, gm, PipelineParams(), bg, fused=False)["render"].clone()
        torch.cuda.synchronize()
        assert torch.equal(render(cam, gm, PipelineParams(), bg)["render"], view)
        assert torch.equal(render(cam, gm, PipelineParams(), bg, fused=False)["render"], op)


def _render_loop(gm, cam, bg, n, out, key):
    from curve_gaussian_amd.gaussian_renderer import PipelineParams, render
    try:
        with torch.cuda.device(cam.world_view_transform.device):
            imgs = [render(cam, gm, PipelineParams(), bg)["render"].clone() for _ in range(n)]
            torch.cuda.synchronize()
        out[key] = imgs
    except Exception as e:   # noqa: BLE001 -- handed to the asserting thread
        out[key] = e


def test_checked_forwards_of_two_threads_share_the_status_slot_pool():
    """the readback slots (pinned words + event) are a process-wide pool; two threads that render
    concurrently take and release slots under the pool's mutex and every image equals the one the thread renders alone."""
    import threading
    from curve_gaussian_amd.gaussian_renderer import PipelineParams, render
    c1, mask1, cam1 = _small(B=150, seed=5)
    c2, mask2, cam2 = _small(B=260, seed=6, H=64, W=80)
    gm1, gm2 = _model(c1, mask1), _model(c2, mask2)
    cam1, cam2 = cam1.to(DEV), cam2.to(DEV)
    bg = torch.zeros(3, device=DEV)
    ref1 = render(cam1, gm1, PipelineParams(), bg)["render"].clone()
    ref2 = render(cam2, gm2, PipelineParams(), bg)["render"].clone()
    out = {}
    ts = [threading.Thread(target=_render_loop, args=(gm1, cam1, bg, 40, out, 1)),
          threading.Thread(target=_render_loop, args=(gm2, cam2, bg, 40, out, 2))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for key, ref in ((1, ref1), (2, ref2)):
        assert not isinstance(out[key], Exception), out[key]
        assert all(torch.equal(i, ref) for i in out[key])


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs")
def test_checked_forwards_on_two_devices():
    """a status slot's event belongs to the device it was created on; a checked forward on cuda:1 after one on
    cuda:0 must not reuse cuda:0's slot (hipEventRecord rejects an event / stream pair of different devices).  The binning
    hints are per device as well."""
    from curve_gaussian_amd.gaussian_renderer import PipelineParams, render
    c1, mask1, cam1 = _small(B=150, seed=5)
    imgs = []
    for dev in ("cuda:0", "cuda:1", "cuda:0", "cuda:1"):
        with torch.cuda.device(dev):
            gm = _model(c1, mask1, device=dev)
            cam = cam1.to(dev)
            out = render(cam, gm, PipelineParams(), torch.zeros(3, device=dev))
            loss = out["render"].sum()
            loss.backward()
            torch.cuda.synchronize()
            imgs.append(out["render"].detach().cpu())
    assert torch.equal(imgs[0], imgs[2]) and torch.equal(imgs[1], imgs[3])
    assert torch.allclose(imgs[0], imgs[1], atol=1e-6)


def test_fused_route_grows_its_buckets_and_remembers_the_capacity():
    from curve_gaussian_amd import _lib as L
    from curve_gaussian_amd.gaussian_renderer import PipelineParams, render
    from curve_gaussian_amd.ops import view_render as VR
    lib = L.load()
    lib.cgs_reset_binning_hints()
    VR._caps.clear()
    c, mask, cam = _small(B=900, seed=3)
    c["width"] = c["width"] + 1.0              # long tile lists on a small image: the first guess (128) overflows
    gm = _model(c, mask)
    cam = cam.to(DEV)
    bg = torch.zeros(3, device=DEV)
    a = render(cam, gm, PipelineParams(), bg)
    import ctypes as C
    R_, longest_, path_ = C.c_int64(0), C.c_int64(0), C.c_int(0)
    lib.cgs_last_forward_stats(C.byref(R_), C.byref(longest_), C.byref(path_))
    longest = [longest_.value]
    assert longest[0] > 128, "scene too sparse to exercise the overflow redo"
    cap = VR._caps[(0, gm._xyz.shape[0], cam.image_width, cam.image_height)]
    assert cap >= longest[0] and int(lib.cgs_bucket_capacity_hint(gm._xyz.shape[0], cam.image_width, cam.image_height)) >= longest[0]
    b = render(cam, gm, PipelineParams(), bg, fused=False)
    assert_close("render after redo", a["render"].detach().cpu().numpy(), b["render"].detach().cpu().numpy())
    assert torch.equal(a["radii"], b["radii"])


# ------------------------------------------------------------------------------------------------ flags of the signature
def test_compute_cov3d_python_routes_the_model_covariance_through_cov3d_precomp():
    """gaussian_renderer/__init__.py:67-68 with scene/gaussian_model.py:32-36,184-185: the same Gaussians, handed over as
    packed 3D covariances; against the torch restatement of build_covariance_from_scaling_rotation and against the default
    route's image."""
    from curve_gaussian_amd.gaussian_renderer import PipelineParams, render
    c, mask, cam = _small(B=200, seed=9)
    gm = _model(c, mask)
    cam = cam.to(DEV)
    bg = torch.zeros(3, device=DEV)
    pipe = PipelineParams()
    pipe.compute_cov3D_python = True
    # restatement (utils/general_utils.py:134-181)
    r = gm._rotation.detach().cpu().double()
    q = r / r.norm(dim=1, keepdim=True)
    w, x, y, z = q.unbind(-1)
    Rm = torch.stack((1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z),
                      1 - 2 * (x * x + z * z), 2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x),
                      1 - 2 * (x * x + y * y)), -1).view(-1, 3, 3)
    Lm = Rm @ torch.diag_embed(gm._scaling.detach().cpu().double())
    cov = Lm @ Lm.transpose(1, 2)
    want = torch.stack((cov[:, 0, 0], cov[:, 0, 1], cov[:, 0, 2], cov[:, 1, 1], cov[:, 1, 2], cov[:, 2, 2]), -1)
    got = gm.get_covariance(1.0).detach().cpu().double()
    assert float((got - want).abs().max() / want.abs().max()) < 1e-6
    pk = render(cam, gm, pipe, bg)
    (pk["render"] * 1.0).sum().backward()
    g_cov = gm._curve_points.grad.clone()
    gm._curve_points.grad = None
    pd = render(cam, gm, PipelineParams(), bg)
    pd["render"].sum().backward()
    assert_close("render", pk["render"].detach().cpu().numpy(), pd["render"].detach().cpu().numpy())
    assert_close("rend_alpha", pk["rend_alpha"].detach().cpu().numpy(), pd["rend_alpha"].detach().cpu().numpy())
    assert (pk["radii"] != pd["radii"]).float().mean() < 1e-3     # ceil(3 sigma) of covariances that differ in the last bits
    rel = float((g_cov - gm._curve_points.grad).norm() / gm._curve_points.grad.norm())
    assert rel < 1e-4, f"curve gradient through cov3D_precomp vs scales / rotations: {rel:.2e}"
    # (:72-76 + diff_cur_rasterization/__init__.py:196-197) with use_mask the reference passes scales AND cov3D_precomp
    with pytest.raises(Exception, match="exactly one of either scale/rotation pair or precomputed 3D covariance"):
        render(cam, gm, pipe, bg, use_mask=True)


def test_use_trained_exp_applies_the_references_expression():
    """:131-135 is a [H,W,C] x [3,3] product: it type-checks for three channels only, so with this rasterizer's single
    channel the reference raises torch's shape error -- and so does the drop-in, on both routes (no silently ignored flag)."""
    from curve_gaussian_amd.gaussian_renderer import PipelineParams, _package, render
    c, mask, cam = _small(B=60)
    gm = _model(c, mask)
    gm.exposure_mapping = {"view0": 0}
    gm._exposure = torch.nn.Parameter((torch.eye(3, 4, device=DEV) * 0.5)[None].contiguous())
    cam = cam.to(DEV)
    cam.image_name = "view0"
    bg = torch.zeros(3, device=DEV)
    img = torch.rand(1, 8, 8, device=DEV)
    ex = gm.get_exposure_from_name("view0")
    with pytest.raises(RuntimeError):      # the restatement of :131-135 on a 1-channel image
        torch.matmul(img.permute(1, 2, 0), ex[:3, :3]).permute(2, 0, 1) + ex[:3, 3, None, None]
    for route in (None, False):
        with pytest.raises(RuntimeError):
            render(cam, gm, PipelineParams(), bg, use_trained_exp=True, fused=route)
    # on a 3-channel image the packaging step applies exposure exactly as the expression says
    img3 = torch.rand(3, 8, 8, device=DEV)
    amap = torch.rand(4, 8, 8, device=DEV)
    pkg = _package(cam, gm, img3, torch.ones(4, dtype=torch.int32, device=DEV), img3[:1], amap, None, True, True, False, False)
    want = (torch.matmul(img3.permute(1, 2, 0), ex[:3, :3]).permute(2, 0, 1) + ex[:3, 3, None, None]).clamp(0, 1)
    assert torch.allclose(pkg["render"], want)


def test_separate_sh_raises_like_the_reference():
    """:108-119: the reference passes `dc=` to a rasterizer without such a parameter."""
    from curve_gaussian_amd.gaussian_renderer import PipelineParams, render
    c, mask, cam = _small(B=20)
    gm = _model(c, mask)
    with pytest.raises(TypeError, match="unexpected keyword argument 'dc'"):
        render(cam.to(DEV), gm, PipelineParams(), torch.zeros(3, device=DEV), separate_sh=True)


# ------------------------------------------------------------------------------------------------ full size
def test_render_route_matches_the_oracle_at_cfg3_under_the_defaults():
    """What train.py:95-107 executes, at the BASELINE size the headline is quoted on: render() with the reference's default
    arguments -> fused view path.  The C oracle gets the model's derived splat tensors (HIP sampling kernels; pinned against
    the torch restatement in test_sampling_gpu.py), so both compositors see the same splats.  Image, alpha, inverse depth,
    world-space direction map and the screen-space gradient under the rasterizer criterion (1e-4 of max, 1e-4 flip budget);
    curve-parameter gradients in relative L2 AND element-wise against the torch pull-back of the oracle's per-splat
    gradients."""
    from curve_gaussian_amd.gaussian_renderer import PipelineParams, render
    curves, cams = S.make_config("cfg3", n_views=1)
    cam = cams[0]
    H, W = cam.image_height, cam.image_width
    gm = _model(curves)
    bg = torch.zeros(3, device=DEV)
    pkg = render(cam.to(DEV), gm, PipelineParams(), bg)
    dimg = torch.randn(1, H, W, generator=torch.Generator().manual_seed(17))
    (pkg["render"] * dimg.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    xyz_h, rot_h, scl_h = (t.detach().cpu() for t in (gm._xyz, gm._rotation, gm._scaling))
    P = xyz_h.shape[0]
    rotn_h = torch.nn.functional.normalize(rot_h)
    opac = torch.sigmoid(curves["opacity"]).repeat_interleave(12, 0)
    amap = TR.build_all_map(rot_h, xyz_h, cam.camera_center, cam.world_view_transform).float().contiguous()
    tfx, tfy = tanfov(cam)
    n = lambda t: np.ascontiguousarray(t.detach().numpy())
    fw = ORA.forward(np.zeros(3, np.float32), n(xyz_h), np.ones((P, 1), np.float32), n(opac), n(scl_h), n(rotn_h), 1.0, None,
                     n(amap), n(cam.world_view_transform), n(cam.full_proj_transform), tfx, tfy, H, W, None, 0,
                     n(cam.camera_center))
    radii = pkg["radii"].cpu().numpy()
    off = radii != fw.radii
    assert off.mean() <= 1e-5 and (np.abs(radii[off] - fw.radii[off]) <= 1).all()
    assert_close("render", pkg["render"].detach().cpu().numpy(), np.clip(fw.color, 0, 1))
    assert_close("rend_alpha", pkg["rend_alpha"].detach().cpu().numpy(), fw.out_all_map[3:4])
    assert_close("depth", pkg["depth"].detach().cpu().numpy(), fw.invdepth)
    rd = torch.tensor(fw.out_all_map[0:3]).permute(1, 2, 0) @ cam.world_view_transform[:3, :3].T
    assert_close("rend_dir", pkg["rend_dir"].detach().cpu().numpy(), rd.permute(2, 0, 1).numpy())
    gr = ORA.backward(fw, np.where((fw.color > 0) & (fw.color < 1), dimg.numpy(), 0).astype(np.float32), None, None)
    assert_close("means2D grad", pkg["viewspace_points"].grad.cpu().numpy(), gr["dL_dmeans2D"], abs_floor=1e-6)
    leaves = [curves[k].clone().requires_grad_(True) for k in ("curve_points", "width", "opacity")]
    xyz, rot, scl = TR.prepare_scaling_rot(leaves[0], leaves[1], curves["is_bezier"])
    t = lambda a: torch.from_numpy(np.asarray(a, np.float32))
    ((xyz * t(gr["dL_dmeans3D"])).sum() + (scl * t(gr["dL_dscales"])).sum()
     + (torch.nn.functional.normalize(rot) * t(gr["dL_drotations"])).sum()
     + (torch.sigmoid(leaves[2]).repeat_interleave(12, 0) * t(gr["dL_dopacity"])).sum()).backward()
    for name, leaf in zip(("_curve_points", "_width", "_opacity"), leaves):
        got = getattr(gm, name).grad.cpu()
        rel = float((got - leaf.grad).norm() / leaf.grad.norm())
        worst = float((got - leaf.grad).abs().max() / leaf.grad.abs().max())
        print(f"render() route cfg3: dL/d{name} relative L2 {rel:.2e}, worst element {worst:.2e} of max")
        # measured 2.5e-5 (curve_points), 5.4e-5 (width): the oracle is fed the model's derived tensors (general sampling kernel)
        # while the fused route samples inside its own kernel -- the last bits of a few splat parameters differ; on
        # bit-identical inputs the same kernels reach 2e-6 .. 8e-6 (test_headline_instances_..., test_pipeline_gpu.py)
        assert rel < 1e-4, f"dL/d{name}: relative L2 error {rel:.2e}"
        # element-wise: 1e-4 of max on all but 1e-3 of the curves, nothing beyond 1e-3 of max (measured worst 1.5e-4: the
        # sampling backward sums 12 samples per curve with cancellation, and the compositor's float atomics reorder)
        assert_close(f"dL/d{name} (element-wise)", got.numpy(), leaf.grad.numpy(), outlier_frac=1e-3, max_outlier=1e-3)
    fw.free()


def test_render_route_on_a_room_scale_scene_with_screen_filling_splats():
    """cfg4-like geometry (cameras inside the scene box: near-camera splats whose tile rect covers the whole screen, deferred
    to the one-workgroup-per-splat scatter once a checked forward has counted them): the fused route against the general one,
    twice in a row (the second call runs with the deferral switched on by the first)."""
    from curve_gaussian_amd import _lib as L
    from curve_gaussian_amd.gaussian_renderer import PipelineParams, render
    L.load().cgs_reset_binning_hints()
    curves, cams = S.make_config("cfg4", n_views=2)
    keep = slice(0, 3000)
    curves = {k: (v[keep] if torch.is_tensor(v) and v.shape[0] > 3000 else v) for k, v in curves.items()}
    bg = torch.zeros(3, device=DEV)
    for cam in cams:
        cam = cam.to(DEV)
        gm = _model(curves)
        a = render(cam, gm, PipelineParams(), bg)
        b = render(cam, gm, PipelineParams(), bg, fused=False)
        assert torch.equal(a["radii"], b["radii"])
        assert int(a["radii"].max()) > 100, "scene has no splat whose tile rect exceeds the 96-tile comfort zone of the wave walk"
        for k in ("render", "depth", "rend_alpha"):
            assert_close(k, a[k].detach().cpu().numpy(), b[k].detach().cpu().numpy())
        assert torch.equal(a["visibility_filter"], b["visibility_filter"])
