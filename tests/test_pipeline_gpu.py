"""GPU: the drop-in renderer glue and the training step on the HIP hot path.
render() (gaussian_renderer/__init__.py:18-157) is checked end-to-end against the composition of the oracles:
torch restatement of the curve model -> C rasterizer oracle."""
import math
import os
import sys

import numpy as np
import pytest
import torch

from oracle import raster as ORA
from oracle import torch_ref as TR
from util import S, assert_close, tanfov

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _model(B, seed, H=96, W=128):
    from curve_gaussian_amd.scene import GaussianCurveModel
    c = S.make_curves(B, seed)
    g = torch.Generator().manual_seed(seed)
    c["width"] = c["width"] + 0.8 + 0.3 * torch.randn(B, 1, generator=g)     # fatter splats for a small image
    c["mask"] = torch.randn(B, 12, 1, generator=g) * 3
    c["is_bezier"] = torch.rand(B, generator=g) > 0.25
    gm = GaussianCurveModel(0, 12, device=DEV).create_from_curves(c["curve_points"], c["width"], c["opacity"],
                                                                  c["mask"], c["is_bezier"])
    cam = S.make_camera((0.5, -1.7, 0.9), (0.5, 0.5, 0.5), (0, 0, 1), H, W)
    return gm, c, cam


@pytest.mark.parametrize("use_mask", [False, True])
def test_render_matches_oracle_composition(use_mask):
    from curve_gaussian_amd.gaussian_renderer import PipelineParams, render
    gm, c, cam = _model(300, 5)
    H, W = cam.image_height, cam.image_width
    bg = torch.zeros(3, device=DEV)
    thr = 0.3
    pkg = render(cam.to(DEV), gm, PipelineParams(), bg, use_mask=use_mask, mask_thr=thr)
    g = torch.Generator().manual_seed(1)
    dimg = torch.randn(1, H, W, generator=g)
    (pkg["render"] * dimg.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    # ---- oracle composition on the splat tensors the model derived (HIP sampling kernels; checked against the torch
    # restatement in test_sampling_gpu.py), so that both rasterizers see the same splats
    xyz, rot, scl = (t.detach().cpu() for t in (gm._xyz, gm._rotation, gm._scaling))
    P = xyz.shape[0]
    rotn = torch.nn.functional.normalize(rot)
    opac = torch.sigmoid(c["opacity"]).unsqueeze(1).expand(-1, 12, -1).reshape(-1, 1)
    if use_mask:
        mk = (torch.sigmoid(c["mask"]) > thr).float().view(-1, 1)
        scl, opac = scl * mk, opac * mk
    amap = TR.build_all_map(rot, xyz, cam.camera_center, cam.world_view_transform)
    tfx, tfy = tanfov(cam)
    n = lambda t: t.detach().numpy()
    fw = ORA.forward(np.zeros(3, np.float32), n(xyz), np.ones((P, 1), np.float32), n(opac), n(scl), n(rotn), 1.0, None,
                     n(amap), n(cam.world_view_transform), n(cam.full_proj_transform), tfx, tfy, H, W, None, 0,
                     n(cam.camera_center))
    assert (pkg["radii"].cpu().numpy() == fw.radii).all()
    assert_close("render", pkg["render"].detach().cpu().numpy(), np.clip(fw.color, 0, 1))
    assert_close("rend_alpha", pkg["rend_alpha"].detach().cpu().numpy(), fw.out_all_map[3:4])
    rd = torch.tensor(fw.out_all_map[0:3]).permute(1, 2, 0) @ cam.world_view_transform[:3, :3].T
    assert_close("rend_dir", pkg["rend_dir"].detach().cpu().numpy(), rd.permute(2, 0, 1).numpy())
    assert pkg["visibility_filter"].shape[1] == 1 and pkg["viewspace_points"].grad.shape == (P, 3)
    # gradient reaches the curve parameters; means2D grad is consumable by add_densification_stats (GM:618-620)
    assert gm._curve_points.grad.abs().max() > 0 and gm._opacity.grad.abs().max() > 0
    gm.add_densification_stats(pkg["viewspace_points"], pkg["visibility_filter"].squeeze(1))
    assert gm.denom.sum() == pkg["visibility_filter"].shape[0]
    gr = ORA.backward(fw, np.where((fw.color > 0) & (fw.color < 1), dimg.numpy(), 0).astype(np.float32), None, None)
    assert_close("means2D grad", pkg["viewspace_points"].grad.cpu().numpy(), gr["dL_dmeans2D"], abs_floor=1e-6)
    fw.free()


def test_edge_aware_loss_matches_reference_golden():
    from curve_gaussian_amd.ops.losses import edge_aware_loss
    d = np.load(os.path.join(G, "edge_aware_loss.npz"))
    img = torch.tensor(d["image"], device=DEV).requires_grad_(True)
    val = edge_aware_loss(img, torch.tensor(d["gt"], device=DEV))
    (3.0 * val).backward()
    np.testing.assert_allclose(float(val), d["value"], rtol=1e-5)
    np.testing.assert_allclose(img.grad.cpu().numpy(), 3.0 * d["grad"], rtol=1e-4, atol=2e-6)
    # multi-channel + degenerate gt (no edges at all)
    g = torch.Generator().manual_seed(2)
    im3, gt3 = torch.rand(3, 33, 47, generator=g), torch.zeros(3, 33, 47)
    ref_in = im3.clone().requires_grad_(True)
    ref = TR.edge_aware_loss(ref_in, gt3)
    ref.backward()
    x = im3.to(DEV).requires_grad_(True)
    v = edge_aware_loss(x, gt3.to(DEV))
    v.backward()
    np.testing.assert_allclose(float(v), float(ref), rtol=1e-5)
    np.testing.assert_allclose(x.grad.cpu().numpy(), ref_in.grad.numpy(), rtol=1e-4, atol=2e-6)


def test_train_step_reduces_loss_and_keeps_layout():
    from curve_gaussian_amd.gaussian_renderer import PipelineParams, render
    from curve_gaussian_amd.train_step import TrainStep
    gm, c, cam = _model(200, 11, 64, 96)
    cams = [S.make_camera((0.5 + 1.8 * math.cos(a), 0.5 + 1.8 * math.sin(a), 0.9), (0.5, 0.5, 0.5), (0, 0, 1), 64, 96).to(DEV)
            for a in (0.3, 1.7, 3.1, 4.4)]
    # targets: renders of a perturbed copy of the model
    with torch.no_grad():
        gts = []
        tgt, _, _ = _model(200, 11, 64, 96)
        tgt._curve_points.add_(0.01 * torch.randn_like(tgt._curve_points))
        tgt.prepare_scaling_rot()
        for cm in cams:
            gts.append(render(cm, tgt, PipelineParams(), torch.zeros(3, device=DEV))["render"].detach())
    ts = TrainStep(gm, cams, gts, densify_until_iter=20)
    losses = [float(ts.step()[0]) for _ in range(30)]      # crosses the use_mask switch at iteration 20
    assert all(np.isfinite(losses))
    assert np.mean(losses[-8:-4]) < np.mean(losses[:4])
    assert gm._xyz.shape == (2400, 3) and gm._rotation.shape == (2400, 4) and gm._scaling.shape == (2400, 3)
    assert gm._curve_points.grad.data_ptr() == ts.flat.flat.data_ptr()   # grads still alias the flat buffer
    cp_group = [g for g in gm.optimizer.param_groups if g["name"] == "curve_points"][0]
    assert cp_group["lr"] < 5e-4   # update_learning_rate drives the fused optimizer through param_groups
    # the reference-style path (torch Adam + composed losses) still works and also descends
    gm2, _, _ = _model(200, 11, 64, 96)
    ts2 = TrainStep(gm2, cams, gts, densify_until_iter=20, fused=False)
    l2 = [float(ts2.step()[0]) for _ in range(12)]
    assert np.isfinite(l2).all() and abs(l2[0] - losses[0]) < 1e-3 * abs(losses[0])


def _train_fixture(n_curves=200, seed=11, H=64, W=96):
    from curve_gaussian_amd.gaussian_renderer import PipelineParams, render
    gm, c, cam = _model(n_curves, seed, H, W)
    cams = [S.make_camera((0.5 + 1.8 * math.cos(a), 0.5 + 1.8 * math.sin(a), 0.9), (0.5, 0.5, 0.5), (0, 0, 1), H, W).to(DEV)
            for a in (0.3, 1.7, 3.1, 4.4)]
    with torch.no_grad():
        gts = []
        tgt, _, _ = _model(n_curves, seed, H, W)
        tgt._curve_points.add_(0.01 * torch.randn_like(tgt._curve_points))
        tgt.prepare_scaling_rot()
        for cm in cams:
            gts.append(render(cm, tgt, PipelineParams(), torch.zeros(3, device=DEV))["render"].detach())
    return gm, cams, gts


def test_graphed_train_step_equals_eager_and_recovers_from_bucket_overflow():
    """GraphedTrainStep (one hipGraph launch per iteration, sync-free forward, device-state Adam) walks the same
    parameter trajectory as the eager fused TrainStep; with deliberately tiny buckets the overflow flag makes the
    captured Adam skip, the host redoes those views through the exact path, and the trajectory is still the same."""
    from curve_gaussian_amd.train_step import GraphedTrainStep, TrainStep
    torch.manual_seed(0)
    gm_a, cams, gts = _train_fixture()
    torch.manual_seed(0)
    gm_b, _, _ = _train_fixture()
    torch.manual_seed(0)
    gm_c, _, _ = _train_fixture()
    n = 12
    eager = TrainStep(gm_a, cams, gts, seed=3)
    la = [float(eager.step()[0]) for _ in range(n)]
    graphed = GraphedTrainStep(gm_b, cams, gts, seed=3)
    lb = []
    for _ in range(n):
        lb.append(graphed.step()[0])
    graphed.finish()
    lb = [float(x) for x in lb[-1:]]
    assert graphed.recaptures == 1 and not graphed._inflight
    tol = dict(rtol=2e-4, atol=2e-6)
    np.testing.assert_allclose(lb[-1], la[-1], rtol=1e-4)
    for name in ("_curve_points", "_width", "_opacity"):
        np.testing.assert_allclose(getattr(gm_b, name).detach().cpu().numpy(), getattr(gm_a, name).detach().cpu().numpy(), **tol)
    np.testing.assert_allclose(gm_b._xyz.detach().cpu().numpy(), gm_a._xyz.detach().cpu().numpy(), **tol)
    # overflow: 64-slot buckets are far too small for this scene -> every captured step is skipped and redone eagerly
    tiny = GraphedTrainStep(gm_c, cams, gts, seed=3)
    tiny._cap = 64
    tiny._probe_capacity = lambda: 64
    for _ in range(n):
        tiny.step()
    tiny.finish()
    assert tiny.recaptures > 1 and gm_c.optimizer.step_count == n   # every view applied exactly once
    for name in ("_curve_points", "_width", "_opacity"):
        np.testing.assert_allclose(getattr(gm_c, name).detach().cpu().numpy(), getattr(gm_a, name).detach().cpu().numpy(), **tol)


def test_flat_adam_matches_torch_adam():
    """cgs_adam_step_flat == torch.optim.Adam over the reference's parameter groups (per-group lr, eps=1e-15)."""
    from curve_gaussian_amd.ops.optim import FlatAdam
    from curve_gaussian_amd.view_parallel import FlatGrads
    g = torch.Generator().manual_seed(0)
    shapes = {"curve_points": (50, 4, 3), "width": (50, 1), "opacity": (50, 1), "mask": (50, 12, 1)}
    lrs = {"curve_points": 5e-4, "width": 5e-3, "opacity": 2.5e-2, "mask": 1e-2}
    init = {k: torch.randn(*s, generator=g) for k, s in shapes.items()}
    ref_p = {k: torch.nn.Parameter(v.clone()) for k, v in init.items()}
    ref_opt = torch.optim.Adam([{"params": [p], "lr": lrs[k], "name": k} for k, p in ref_p.items()], lr=0.0, eps=1e-15)
    hp = {k: torch.nn.Parameter(v.clone().to(DEV)) for k, v in init.items()}
    fg = FlatGrads(hp)
    opt = FlatAdam(hp, lrs, fg, eps=1e-15)
    for it in range(5):
        if it == 3:   # learning-rate schedule through param_groups, like update_learning_rate
            ref_opt.param_groups[0]["lr"] = 1e-4
            opt.param_groups[0]["lr"] = 1e-4
        grads = {k: torch.randn(*s, generator=g) * (10.0 ** (it - 2)) for k, s in shapes.items()}
        for k in shapes:
            ref_p[k].grad = grads[k].clone()
            fg.view(k).copy_(grads[k].to(DEV))
        ref_opt.step()
        opt.step(zero_grad=(it % 2 == 1))
        assert (float(fg.flat.abs().max()) == 0.0) == (it % 2 == 1)   # zero_grad folded into the Adam launch
    for k in shapes:
        np.testing.assert_allclose(hp[k].detach().cpu().numpy(), ref_p[k].detach().numpy(), rtol=2e-5, atol=1e-7)
        assert hp[k].data_ptr() >= opt.flat.data_ptr()  # parameters are views of the flat buffer


def test_photometric_loss_indexed_picks_the_view_on_the_device():
    """cgs_photometric_loss_indexed(gt_stack, n_pos_table, *view_index) == cgs_photometric_loss(gt_stack[v], n_pos[v]),
    bit for bit, for every v, with the index changed between calls through device memory only."""
    import ctypes as C
    from curve_gaussian_amd import _lib as L
    lib = L.load()
    H, W, V = 70, 93, 3
    g = torch.Generator().manual_seed(9)
    img = (torch.rand(1, H, W, generator=g) * 1.4 - 0.2).to(DEV)
    stack = ((torch.rand(V, H, W, generator=g) > 0.9).float() * torch.rand(V, H, W, generator=g)).to(DEV).contiguous()
    table = torch.zeros(V, dtype=torch.int32, device=DEV)
    s = L.raw_stream(torch.device(DEV))
    for v in range(V):
        L.check(lib.cgs_edge_count(1, H, W, L.ptr(stack[v]), C.c_float(0.1), L.ptr(table[v:v + 1]), s), "edge_count")
    ws = torch.zeros(int(lib.cgs_photometric_workspace_bytes(H, W)), dtype=torch.uint8, device=DEV)
    idx = torch.zeros(1, dtype=torch.int32, device=DEV)
    for v in (2, 0, 1):
        idx.fill_(v)
        g_i, l_i = torch.empty(1, H, W, device=DEV), torch.zeros((), device=DEV)
        g_p, l_p = torch.empty(1, H, W, device=DEV), torch.zeros((), device=DEV)
        L.check(lib.cgs_photometric_loss_indexed(H, W, L.ptr(img), L.ptr(stack), L.ptr(idx), C.c_float(0.1), L.ptr(table),
                                                 C.c_float(9.0), C.c_float(1.0), 1, L.ptr(ws), L.ptr(g_i), L.ptr(l_i), s),
                "photometric_loss_indexed")
        L.check(lib.cgs_photometric_loss(H, W, L.ptr(img), L.ptr(stack[v]), C.c_float(0.1), L.ptr(table[v:v + 1]),
                                         C.c_float(9.0), C.c_float(1.0), 1, L.ptr(ws), L.ptr(g_p), L.ptr(l_p), s),
                "photometric_loss")
        torch.cuda.synchronize()
        assert torch.equal(g_i, g_p), v
        assert float(l_i) == float(l_p) and float(l_i) > 0, v


@pytest.mark.parametrize("clamp", [False, True])
def test_photometric_loss_equals_composition(clamp):
    """cgs_photometric_loss == lambda_mse ((1-l) edge_aware_loss + l (1 - fused_ssim)) composed from the drop-in ops
    (themselves pinned to reference goldens), with and without render()'s clamp folded in; value, gradient, the clamp's
    gradient mask, and repeated calls on the same self-cleaning workspace."""
    from curve_gaussian_amd.fused_ssim import fused_ssim
    from curve_gaussian_amd.ops.losses import edge_aware_loss, photometric_loss
    g = torch.Generator().manual_seed(4)
    img = torch.rand(1, 70, 93, generator=g) * (1.6 if clamp else 1.0) - (0.3 if clamp else 0.0)  # some pixels outside [0,1]
    gt = (torch.rand(1, 70, 93, generator=g) > 0.9).float() * torch.rand(1, 70, 93, generator=g)
    gt_d = gt.to(DEV)
    a = img.to(DEV).requires_grad_(True)
    x = a.clamp(0, 1) if clamp else a
    ref = 10.0 * (0.9 * edge_aware_loss(x, gt_d) + 0.1 * (1.0 - fused_ssim(x.unsqueeze(0), gt_d.unsqueeze(0))))
    ref.backward()
    for rep in range(3):
        b = img.to(DEV).requires_grad_(True)
        val = photometric_loss(b, gt_d, 10.0, 0.1, clamp=clamp)
        (2.0 * val).backward()
        np.testing.assert_allclose(float(val), float(ref), rtol=1e-5)
        np.testing.assert_allclose(b.grad.cpu().numpy(), 2.0 * a.grad.cpu().numpy(), rtol=1e-4, atol=2e-6)
    if clamp:
        outside = ((img < 0) | (img > 1)).numpy()
        assert outside.any() and (b.grad.cpu().numpy()[outside] == 0).all()


def test_cfg1_plumbing_scan_on_disk_to_parametric_edges(tmp_path):
    """BASELINE cfg1 end to end without the reference's loaders: a synthetic EMAP-format scan is written to disk
    (meta_data.json + edge_DexiNed/*.png), read back with scene.dataset_io, trained for a few iterations on the HIP
    path (graphed train step), and the curves are written out as parametric_edges.json / edge_points.ply."""
    import json
    from curve_gaussian_amd.gaussian_renderer import PipelineParams, render
    from curve_gaussian_amd.scene import GaussianCurveModel, dataset_io as IO
    from curve_gaussian_amd.train_step import GraphedTrainStep
    H = W = 160
    curves = S.make_curves(417, 1)
    cams = S.fibonacci_cameras(6, H, W)
    tgt = GaussianCurveModel(0, 12, device=DEV).create_from_curves(curves["curve_points"], curves["width"], curves["opacity"],
                                                                   curves["mask"], curves["is_bezier"])
    with torch.no_grad():
        maps = [render(c.to(DEV), tgt, PipelineParams(), torch.zeros(3, device=DEV))["render"].cpu() for c in cams]
    IO.write_emap(str(tmp_path / "scan"), cams, maps)
    loaded = [c.to(DEV) for c in IO.read_emap(str(tmp_path / "scan"))]
    assert len(loaded) == 6 and loaded[0].original_image.shape == (3, H, W)
    for a, b in zip(cams, loaded):
        np.testing.assert_allclose(b.full_proj_transform.cpu().numpy(), a.full_proj_transform.numpy(), atol=2e-5)
    # start from perturbed curves and fit the loaded edge maps (train.py uses channel 0 of the edge map)
    start = {k: v.clone() for k, v in curves.items()}
    start["curve_points"] = start["curve_points"] + 0.004 * torch.randn(start["curve_points"].shape, generator=torch.Generator().manual_seed(2))
    gm = GaussianCurveModel(0, 12, device=DEV).create_from_curves(start["curve_points"], start["width"], start["opacity"],
                                                                  start["mask"], start["is_bezier"])
    ts = GraphedTrainStep(gm, loaded, [c.original_image[:1].contiguous() for c in loaded], seed=0)
    losses = []
    for it in range(40):
        l, _ = ts.step()
        if it % 10 == 0 or it == 39:
            losses.append(float(l))
    ts.finish()
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    edge_dict, pts = IO.write_parametric_edges(gm, str(tmp_path / "out"))
    saved = json.load(open(tmp_path / "out" / "parametric_edges.json"))
    assert np.array(saved["curves_ctl_pts"]).shape == (417, 4, 3) and saved["lines_end_pts"] == []
    assert len(pts) > 417 and os.path.getsize(tmp_path / "out" / "edge_points.ply") > 0
    np.testing.assert_allclose(np.array(saved["curves_ctl_pts"]), gm._curve_points.detach().cpu().numpy(), rtol=1e-6)


def test_scene_builds_the_model_from_a_scan_like_the_reference(tmp_path):
    """scene/__init__.py:27-92 for an EMAP scan: cameras from meta_data.json, the 15^3 seed grid, create_from_pcd (HIP
    distCUDA2) -- then the reference's training_setup and a few eager iterations on the HIP path."""
    from curve_gaussian_amd.gaussian_renderer import PipelineParams, render
    from curve_gaussian_amd.scene import GaussianCurveModel, Scene, dataset_io as IO
    from curve_gaussian_amd.train_step import TrainStep
    H = W = 128
    cams = S.fibonacci_cameras(4, H, W)
    g = torch.Generator().manual_seed(0)
    maps = [(torch.rand(1, H, W, generator=g) > 0.97).float() for _ in cams]
    IO.write_emap(str(tmp_path / "scan"), cams, maps)
    gm = GaussianCurveModel(0, 12, device=DEV)
    scene = Scene(str(tmp_path / "scan"), gm, rng=np.random.default_rng(0), device=DEV)
    assert gm._curve_points.shape == (3375, 4, 3) and gm._xyz.shape == (3375 * 12, 3)
    assert len(scene.getTrainCameras()) == 4 and gm.exposure_mapping == {"0_colors": 0, "1_colors": 1, "2_colors": 2, "3_colors": 3}
    centres = np.stack([c.camera_center.numpy() for c in cams])
    np.testing.assert_allclose(scene.cameras_extent, 1.1 * np.linalg.norm(centres - centres.mean(0), axis=1).max(), rtol=1e-5)
    out = render(scene.getTrainCameras()[0], gm, PipelineParams(), torch.zeros(3, device=DEV))
    assert out["render"].shape == (1, H, W) and float(out["render"].max()) > 0
    ts = TrainStep(gm, scene.getTrainCameras(), [c.original_image[:1].contiguous() for c in scene.getTrainCameras()], seed=0)
    l0 = float(ts.step()[0])
    for _ in range(5):
        l = float(ts.step()[0])
    assert np.isfinite([l0, l]).all()
    assert gm.xyz_gradient_accum.shape == (3375 * 12, 1)


def test_regularisers_match_the_reference_formulas():
    """ops/regularizers.py (sync-free masked means) against train.py:113-131 written out literally with its host-side
    conditions, values and gradients; then the eager and the graphed train step with regularisers on agree."""
    import torch.nn.functional as F
    from curve_gaussian_amd.gaussian_renderer import PipelineParams, render
    from curve_gaussian_amd.ops import regularizers as RG
    from curve_gaussian_amd.train_step import GraphedTrainStep, TrainStep
    gm, cams, gts = _train_fixture()
    with torch.no_grad():
        gm._width[::3] += 0.4          # some curves above the 0.005 width threshold, some below
    gm.prepare_scaling_rot()
    radii = torch.zeros(gm._xyz.shape[0], dtype=torch.int32, device=DEV)
    radii[::2] = 3
    names = ("_curve_points", "_width", "_opacity")

    def grads(loss):
        for n in names:
            getattr(gm, n).grad = None
        loss.backward()
        out = [getattr(gm, n).grad for n in names]
        gm.prepare_scaling_rot()
        return [None if g is None else g.detach().clone() for g in out]

    # literal reference
    vis = (radii > 0).nonzero()
    ref = 0
    if vis.sum() > 0:
        opacity = gm.get_opacity[vis]
        ref = ref + 0.01 * torch.log(1 + opacity ** 2 / 0.5).mean()
    if vis.sum() > 0:
        d = gm.get_rotation_matrix[..., 0].reshape(-1, 12, 3)
        ref = ref + 0.1 * (1 - F.cosine_similarity(d[:, :-1, :], d[:, 1:, :], dim=-1).abs()).mean()
    mask = gm.get_curve_width >= 0.005
    assert bool(mask.any()) and not bool(mask.all())
    ref = ref + 0.01 * (gm.get_curve_width[mask] - 0.005).mean()
    g_ref = grads(ref)
    mine = RG.opacity_loss(gm, radii, 0.01) + RG.curve_smoothness_loss(gm, radii, 0.1) + RG.width_loss(gm, 0.01)
    np.testing.assert_allclose(float(mine), float(ref), rtol=1e-6)
    for a, b in zip(grads(mine), g_ref):
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=1e-5, atol=1e-9)
    # the fused HIP op (cgs_curve_regularizers) against the same reference, incl. a device-side opacity gate
    for gate in (1.0, torch.ones((), device=DEV), 0.0):
        fused = RG.curve_regularizers(gm, radii, 0.01, gate, 0.1, 0.01)
        if float(gate) == 1.0:
            np.testing.assert_allclose(float(fused), float(ref), rtol=2e-5)
            for a, b, n in zip(grads(fused), g_ref, names):
                np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=2e-4, atol=1e-8, err_msg="fused " + n)
        else:
            no_op = RG.curve_smoothness_loss(gm, radii, 0.1) + RG.width_loss(gm, 0.01)
            np.testing.assert_allclose(float(fused), float(no_op), rtol=2e-5)
    assert float(RG.curve_regularizers(gm, torch.zeros_like(radii), 0.01, 1.0, 0.1, 0.0)) == 0.0   # nothing visible
    # nothing visible / nothing above the threshold: the conditional terms vanish instead of dividing by zero
    none = torch.zeros_like(radii)
    assert float(RG.opacity_loss(gm, none)) == 0.0 and float(RG.curve_smoothness_loss(gm, none)) == 0.0
    with torch.no_grad():
        gm._width.fill_(-9.0)
    assert float(RG.width_loss(gm)) == 0.0
    # train.py:74-76,114: reset_timestep is incremented at the top of every iteration, so the opacity term is part of
    # the loss from the FIRST iteration: default regularisers=True step == photometric loss + the literal formulas
    torch.manual_seed(0); g0, cams0, gts0 = _train_fixture()
    torch.manual_seed(0); g1, _, _ = _train_fixture()
    with torch.no_grad():
        rad0 = render(cams0[0], g1, PipelineParams(), torch.zeros(3, device=DEV))["radii"]
        want = (RG.opacity_loss(g1, rad0, 0.01) + RG.curve_smoothness_loss(g1, rad0, 0.1) + RG.width_loss(g1, 0.01))
    plain = TrainStep(g0, cams0, gts0, seed=4).step(view_index=0)[0]
    with_regs = TrainStep(g1, cams0, gts0, seed=4, regularisers=True)
    assert with_regs.reset_timestep == 0
    l_regs = with_regs.step(view_index=0)[0]
    assert with_regs.reset_timestep == 1 and float(want) > 0
    np.testing.assert_allclose(float(l_regs) - float(plain), float(want), rtol=2e-3, atol=1e-7)
    # eager vs graphed step with the regularisers switched on
    torch.manual_seed(0); ga, cams, gts = _train_fixture()
    torch.manual_seed(0); gb, _, _ = _train_fixture()
    ea = TrainStep(ga, cams, gts, seed=4, regularisers=True)
    gs = GraphedTrainStep(gb, cams, gts, seed=4, regularisers=True)
    ea.reset_timestep = gs.reset_timestep = -4            # (a resumed counter: the gate opens at the fifth iteration,
    for it in range(8):                                   #  on the device, without a re-capture)
        la = ea.step()[0]
        lb = gs.step()[0]
    gs.finish()
    assert gs.recaptures == 1
    np.testing.assert_allclose(float(lb), float(la), rtol=1e-4)
    for n in names:
        np.testing.assert_allclose(getattr(gb, n).detach().cpu().numpy(), getattr(ga, n).detach().cpu().numpy(), rtol=1e-3, atol=1e-5)   # 8 Adam steps amplify rounding


@pytest.mark.parametrize("regs", [False, True])
def test_graphed_train_step_autograd_body_matches_direct_body(regs):
    """GraphedTrainStep(direct=False) captures the Python-autograd sequence, direct=True (default) the same kernels
    called through the C ABI with gradients written straight into the flat buffer: identical trajectories."""
    from curve_gaussian_amd.train_step import GraphedTrainStep
    torch.manual_seed(0); ga, cams, gts = _train_fixture()
    torch.manual_seed(0); gb, _, _ = _train_fixture()
    sa = GraphedTrainStep(ga, cams, gts, seed=8, direct=False, regularisers=regs, densify_until_iter=6)
    sb = GraphedTrainStep(gb, cams, gts, seed=8, direct=True, regularisers=regs, densify_until_iter=6)
    sa.reset_timestep = sb.reset_timestep = -3
    for it in range(10):
        la, lb = sa.step()[0], sb.step()[0]
    sa.finish(); sb.finish()
    np.testing.assert_allclose(float(lb), float(la), rtol=1e-4)
    for n in ("_curve_points", "_width", "_opacity", "_mask"):
        np.testing.assert_allclose(getattr(gb, n).detach().cpu().numpy(), getattr(ga, n).detach().cpu().numpy(),
                                   rtol=1e-3, atol=1e-5, err_msg=n)
    assert sb.last["radii"].shape[0] == gb._curve_points.shape[0] * 12 and torch.isfinite(sb.last["dL_dmeans2D"]).all()


@pytest.mark.parametrize("regs", [False, True])
def test_fused_view_entry_points_match_the_separate_calls(regs):
    """cgs_view_forward / cgs_view_backward (per-splat chains fused, csrc/view.hip) against the same iteration built from
    cgs_sample_curves_* / cgs_splat_attrs_* / cgs_rasterize_*: identical trajectories, through the mask phase
    (densify_until_iter = 5) and with straight segments in the model."""
    from curve_gaussian_amd.train_step import GraphedTrainStep
    torch.manual_seed(0); ga, cams, gts = _train_fixture()
    torch.manual_seed(0); gb, _, _ = _train_fixture()
    assert not bool(ga.is_bezier.all())
    sa = GraphedTrainStep(ga, cams, gts, seed=8, fused_view=False, regularisers=regs, densify_until_iter=5)
    sb = GraphedTrainStep(gb, cams, gts, seed=8, fused_view=True, regularisers=regs, densify_until_iter=5)
    for it in range(9):
        la, lb = sa.step()[0], sb.step()[0]
        if it in (0, 3, 8):
            np.testing.assert_allclose(float(lb), float(la), rtol=2e-5)
            np.testing.assert_allclose(sb.last["dL_dmeans2D"].cpu().numpy(), sa.last["dL_dmeans2D"].cpu().numpy(), rtol=1e-4, atol=2e-6)
            assert torch.equal(sb.last["radii"], sa.last["radii"])
            # first iteration: same parameters, same image; later the two Adam trajectories differ in the last bits
            # (atomics order, divide / sqrt rounding of the two builds) and a few alpha < 1/255 tests flip
            assert_close("render", sb.last["render"].cpu().numpy(), sa.last["render"].cpu().numpy(), rel=2e-5 if it == 0 else 1e-4,
                         outlier_frac=0.0 if it == 0 else 5e-3)
    sa.finish(); sb.finish()
    for n in ("_curve_points", "_width", "_opacity", "_mask"):
        np.testing.assert_allclose(getattr(gb, n).detach().cpu().numpy(), getattr(ga, n).detach().cpu().numpy(),
                                   rtol=2e-4, atol=2e-6, err_msg=n)


class _ViewCalls:
    """cgs_view_forward / cgs_view_backward through ctypes on caller-owned buffers, the way bench.py and GraphedTrainStep
    call them (no autograd)."""

    def __init__(self, cp, width, opacity, is_bezier, cam, cap, colors=None, bg=0.0, mask=None, m=12):
        import ctypes as C
        from curve_gaussian_amd import _lib as L
        from curve_gaussian_amd.ops import curve_sampling
        self.L, self.C, self.lib = L, C, L.load()
        lib = self.lib
        self.cam = cam.to(DEV)
        self.B, self.m = cp.shape[0], m
        self.P = self.B * self.m
        self.H, self.W = cam.image_height, cam.image_width
        tiles = ((self.W + 15) // 16) * ((self.H + 15) // 16)
        self.cap = cap
        self.tf = tanfov(cam)
        u8 = lambda n: torch.zeros(int(n), dtype=torch.uint8, device=DEV)
        self.f32 = lambda *sh: torch.zeros(*sh, dtype=torch.float32, device=DEV)
        self.cp, self.w, self.op = (t.detach().to(DEV).contiguous() for t in (cp, width, opacity))
        self.colors = None if colors is None else colors.detach().to(DEV).float().contiguous()   # [P] (None: unit colours)
        self.mask = None if mask is None else mask.detach().to(DEV).float().contiguous()         # [B,m,1] logits (use_mask)
        self.isb = curve_sampling._bezier_mask(is_bezier.to(DEV), DEV)
        self.coef = curve_sampling.sample_coefficients(self.m, DEV)
        self.norms = torch.empty(384, dtype=torch.float64, device=DEV)
        self.geom, self.img = u8(lib.cgs_geometry_bytes(self.P)), u8(lib.cgs_image_bytes(self.W, self.H))
        self.nbin = int(lib.cgs_binning_bytes(cap * tiles))
        self.binb = u8(self.nbin)
        self.color, self.invd, self.omap = self.f32(1, self.H, self.W), self.f32(1, self.H, self.W), self.f32(4, self.H, self.W)
        self.radii = torch.empty(self.P, dtype=torch.int32, device=DEV)
        self.bg = torch.full((3,), float(bg), device=DEV)
        self.scratch = self.f32(int(lib.cgs_view_backward_scratch_floats(self.B, self.m)))
        off = int(lib.cgs_image_status_offset(self.W, self.H))
        self.status = self.img[off:off + 4 * int(lib.cgs_status_words())].view(torch.int32)

    def forward(self, want_splats=False, image_only=False, shared=False):
        """want_splats: also return the model's derived splat tensors (xyz, raw rotation, scaling) the kernels computed;
        image_only: pass neither inverse depth nor all_map (the image-only instance of the unit-colour forward); shared:
        cgs_view_forward_shared (the norm pass was run by cgs_view_shared_begin)."""
        L, lib, pt, cf, cam = self.L, self.lib, self.L.ptr, self.C.c_float, self.cam
        st = L.raw_stream(torch.device(DEV))
        if want_splats:
            self.xyz, self.rot, self.scl = self.f32(self.P, 3), self.f32(self.P, 4), self.f32(self.P, 3)
        sp = (pt(self.xyz), pt(self.rot), pt(self.scl)) if want_splats else (None, None, None)
        fwd = lib.cgs_view_forward_shared if shared else lib.cgs_view_forward
        L.check(fwd(self.B, self.m, pt(self.cp), pt(self.w), pt(self.isb), pt(self.coef), cf(1e-8),
                                     pt(self.norms), pt(self.op), pt(self.mask), cf(0.01), pt(self.colors), pt(self.geom), pt(self.binb),
                                     self.nbin, pt(self.img), self.cap, pt(self.bg), self.W, self.H,
                                     pt(cam.world_view_transform), pt(cam.full_proj_transform), pt(cam.camera_center),
                                     self.tf[0], self.tf[1], pt(self.color), None if image_only else pt(self.invd),
                                     None if image_only else pt(self.omap), pt(self.radii), *sp, st), "cgs_view_forward")
        torch.cuda.synchronize()
        assert int(self.status[2]) == 0, "bucket overflow: raise cap"

    def final_T(self):
        """[H,W] final transmittance the forward left in the image buffer (first carve-out, csrc/common.h)."""
        return self.img[:4 * self.H * self.W].view(torch.float32).reshape(self.H, self.W).clone()

    def backward(self, dimg, g_cp, g_w, g_op, accumulate, g_mask=None):
        L, lib, pt, cf, cam = self.L, self.lib, self.L.ptr, self.C.c_float, self.cam
        st = L.raw_stream(torch.device(DEV))
        g_m2d = self.f32(self.P, 3)
        L.check(lib.cgs_view_backward(self.B, self.m, pt(self.cp), pt(self.w), pt(self.isb), pt(self.coef), cf(1e-8),
                                      pt(self.norms), pt(self.op), pt(self.mask), cf(0.01), pt(self.colors), pt(self.geom), pt(self.binb),
                                      pt(self.img), pt(self.bg), self.W, self.H, pt(cam.world_view_transform),
                                      pt(cam.full_proj_transform), pt(cam.camera_center), self.tf[0], self.tf[1],
                                      pt(self.radii), pt(dimg), None, pt(g_m2d), pt(g_cp), pt(g_w), pt(g_op), pt(g_mask),
                                      pt(self.scratch), accumulate, st), "cgs_view_backward")
        torch.cuda.synchronize()
        return g_m2d


def test_view_backward_accumulate_flag_adds_to_the_gradient_buffers():
    """cgs_view_backward(accumulate = 0) overwrites the curve-parameter gradients, accumulate = 1 adds to them (the
    view-batch schedule of bench.py sums the views of one optimizer step in place): two accumulating calls on zeroed
    buffers give twice one overwriting call, and an overwriting call forgets what the buffers held."""
    gm, c, cam = _model(300, 7)
    vc = _ViewCalls(gm._curve_points, gm._width, gm._opacity, gm.is_bezier, cam, 1024)
    B, f32 = vc.B, vc.f32
    dimg = torch.randn(1, vc.H, vc.W, generator=torch.Generator().manual_seed(3)).to(DEV)
    vc.forward()
    once = [f32(B, 4, 3), f32(B, 1), f32(B, 1)]
    vc.backward(dimg, *once, 0)
    assert float(once[0].abs().max()) > 0
    dirty = [f32(B, 4, 3), f32(B, 1), f32(B, 1)]
    for t in dirty:
        t.fill_(1e6)                        # overwritten, not added to
    vc.backward(dimg, *dirty, 0)
    # float atomics in the compositor make two passes differ in the last bits, and the curve-sampling backward amplifies
    # that (cancellation between the samples of one curve): compare in relative L2, as bench.py does for its step gradient
    rel_l2 = lambda got, want: float((got - want).norm() / want.norm())
    for a, b in zip(once, dirty):
        assert rel_l2(b, a) < 1e-3
    twice = [f32(B, 4, 3), f32(B, 1), f32(B, 1)]
    vc.backward(dimg, *twice, 1)
    vc.backward(dimg, *twice, 1)
    for name, a, b in zip(("curve_points", "width", "opacity"), once, twice):
        assert rel_l2(b, 2.0 * a) < 1e-3, name


@pytest.mark.parametrize("cfg,coloured,bg", [("cfg1", False, 0.0), ("cfg3", False, 0.0), ("cfg1", True, 0.0), ("cfg2", True, 0.0),
                                              ("cfg2", False, 0.35), ("cfg1", True, 0.35), ("cfg5", False, 0.0)])
def test_view_entry_points_match_the_oracle_chain_at_full_size(cfg, coloured, bg):
    """The whole per-view path of a BASELINE config through its two C-ABI calls -- curve tensors in, image out; image
    gradient in, curve-parameter gradients out -- against the chain of oracles: torch restatement of prepare_scaling_rot /
    get_rotation / get_opacity / all_map (autograd for their backward) around the C rasterizer oracle's forward and
    backward.  Image under the rasterizer criterion (1e-4 of max, flip budget); curve-parameter gradients in relative L2
    (the sampling backward sums 12 samples per curve with cancellation: element-wise noise of a few 1e-4 of max from the
    compositor's atomics order alone, see test_view_backward_accumulate_flag...).  Without colors_precomp the entry points
    run the unit-colour instances of the compositors (closed-form sums), with it the general ones."""
    curves, cams = S.make_config(cfg, n_views=1)
    cam = cams[0]
    H, W = cam.image_height, cam.image_width
    leaves = [curves[k].clone().requires_grad_(True) for k in ("curve_points", "width", "opacity")]
    cp, wd, op = leaves
    xyz, rot, scl = TR.prepare_scaling_rot(cp, wd, curves["is_bezier"])
    P = xyz.shape[0]
    rotn = torch.nn.functional.normalize(rot)
    opac = torch.sigmoid(op).repeat_interleave(12, 0)
    amap = TR.build_all_map(rot.detach(), xyz.detach(), cam.camera_center, cam.world_view_transform).float().contiguous()
    tfx, tfy = tanfov(cam)
    n = lambda t: np.ascontiguousarray(t.detach().numpy())
    colors = 0.2 + 0.8 * torch.rand(P, 1, generator=torch.Generator().manual_seed(5)) if coloured else torch.ones(P, 1)
    fw = ORA.forward(np.full(3, bg, np.float32), n(xyz), n(colors), n(opac), n(scl), n(rotn), 1.0, None,
                     n(amap), n(cam.world_view_transform), n(cam.full_proj_transform), tfx, tfy, H, W, None, 0,
                     n(cam.camera_center))
    dimg = torch.randn(1, H, W, generator=torch.Generator().manual_seed(17))
    gr = ORA.backward(fw, dimg.numpy(), None, None)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float32))
    chain = ((xyz * t(gr["dL_dmeans3D"])).sum() + (scl * t(gr["dL_dscales"])).sum()
             + (rotn * t(gr["dL_drotations"])).sum() + (opac * t(gr["dL_dopacity"])).sum())
    chain.backward()
    # ---- product
    # cfg5 (1 M splats, a third of the pixels terminated early): lists beyond the in-kernel sort's capacity -> separate sort
    vc = _ViewCalls(curves["curve_points"], curves["width"], curves["opacity"], curves["is_bezier"], cam,
                    4096 if cfg == "cfg5" else 1024, colors=colors.reshape(-1) if coloured else None, bg=bg)
    vc.forward()
    # magnitude cap of the outliers: the two sides' splats differ in their last bits here, so a handful of radii differ by one
    # pixel -- and the reference's 3-sigma tile rect cuts a splat off at alpha = opacity exp(-4.5) = 6.7e-3 (> 1/255): a pixel
    # at that rim gains or loses up to 6.7e-3 (identical-input tests keep the 5e-3 default: one 1/255 flip)
    # (no cluster criterion either: a splat missing from one tile's list moves that tile's whole rim)
    assert_close("color", vc.color.cpu().numpy(), fw.color, max_outlier=1.2e-2, tile_cluster=None)
    assert_close("all_map", vc.omap.cpu().numpy(), fw.out_all_map, outlier_frac=2e-4, max_outlier=1.2e-2, tile_cluster=None)
    assert (vc.radii.cpu().numpy() == fw.radii).mean() > 0.9999
    B = vc.B
    g = [vc.f32(B, 4, 3), vc.f32(B, 1), vc.f32(B, 1)]
    g_m2d = vc.backward(dimg.to(DEV), *g, 0)
    # the rasterizer's inputs are not bit-identical on the two sides (HIP vs torch sampling arithmetic: a few ulp in
    # means / scales / rotations), so a small fraction of the per-splat screen-space gradients moves by ~1e-3 of max --
    # same allowance as test_render_matches_oracle_composition; the relative L2 error bounds the rest
    want = torch.from_numpy(gr["dL_dmeans2D"])
    # cfg5: EVERY pixel of the view terminates early (T < 1e-4), and which splat terminates a pixel flips under the few-ulp
    # input differences far more often than anything else does; the unit-colour and the general instances land on the
    # same 2.8e-3 relative L2 distance from the oracle and 4.9e-5 from each other (scratch diagnosis, round 2)
    tol = 6e-3 if cfg == "cfg5" else 1e-3
    assert_close("dL_dmeans2D", g_m2d.cpu().numpy(), gr["dL_dmeans2D"], abs_floor=1e-6, outlier_frac=4e-2 if cfg == "cfg5" else 5e-3)
    rel = float((g_m2d.cpu() - want).norm() / want.norm())
    print(f"{cfg}: dL_dmeans2D relative L2 {rel:.2e}; pixels with T_final < 1e-2: {float((torch.from_numpy(fw.final_T) < 1e-2).float().mean()):.3f}")
    assert rel < tol
    for name, got, leaf in zip(("curve_points", "width", "opacity"), g, leaves):
        want = leaf.grad
        rel = float((got.cpu() - want).norm() / want.norm())
        print(f"{cfg}: dL/d{name} relative L2 {rel:.2e}")
        assert rel < tol, f"dL/d{name}: relative L2 error {rel:.2e}"
    fw.free()


def _opaque(curves):
    """Every third curve nearly opaque (0.995 / 0.9995): alpha reaches the reference's 0.99 clamp (forward.cu:368), which the
    clamp-free walk of the pair-major backward must not be used for."""
    c = dict(curves)
    op = c["opacity"].clone()
    op[0::3] = float(np.log(0.995 / 0.005))
    op[1::6] = float(np.log(0.9995 / 0.0005))
    c["opacity"] = op
    return c


@pytest.mark.parametrize("cfg,bg,opaque", [("cfg1", 0.0, False), ("cfg2", 0.35, False), ("cfg3", 0.0, False), ("cfg3", 0.35, False),
                                            ("cfg4", 0.0, False), ("cfg5", 0.0, False), ("cfg2", 0.0, True), ("cfg1", 0.35, True)])
def test_headline_instances_meet_the_raster_criterion_on_identical_inputs(cfg, bg, opaque):
    """The kernel instances bench.py times (cgs_view_forward / cgs_view_backward without colors_precomp: unit-colour forward
    with the in-kernel tile sort, pair-major unit-colour backward) held to the SAME criterion as the general rasterizer
    instances in test_raster_gpu.py: the splat tensors the fused forward computed (xyz, raw rotation, scaling) are read back
    and handed to oracle/raster_ref.c -- together with the oracle-side normalisation, opacity and all_map -- so both
    compositors see the same splats up to the last bits of one normalisation; image, all_map and dL/dmeans2D then have to
    agree to 1e-4 of the tensor's maximum on all but 1e-4 of the elements (assert_close defaults), radii exactly up to +-1 on
    <= 1e-5 of the splats.  The curve-parameter gradients are compared with the torch pull-back of the ORACLE's per-splat
    gradients through the restated sampling graph, in relative L2 (the sampling backward sums 12 samples per curve with
    cancellation; two runs of the same kernels differ by 1e-4 from the order of the compositor's float atomics alone)."""
    curves, cams = S.make_config(cfg, n_views=1)
    if opaque:
        curves = _opaque(curves)
    cam = cams[0]
    H, W = cam.image_height, cam.image_width
    vc = _ViewCalls(curves["curve_points"], curves["width"], curves["opacity"], curves["is_bezier"], cam,
                    4096 if cfg == "cfg5" else 1024, bg=bg)
    vc.forward(want_splats=True)
    xyz_h, rot_h, scl_h = vc.xyz.cpu(), vc.rot.cpu(), vc.scl.cpu()
    P = xyz_h.shape[0]
    rotn_h = torch.nn.functional.normalize(rot_h)
    opac = torch.sigmoid(curves["opacity"]).repeat_interleave(12, 0)
    amap = TR.build_all_map(rot_h, xyz_h, cam.camera_center, cam.world_view_transform).float().contiguous()
    tfx, tfy = tanfov(cam)
    n = lambda t: np.ascontiguousarray(t.detach().numpy())
    fw = ORA.forward(np.full(3, bg, np.float32), n(xyz_h), np.ones((P, 1), np.float32), n(opac), n(scl_h), n(rotn_h), 1.0, None,
                     n(amap), n(cam.world_view_transform), n(cam.full_proj_transform), tfx, tfy, H, W, None, 0,
                     n(cam.camera_center))
    radii = vc.radii.cpu().numpy()
    off = radii != fw.radii
    assert off.mean() <= 1e-5 and (np.abs(radii[off] - fw.radii[off]) <= 1).all(), f"radii: {off.sum()} of {P} differ"
    assert_close("color", vc.color.cpu().numpy(), fw.color)
    assert_close("all_map", vc.omap.cpu().numpy(), fw.out_all_map)
    assert_close("invdepth", vc.invd.cpu().numpy(), fw.invdepth)
    dimg = torch.randn(1, H, W, generator=torch.Generator().manual_seed(17))
    # Pixels where the two compositors took a DIFFERENT termination decision (the splat that would push T below 1e-4 is not
    # blended, forward.cu:371-376: under the last bits of the exponent the cut lands one entry earlier or later and the final
    # transmittance jumps by a factor 1 - alpha) carry no upstream gradient on either side: the gradients are compared on the
    # pixels both sides composited alike, and the number of excluded pixels is asserted.  At cfg5 EVERY pixel terminates
    # early; without the exclusion its curve gradients sit at 2e-4 relative L2 instead of the 1e-5 class of the other configs.
    T_h, T_o = vc.final_T().cpu().numpy(), fw.final_T.reshape(H, W)
    flipped = np.abs(T_h - T_o) > 1e-3 * np.abs(T_o) + 1e-9
    print(f"{cfg} bg={bg}: {int(flipped.sum())} of {H * W} pixels took another termination decision ({flipped.mean():.2e})")
    assert flipped.mean() <= 1e-4          # measured: 0 .. 8.2e-6 (cfg3: 21 pixels, cfg5: 32)
    dimg = dimg * torch.from_numpy(~flipped)[None]
    gr = ORA.backward(fw, dimg.numpy(), None, None)
    B = vc.B
    g = [vc.f32(B, 4, 3), vc.f32(B, 1), vc.f32(B, 1)]
    g_m2d = vc.backward(dimg.to(DEV).contiguous(), *g, 0)
    assert_close("dL_dmeans2D", g_m2d.cpu().numpy(), gr["dL_dmeans2D"], abs_floor=1e-6)
    want = torch.from_numpy(gr["dL_dmeans2D"])
    print(f"{cfg} bg={bg}: dL_dmeans2D relative L2 {float((g_m2d.cpu() - want).norm() / want.norm()):.2e}")
    # curve-parameter gradients: the oracle's per-splat gradients pulled back through the restated sampling graph
    leaves = [curves[k].clone().requires_grad_(True) for k in ("curve_points", "width", "opacity")]
    xyz, rot, scl = TR.prepare_scaling_rot(leaves[0], leaves[1], curves["is_bezier"])
    t = lambda a: torch.from_numpy(np.asarray(a, np.float32))
    ((xyz * t(gr["dL_dmeans3D"])).sum() + (scl * t(gr["dL_dscales"])).sum()
     + (torch.nn.functional.normalize(rot) * t(gr["dL_drotations"])).sum()
     + (torch.sigmoid(leaves[2]).repeat_interleave(12, 0) * t(gr["dL_dopacity"])).sum()).backward()
    for name, got, leaf in zip(("curve_points", "width", "opacity"), g, leaves):
        rel = float((got.cpu() - leaf.grad).norm() / leaf.grad.norm())
        print(f"{cfg} bg={bg}: dL/d{name} relative L2 {rel:.2e}")
        # measured 2e-6 .. 8e-6 (cfg1-4)
        # (cfg5, where every pixel terminates early: 7e-5 on the pixels both sides composited alike -- 2.0e-4 before the
        # 32 flipped pixels were excluded)
        assert rel < (1e-4 if cfg == "cfg5" else 3e-5), f"dL/d{name}: relative L2 error {rel:.2e}"
        # element-wise next to the L2 figure: 1e-4 of the tensor's maximum on all but 1e-3 of the curves, no curve beyond
        # 2e-3 of it (measured worst element: <= 5e-5 of the maximum at every config) -- see the printed worst element
        worst = assert_close(f"dL/d{name} (element-wise)", got.cpu().numpy(), leaf.grad.numpy(),
                             outlier_frac=1e-3, max_outlier=2e-3)
        print(f"{cfg} bg={bg}: dL/d{name} worst element {worst:.2e} of max")
    if cfg == "cfg3" and bg == 0.0:
        # the image-only instance of the forward (no inverse depth, no all_map) at a BASELINE size: same image, bit for bit
        full = vc.color.clone()
        vc.forward(image_only=True)
        assert torch.equal(vc.color, full)
    fw.free()


@pytest.mark.parametrize("name", ["small", "lines", "masked"])
def test_view_path_matches_the_frozen_oracle_chain(name):
    """cgs_view_forward / cgs_view_backward (the kernels bench.py's headline times) against tests/golden/view_*.npz: the oracle
    chain curves -> image -> curve-parameter gradients frozen by tests/golden/make_view_golden.py, including straight-line
    curves (is_bezier = False) and the straight-through mask of use_mask.  The CPU suite holds today's oracle to the same
    files (tests/test_view_golden_cpu.py)."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    from make_view_golden import load_scene
    curves, mask, cam, bg, z = load_scene(name)
    vc = _ViewCalls(curves["curve_points"], curves["width"], curves["opacity"], curves["is_bezier"], cam, 1024, bg=bg, mask=mask)
    vc.forward()
    radii = vc.radii.cpu().numpy()
    assert (radii != z["radii"]).mean() <= 1e-3 and np.abs(radii - z["radii"]).max() <= 1
    assert_close("color", vc.color.cpu().numpy(), z["color"], min_outliers=2)
    assert_close("invdepth", vc.invd.cpu().numpy(), z["invdepth"], min_outliers=2)
    assert_close("all_map", vc.omap.cpu().numpy(), z["out_all_map"], min_outliers=8)
    B = vc.B
    g = [vc.f32(B, 4, 3), vc.f32(B, 1), vc.f32(B, 1)]
    g_mask = vc.f32(B, 12, 1) if mask is not None else None
    g_m2d = vc.backward(torch.from_numpy(z["dL_dcolor"]).to(DEV), *g, 0, g_mask)
    assert_close("dL_dmeans2D", g_m2d.cpu().numpy(), z["g_means2D"], abs_floor=1e-6, outlier_frac=2e-3, max_outlier=5e-2)
    pairs = [("curve_points", g[0]), ("width", g[1]), ("opacity", g[2])] + ([("mask", g_mask)] if mask is not None else [])
    for pname, got in pairs:
        want = torch.from_numpy(z["g_" + pname])
        rel = float((got.cpu() - want).norm() / want.norm())
        print(f"view_{name}: dL/d{pname} relative L2 {rel:.2e}")
        # small scenes (a few thousand splats): one alpha >= 1/255 decision taken the other way moves one curve's gradient by
        # per cent of ITS value; the relative L2 over all curves stays in the 1e-4 class (measured: see the printed values)
        assert rel < 5e-4, f"view_{name}: dL/d{pname} relative L2 error {rel:.2e}"


@pytest.mark.parametrize("B,H,W,opaque,wide,ties", [(900, 128, 160, False, 0.0, False), (1000, 96, 128, True, 0.8, False),
                                                     (500, 64, 80, True, 1.0, False), (600, 96, 96, False, 0.3, True)])
def test_bucket_capacity_and_sort_placement_do_not_change_the_view(B, H, W, opaque, wide, ties):
    """The same scene with bucket capacity 1 024 (tile sort INSIDE the unit-colour forward) and with 2 048 / 4 096 (separate
    sort launches, non-sorting forward -- the cfg5 route): images, saved per-pixel state and cuts are bit-identical, the
    gradients agree to float-atomics noise.  Cases: short lists, lists of several batches with early termination (opaque, fat
    splats), equal depths (coincident curves).  (Written for round 6's lazy batch-by-batch ordering of long buckets, which
    passed it bit for bit and lost on time: profiles/r06_experiments.md #6.)"""
    curves = S.make_curves(B, 31 + B)
    curves["width"] = curves["width"] + wide
    if opaque:
        curves = _opaque(curves)
    if ties:   # every curve three times: equal depths in every tile list
        for k in ("curve_points", "width", "opacity", "is_bezier"):
            curves[k] = torch.cat([curves[k][: B // 3]] * 3)
    cam = S.make_camera((0.5, -1.7, 0.9), (0.5, 0.5, 0.5), (0, 0, 1), H, W)
    dimg = torch.randn(1, H, W, generator=torch.Generator().manual_seed(B)).to(DEV)
    outs = {}
    for cap in (1024, 2048, 4096):
        vc = _ViewCalls(curves["curve_points"], curves["width"], curves["opacity"], curves["is_bezier"], cam, cap)
        vc.forward()
        n = curves["curve_points"].shape[0]
        g = [vc.f32(n, 4, 3), vc.f32(n, 1), vc.f32(n, 1)]
        g_m2d = vc.backward(dimg, *g, 0)
        off = (4 * H * W + 127) // 128 * 128
        ncw = vc.img[off:off + 4 * H * W].view(torch.int32).clone()
        outs[cap] = (vc.color.clone(), vc.invd.clone(), vc.omap.clone(), vc.final_T(), ncw, [t.clone() for t in g], g_m2d)
    longest = int((outs[1024][4] & 0x7fffffff).max())
    ref = outs[1024]
    for cap in (2048, 4096):
        o = outs[cap]
        for a, b, name in zip(o[:5], ref[:5], ("color", "invdepth", "all_map", "final_T", "n_contrib")):
            assert torch.equal(a, b), f"cap {cap}: {name} differs from the sorting forward"
        for a, b, name in zip(o[5], ref[5], ("curve_points", "width", "opacity")):
            rel = float((a - b).norm() / b.norm().clamp_min(1e-30))
            assert rel < 1e-3, f"cap {cap}: dL/d{name} relative L2 {rel:.2e}"
    print(f"deepest cut / list position {longest}")
    assert longest > 0


@pytest.mark.parametrize("W,H,B,seed,bg,opaque,wide", [(70, 50, 60, 1, 0.0, False, 0.0), (129, 97, 300, 2, 0.35, False, 0.0),
                                                         (160, 128, 900, 3, 0.0, True, 0.0), (48, 16, 40, 4, 0.0, False, 1.5),
                                                         (333, 211, 2500, 5, 0.2, True, 0.8), (16, 16, 5, 6, 0.0, False, 0.0),
                                                         (64, 48, 110, 7, 0.0, True, 1.5)])
def test_pair_major_backward_matches_pixel_major(W, H, B, seed, bg, opaque, wide):
    """Two independent implementations of the unit-colour view on the same curves: the view path's own instances (unit-colour
    forward with the closed-form sums, pair-major `k_render_bwd_unit`) and the GENERAL instances the same entry points run
    when they are handed an explicit all-ones `colors_precomp` (general forward, untagged lists, pixel-major `k_render_bwd3`
    with the reference's recurrences).  Cases: image sizes that are not multiples of the tile (partial border tiles and
    quadrants), a single tile, tile lists longer than one 256-entry batch (dense small images), grey background, opacities at
    the 0.99 clamp (exact walk instead of the clamp-free one), fat splats that fill whole tiles.  The kernels evaluate the same
    quantities with different exponent roundings (quadrant- vs half-quadrant-centred) and different arithmetic, so they agree
    to threshold flips: relative L2 and the 1e-4-of-max criterion."""
    curves = S.make_curves(B, seed)
    if opaque:
        curves = _opaque(curves)
    if wide:
        curves = dict(curves)
        curves["width"] = curves["width"] + wide          # log-width: e^wide times wider splats
    cam = S.make_camera((0.5, -1.5, 0.8), (0.5, 0.5, 0.5), (0, 0, 1), H, W)
    dimg = torch.randn(1, H, W, generator=torch.Generator().manual_seed(seed)).to(DEV)
    res, img = {}, {}
    for v in (3, 4):   # 3: general instances (explicit unit colours), 4: the view path's unit instances
        # (the last case keeps the capacity within the in-kernel sort's reach, so the SORTING forward stages the batches)
        vc = _ViewCalls(curves["curve_points"], curves["width"], curves["opacity"], curves["is_bezier"], cam,
                        1024 if seed == 7 else 2048, bg=bg, colors=torch.ones(B * 12) if v == 3 else None)
        # poison the binning buffer: every list entry a backward may read has to be WRITTEN by this forward -- batches
        # the forward never stages (every pixel terminated before them: the last case, opaque lists of > 256 entries) keep
        # valid, untagged indices, not whatever the buffer held (the pixel-major kernel stages the whole range)
        vc.binb.fill_(0xFF)
        vc.forward()
        img[v] = (vc.color.cpu().numpy(), vc.invd.cpu().numpy(), vc.omap.cpu().numpy())
        g = [vc.f32(vc.B, 4, 3), vc.f32(vc.B, 1), vc.f32(vc.B, 1)]
        m2d = vc.backward(dimg, *g, 0)
        res[v] = [m2d.cpu().double()] + [t.cpu().double() for t in g]
    assert float(res[3][0].abs().max()) > 0
    if seed == 7:
        longest = int(vc.status[5::2][:256].max())
        assert 256 < longest <= 1024, f"case 7 is meant to have tile lists of several batches (longest {longest})"
    for name, a, b in zip(("color", "invdepth", "all_map"), img[4], img[3]):
        assert_close(name, a, b, abs_floor=1e-7, outlier_frac=1e-3, tile_cluster=None)
    for name, a, b in zip(("dL_dmeans2D", "curve_points", "width", "opacity"), res[4], res[3]):
        rel = float((a - b).norm() / b.norm().clamp_min(1e-30))
        assert rel < 2e-4, f"{name}: relative L2 {rel:.2e}"
    assert_close("dL_dmeans2D", res[4][0].numpy(), res[3][0].numpy(), abs_floor=1e-7, outlier_frac=1e-3)


def test_headline_backward_is_linear_in_the_image_gradient_at_cfg3():
    """Size-independent property of the headline backward (cgs_view_backward, pair-major unit compositor) at the BASELINE size it
    is benchmarked on: the curve-parameter gradients are linear in the upstream image gradient -- g(2 a - 3 b) = 2 g(a) - 3 g(b)
    up to the order of the compositor's float atomics -- and nothing for a zero image gradient (the clamp-free walk divides by
    (E - 1) / K with 1e30 standing in for 1 / 0: 1e-30 per pair instead of an exact zero)."""
    curves, cams = S.make_config("cfg3", n_views=1)
    vc = _ViewCalls(curves["curve_points"], curves["width"], curves["opacity"], curves["is_bezier"], cams[0], 1024)
    gen = torch.Generator().manual_seed(23)
    da = torch.randn(1, vc.H, vc.W, generator=gen).to(DEV)
    db = torch.randn(1, vc.H, vc.W, generator=gen).to(DEV)

    def grads(dimg):
        vc.forward()
        g = [vc.f32(vc.B, 4, 3), vc.f32(vc.B, 1), vc.f32(vc.B, 1)]
        m2d = vc.backward(dimg, *g, 0)
        return [m2d.double()] + [t.double() for t in g]
    ga, gb, gc, gz = grads(da), grads(db), grads(2.0 * da - 3.0 * db), grads(torch.zeros_like(da))
    for name, a, b, c, z in zip(("dL_dmeans2D", "curve_points", "width", "opacity"), ga, gb, gc, gz):
        want = 2.0 * a - 3.0 * b
        rel = float((c - want).norm() / want.norm())
        assert rel < 1e-4, f"{name}: relative L2 {rel:.2e}"
        assert float(z.abs().max()) < 1e-20, name


def test_unit_colour_instances_agree_with_the_general_ones_on_random_scenes():
    """Seeded fuzz of the whole per-view path: cgs_view_forward / cgs_view_backward WITHOUT colors_precomp (unit-colour forward,
    pair-major unit backward) against the same calls WITH an all-ones colors_precomp (general compositor instances) on 16 random
    scenes -- curve counts 40 .. 8 000, odd image sizes, cameras outside, at the rim of and inside the cloud (near culls,
    screen-filling splats), widths up to e^2.5 times the default, opacities from 0.1 to 0.97, black and grey background."""
    import random
    cams_at = [((0.5, -1.6, 0.7), (0.5, 0.5, 0.5), (0, 0, 1)), ((2.0, 1.4, 1.1), (0.4, 0.5, 0.6), (0, 0, 1)),
               ((0.5, 0.5, 0.5), (0.9, 0.2, 0.5), (0, 0, 1)), ((0.5, -0.6, 0.5), (0.5, 0.5, 0.5), (0, 0, 1))]
    # (CGS_FUZZ_SEED / CGS_FUZZ_CASES: longer one-off campaigns; the defaults are the suite's fixed 16 scenes)
    rng = random.Random(int(os.environ.get("CGS_FUZZ_SEED", "3")))
    want = int(os.environ.get("CGS_FUZZ_CASES", "16"))
    done = 0
    for case in range(want * 3 // 2):
        B = rng.choice([40, 150, 600, 2500, 8000])
        H, W = rng.choice([64, 77, 128, 200, 333]), rng.choice([64, 130, 176, 256, 401])
        seed = rng.randrange(10000)
        curves = S.make_curves(B, seed)
        curves["width"] = curves["width"] + rng.choice([0.0, 0.8, 1.6, 2.5])
        curves["opacity"] = curves["opacity"] + rng.choice([-2.0, 0.0, 3.0])
        cam = S.make_camera(*cams_at[rng.randrange(len(cams_at))], H, W)
        bg = rng.choice([0.0, 0.0, 0.4])
        out = {}
        # (the general instances run twice: their own run-to-run difference -- float atomics order, amplified by the cancellation
        # inside the curve-sampling backward -- is the noise floor of the comparison; on a fully opaque 8 000-curve cloud at
        # 64 x 333 it reaches 3e-4 relative L2 for dL/dwidth, elsewhere 1e-9 .. 1e-5)
        for name, colors in (("unit", None), ("general", torch.ones(B * 12)), ("general_again", torch.ones(B * 12))):
            vc = _ViewCalls(curves["curve_points"], curves["width"], curves["opacity"], curves["is_bezier"], cam, 4096, colors=colors, bg=bg)
            try:
                vc.forward()
            except AssertionError:            # tile lists beyond the largest bucket (dense cloud on a tiny image): not this test's subject
                out = None
                break
            g = [vc.f32(B, 4, 3), vc.f32(B, 1), vc.f32(B, 1)]
            dimg = torch.randn(1, H, W, generator=torch.Generator().manual_seed(seed)).to(DEV)
            m2d = vc.backward(dimg, *g, 0)
            out[name] = dict(color=vc.color.clone(), omap=vc.omap.clone(), invd=vc.invd.clone(), radii=vc.radii.clone(), m2d=m2d,
                             g=[t.clone() for t in g])
        if out is None:
            continue
        u, gen = out["unit"], out["general"]
        assert torch.equal(u["radii"], gen["radii"])
        amax = lambda a, b: float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)
        l2 = lambda a, b: float((a - b).norm()) / max(float(b.norm()), 1e-30)
        where = f"case {case}: B={B} {W}x{H} bg={bg} seed={seed}"
        for k in ("color", "omap", "invd"):
            assert amax(u[k], gen[k]) < 2e-5, f"{where}: {k} {amax(u[k], gen[k]):.2e}"
        # dL/dmeans2D per splat: equal up to the alpha >= 1/255 decisions that flip between the two exponent roundings -- one
        # flipped (pixel, splat) pair moves that ONE splat by alpha * |conic d| * T * dL/dpixel * W/2, which on a 150-curve scene
        # is several per cent of the splat (seeds 204 / 215 / 219 of the CGS_FUZZ_SEED campaign: one pair each, alpha within
        # 2e-6 of the threshold, the general instance equal to the oracle to 5e-6) -- so: at most a few such splats, the rest tight
        d_m2d = (u["m2d"] - gen["m2d"]).norm(dim=1)
        moved = d_m2d > 1e-3 * float(gen["m2d"].norm(dim=1).max())
        assert int(moved.sum()) <= max(2, int(2e-3 * int((gen["radii"] > 0).sum()))), f"{where}: {int(moved.sum())} splats moved in dL_dmeans2D"
        assert l2(u["m2d"][~moved], gen["m2d"][~moved]) < 1e-3, f"{where}: dL_dmeans2D {l2(u['m2d'][~moved], gen['m2d'][~moved]):.2e}"
        keep = ~moved.view(B, 12).any(dim=1)          # curves none of whose splats carries a flipped pair
        for name, a, b, b2 in zip(("curve_points", "width", "opacity"), u["g"], gen["g"], out["general_again"]["g"]):
            noise = l2(b2, b)
            # (premise, not parity: a camera inside a cloud of e^2.5-times-wider curves amplifies the raster backward's 3e-6
            # atomics-order noise in dL/dmeans2D two-hundredfold on its way through the sampling backward -- 1e-4 .. 1.1e-3 for
            # dL/dcurve_points and dL/dwidth over six runs of CGS_FUZZ_SEED=6100 case 74, with round 5's kernels as well)
            assert noise < 3e-3, f"{where}: dL/d{name}: the general instances differ from themselves by {noise:.2e}"
            assert l2(a[keep], b[keep]) < 1e-3 + 4.0 * noise and bool(torch.isfinite(a).all()), \
                f"{where}: dL/d{name} {l2(a[keep], b[keep]):.2e} (run-to-run noise of the general instances {noise:.2e})"
        done += 1
        if done == want:
            break
    assert done >= want * 3 // 4


def test_graphed_train_step_image_only_forward_follows_the_same_trajectory():
    """GraphedTrainStep(aux_outputs=False): cgs_view_forward without inverse depth / all_map (the iteration reads `render`
    only, train.py:98-107).  Same image, same parameters after ten iterations as with every output, through the mask phase."""
    from curve_gaussian_amd.train_step import GraphedTrainStep
    torch.manual_seed(0); ga, cams, gts = _train_fixture()
    torch.manual_seed(0); gb, _, _ = _train_fixture()
    sa = GraphedTrainStep(ga, cams, gts, seed=4, densify_until_iter=5)
    sb = GraphedTrainStep(gb, cams, gts, seed=4, densify_until_iter=5, aux_outputs=False)
    for it in range(10):
        la, lb = sa.step()[0], sb.step()[0]
        if it == 0:
            assert torch.equal(sb.last["render"], sa.last["render"]) and sb.last["all_map"] is None
    sa.finish(); sb.finish()
    np.testing.assert_allclose(float(lb), float(la), rtol=2e-5)
    for n in ("_curve_points", "_width", "_opacity", "_mask"):
        np.testing.assert_allclose(getattr(gb, n).detach().cpu().numpy(), getattr(ga, n).detach().cpu().numpy(),
                                   rtol=2e-4, atol=2e-6, err_msg=n)


def test_graphed_train_step_crosses_the_mask_phase():
    """At densify_until_iter the iteration switches to the straight-through curve mask + mask loss (train.py:97,110-111);
    the graphed step re-captures once and keeps following the eager trajectory."""
    from curve_gaussian_amd.train_step import GraphedTrainStep, TrainStep
    torch.manual_seed(0); ga, cams, gts = _train_fixture()
    torch.manual_seed(0); gb, _, _ = _train_fixture()
    ea = TrainStep(ga, cams, gts, seed=6, densify_until_iter=5)
    gs = GraphedTrainStep(gb, cams, gts, seed=6, densify_until_iter=5)
    for _ in range(10):
        la = ea.step()[0]
        lb = gs.step()[0]
    gs.finish()
    assert gs.recaptures == 2 and gs._use_mask
    np.testing.assert_allclose(float(lb), float(la), rtol=1e-4)
    for n in ("_curve_points", "_width", "_opacity", "_mask"):
        np.testing.assert_allclose(getattr(gb, n).detach().cpu().numpy(), getattr(ga, n).detach().cpu().numpy(),
                                   rtol=1e-3, atol=1e-5, err_msg=n)
    assert float((gb._mask.detach() - 1.0).abs().max()) > 0   # the mask logits did move in the mask phase


def test_graphed_train_step_view_parallel_mode_single_rank_group():
    """The view-parallel code path of GraphedTrainStep (graph without optimizer -> RCCL all-reduce of the flat gradients
    and of the overflow flag -> Adam kernel; overflow handled with a fixed two-iteration lag so that all ranks agree)
    exercised on a single-rank RCCL group: same trajectory as the eager step, with and without forced overflow."""
    import torch.distributed as dist
    from curve_gaussian_amd.train_step import GraphedTrainStep, TrainStep
    created = False
    if not dist.is_initialized():
        dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29541", rank=0, world_size=1,
                                device_id=torch.device("cuda", 0))
        created = True
    try:
        torch.manual_seed(0); ga, cams, gts = _train_fixture()
        torch.manual_seed(0); gb, _, _ = _train_fixture()
        torch.manual_seed(0); gc, _, _ = _train_fixture()
        ea = TrainStep(ga, cams, gts, seed=9)
        gs = GraphedTrainStep(gb, cams, gts, seed=9, collectives=True)
        torch.manual_seed(0); gd, _, _ = _train_fixture()
        gcap = GraphedTrainStep(gd, cams, gts, seed=9, collectives=True, capture_collectives=True)   # RCCL inside the graph
        tiny = GraphedTrainStep(gc, cams, gts, seed=9, collectives=True)
        tiny._cap = 64
        tiny._probe_capacity = lambda: 64
        torch.manual_seed(0); ge, _, _ = _train_fixture()
        tcap = GraphedTrainStep(ge, cams, gts, seed=9, collectives=True, capture_collectives=True)   # ... across overflows
        tcap._cap = 64
        tcap._probe_capacity = lambda: 64
        for _ in range(10):
            ea.step(); gs.step(); tiny.step(); gcap.step(); tcap.step()
        gs.finish(); tiny.finish(); gcap.finish(); tcap.finish()
        assert gs.recaptures == 1 and tiny.recaptures > 1 and gc.optimizer.step_count == 10
        assert tcap.recaptures > 1 and ge.optimizer.step_count == 10
        np.testing.assert_allclose(ge._curve_points.detach().cpu().numpy(), ga._curve_points.detach().cpu().numpy(), rtol=2e-4,
                                   atol=2e-6, err_msg="captured collectives across a bucket overflow")
        for n in ("_curve_points", "_width", "_opacity"):
            ref = getattr(ga, n).detach().cpu().numpy()
            np.testing.assert_allclose(getattr(gb, n).detach().cpu().numpy(), ref, rtol=2e-4, atol=2e-6, err_msg=n)
            np.testing.assert_allclose(getattr(gc, n).detach().cpu().numpy(), ref, rtol=2e-4, atol=2e-6, err_msg="overflow " + n)
            np.testing.assert_allclose(getattr(gd, n).detach().cpu().numpy(), ref, rtol=2e-4, atol=2e-6, err_msg="captured collectives " + n)
    finally:
        if created:
            dist.destroy_process_group()


@pytest.mark.parametrize("launcher", ["torchrun", "self"])
def test_bench_two_rank_control_flow_rehearsal(launcher):
    """bench.py launched the way the driver launches it for N > 1 (torch.distributed.run, one process per rank) and the way
    a plain `python bench.py --gpus 2` launches ITSELF, as a rehearsal on ONE GPU: both ranks on device 0, collectives through
    gloo (CGS_BENCH_REHEARSAL).  Guards the control flow of the multi-rank path -- every rank reaches every collective, rank
    0 finishes its rank-0-only sections without one, exactly one JSON line comes out -- not its performance."""
    import json
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, CGS_BENCH_REHEARSAL="1")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    tail = [os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "8", "--warmup", "2", "--config", "cfg1",
            "--no-cpu-baseline", "--train-step-multi"]
    if launcher == "torchrun":
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
               "127.0.0.1", "--master-port", str(port)] + tail
    else:
        cmd = [sys.executable] + tail
    r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 8 and out["value"] > 0
    assert "roofline" in out and out["config"]["parallelism"] == "view-parallel x2"
    assert out["train_step_view_parallel_ms"] > 0
    # what the first hardware scaling record will be judged against: the collective's span, the step-boundary schedule and
    # the machine-readable prediction travel with every N > 1 line
    assert out["rccl_ranks"] == 2 and out["step_boundary"].startswith("double-buffered")
    es = out["expected_scaling"]
    assert es["all_reduce_bytes"] == 38 * 4 * out["config"]["curves"] and es["overlapped_with_next_step"] is True
    assert es["min_efficiency_vs_1gpu"] == 0.97 and es["reference_predictions"]["cfg5"]["step_ms"] == 5.6
    # ... and the MEASURED counterparts that make a first hardware run self-diagnosing: the all-reduce timed
    # alone, every rank's time for the timed region, and each rank's own single-GPU rate from before the group formed
    assert out["all_reduce_ms"] > 0
    pr = out["per_rank_ms_per_step"]
    assert len(pr["all"]) == 2 and pr["min"] <= pr["max"] and pr["slowest_rank"] in (0, 1)
    assert abs(pr["max"] - out["ms_per_step"]) <= 1e-3 * out["ms_per_step"] + 1e-3
    assert out["own_n1"]["msplats_per_s_rank0"] > 0 and out["own_n1"]["msplats_per_s_min_over_ranks"] > 0
    assert 0 < out["efficiency_vs_own_n1"] < 1.5


def _bench_cmd(*flags):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT",
                                                             "CGS_BENCH_REHEARSAL", "CGS_BENCH_FORCE_DIST")}
    return [sys.executable, os.path.join(root, "bench.py")] + list(flags), root, env


def test_bench_refuses_more_ranks_than_gpus():
    """`python bench.py --gpus N` on a node with fewer than N GPUs must exit non-zero with a message -- not print a 1-rank line
    that a scaling table would mistake for an N-GPU measurement."""
    import subprocess
    n = torch.cuda.device_count()
    cmd, root, env = _bench_cmd("--gpus", str(n + 1), "--steps", "2", "--warmup", "1", "--config", "cfg1", "--no-cpu-baseline")
    r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert f"--gpus {n + 1}" in r.stderr and "visible" in r.stderr, r.stderr[-1000:]
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    # ... and a launcher / flag disagreement is an error too (WORLD_SIZE says 1 rank, --gpus says the whole node)
    if n >= 2:
        env2 = dict(env, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
        r = subprocess.run(cmd[:2] + ["--gpus", str(n)] + cmd[4:], cwd=root, env=env2, capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and "must agree" in r.stderr


def test_bench_two_rank_rccl_self_launch():
    """The real thing on a box with >= 2 GPUs: `python bench.py --gpus 2` starts two ranks itself, the step's all-reduce runs
    over RCCL, and the line says so."""
    import json
    import subprocess
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two visible GPUs (one rank per GPU; RCCL refuses two ranks on one device)")
    cmd, root, env = _bench_cmd("--gpus", "2", "--steps", "4", "--warmup", "1", "--min-seconds", "0.5", "--config", "cfg1",
                                "--no-cpu-baseline", "--train-step-multi")
    r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["rccl_ranks"] == 2 and out["value"] > 0
    assert out["train_step_view_parallel_ms"] > 0


def test_captured_collectives_need_an_explicit_opt_in_beyond_one_rank(monkeypatch):
    """GraphedTrainStep(capture_collectives=True) has never seen a second rank: with world > 1 it refuses unless
    CGS_ALLOW_CAPTURED_COLLECTIVES=1 (the check comes before any process-group use)."""
    from curve_gaussian_amd.train_step import GraphedTrainStep
    gm, cams, gts = _train_fixture()
    monkeypatch.delenv("CGS_ALLOW_CAPTURED_COLLECTIVES", raising=False)
    with pytest.raises(ValueError, match="CGS_ALLOW_CAPTURED_COLLECTIVES"):
        GraphedTrainStep(gm, cams, gts, rank=0, world=2, capture_collectives=True, collectives=True)


def test_bench_default_schedule_over_single_rank_rccl():
    """bench.py with CGS_BENCH_FORCE_DIST=1: the default schedule (graph replay per view, three views in flight, double-buffered
    gradient sets, one all-reduce per step) and --train-step-multi with the collectives going through a real RCCL communicator
    of ONE rank -- what the driver's N > 1 runs execute per rank, minus the peers.  `rccl_ranks` says what the group spanned."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, CGS_BENCH_FORCE_DIST="1", MASTER_PORT="29547")
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--steps", "4", "--warmup", "1", "--min-seconds", "0.2", "--config", "cfg1",
           "--no-cpu-baseline", "--no-train-step", "--train-step-multi"]
    r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["rccl_ranks"] == 1 and out["n_gpus"] == 1 and out["value"] > 0
    assert out["step_boundary"].startswith("double-buffered") and "expected_scaling" not in out
    assert out["train_step_view_parallel_ms"] > 0
    assert out["step_gradient_rel_l2_vs_serial_eager"] < 1e-3
    # the measured diagnostics of a multi-rank line, here over a one-rank RCCL communicator
    assert out["all_reduce_ms"] > 0 and len(out["per_rank_ms_per_step"]["all"]) == 1
    assert out["own_n1"]["msplats_per_s_rank0"] > 0 and 0.3 < out["efficiency_vs_own_n1"] < 1.5


def test_bench_default_command_runs_every_section():
    """`python bench.py --gpus 1 --steps K --warmup W` -- the driver's command, nothing switched off -- end to end on the
    smallest config: the timed region, per-kernel times, shared sampling, the drop-in routes (shim and ctypes), the operator-API
    instances (`general_route`), every train-step variant and the CPU baseline all run and land in ONE JSON line with the
    contract's fields.  (Round 5: a shadowed name crashed the CPU-baseline section of exactly this command while every test
    that switches sections off stayed green.)"""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--min-seconds", "0.2",
           "--config", "cfg1", "--cpu-views", "1", "--torch-cpu-splats", "4"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and r.stdout.rstrip().endswith(lines[0]), r.stdout[-2000:]
    out = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in out, k
    assert out["n_gpus"] == 1 and out["rccl_ranks"] == 1 and out["steps"] == 3 and out["warmup"] == 1 and out["value"] > 0
    assert set(("bound", "achieved", "peak", "unit", "frac", "traffic")) <= set(out["roofline"])
    assert set(("value", "unit", "cores", "kind", "sample")) <= set(out["cpu_baseline"]) and out["cpu_baseline"]["value"] > 0
    assert "workload" in out["config"] and "model" not in out["config"]
    for k in ("dropin_view_ms", "dropin_view_general_route_ms", "dropin_view_ctypes_ms", "train_step_ms", "train_step_eager_ms"):
        assert out[k] > 0, k
    gr = out["general_route"]
    assert set(gr["instances"]) == {"reference_call", "training_general", "colour_grad", "colour_allmap", "all_grad"}
    assert gr["roofline"]["bound"] == "hbm" and 0 < gr["roofline"]["frac"] < 1


@pytest.mark.parametrize("flags,launch", [
    (["--mode", "raster"], None),
    (["--no-graph"], "eager launches (fused direct body"),
    (["--autograd-view"], "hipGraph replay per view (autograd body"),
    (["--no-graph", "--autograd-view"], "eager launches (autograd body"),
    (["--no-pingpong"], "hipGraph replay per view (fused direct body"),
    (["--streams", "1", "--views-per-step", "1"], "hipGraph replay per view (fused direct body"),
], ids=["raster", "eager_direct", "graph_autograd", "eager_autograd", "single_gradient_set", "reference_schedule"])
def test_bench_other_schedules(flags, launch):
    """Every schedule bench.py's ViewPipeline offers besides the default one, short, on the smallest config: each runs to its
    JSON line, says which launch form it used, and -- wherever views overlap or graphs replay -- reproduces the serial eager
    step gradient (bench.check_step_gradient raises otherwise)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--steps", "3", "--warmup", "1", "--min-seconds", "0.2", "--config", "cfg1",
           "--no-cpu-baseline", "--no-train-step"] + flags
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["value"] > 0 and out["config"]["mode"] == ("raster" if "raster" in flags else "view")
    if launch is not None:
        assert out["config"]["launch"].startswith(launch), out["config"]["launch"]
        assert out["kernel_ms_per_view"]["render_fwd"] > 0
    if "step_gradient_rel_l2_vs_serial_eager" in out:
        assert out["step_gradient_rel_l2_vs_serial_eager"] < 1e-3
    if "--no-pingpong" in flags:
        assert out["step_boundary"] == "join per step"


def test_bench_dump_outputs_reproduce_across_runs_and_schedules():
    """--dump-outputs DIR writes what the last timed step computed, float32, within 64 MB, and the line says what it wrote.
    Two runs with the same arguments see the same inputs, so their dumps agree (gradients up to the order of float atomics,
    radii exactly).  So does a run over a one-rank RCCL group on one stream: there the all-reduce diagnostic after the
    timed region reuses the very buffer the last step reduced into, and the dump must be taken before it.  Raster mode dumps
    the rasterizer's outputs and gradients.  --steps K is echoed and is the number of timed steps."""
    import json
    import subprocess
    import sys
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "CGS_BENCH_FORCE_DIST")}
    base = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "1", "--config", "cfg1",
            "--no-cpu-baseline", "--no-train-step", "--no-kernel-times", "--no-general-route"]
    runs = (([], {}), ([], {}), (["--streams", "1"], {"CGS_BENCH_FORCE_DIST": "1", "MASTER_PORT": "29553"}),
            (["--mode", "raster"], {}))
    with tempfile.TemporaryDirectory() as tmp:
        dumps = []
        for i, (extra, extra_env) in enumerate(runs):
            d = os.path.join(tmp, str(i))
            r = subprocess.run(base + extra + ["--dump-outputs", d], cwd=root, env=dict(env, **extra_env), capture_output=True,
                               text=True, timeout=600)
            assert r.returncode == 0, r.stderr[-2000:]
            out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
            assert out["steps"] == 5 and "repeats" not in out
            assert out["views_timed"] == 5 * out["config"]["views_per_step_per_rank"]
            man = out["dump_outputs"]["arrays"]
            assert sorted(f[:-4] for f in os.listdir(d)) == sorted(man)
            arrs = {n: np.load(os.path.join(d, n + ".npy")) for n in man}
            assert sum(os.path.getsize(os.path.join(d, n + ".npy")) for n in man) <= 64 * 2 ** 20
            for n, a in arrs.items():
                assert a.dtype == np.float32 and np.isfinite(a).all(), n
                assert "sampled" in man[n] or list(a.shape) == man[n]["shape"], n
            dumps.append(arrs)
        a, b, dist1, ras = dumps
        assert out["config"]["mode"] == "raster"
        B = 417
        assert a["grad_curve_points"].shape == (B, 4, 3) and a["grad_width"].shape == (B, 1)
        assert a["last_view_color"].shape == (1, 800, 800) and a["last_view_all_map"].shape == (4, 800, 800)
        assert np.abs(a["grad_curve_points"]).max() > 0 and (a["last_view_radii"] > 0).any()
        for other in (b, dist1):
            assert sorted(a) == sorted(other)
            np.testing.assert_array_equal(a["last_view_radii"], other["last_view_radii"])
            for n in a:
                rel = np.linalg.norm(a[n] - other[n]) / max(np.linalg.norm(a[n]), 1e-30)
                assert rel < 1e-4, (n, rel)
        assert {"color", "radii", "all_map", "dL_dmeans3D", "dL_dscales", "dL_drotations", "dL_dopacity"} <= set(ras)


def test_bench_times_k_steps_and_dumps_the_last_one(tmp_path, monkeypatch):
    """In process, on the default schedule (graph replay, three streams, double-buffered gradient sets): the timed region
    dispatches exactly the K steps of views my_cams[Wm G:(Wm + K) G], and the dump holds the LAST of them -- its summed
    gradient and its last view's outputs equal the same views run again one at a time, eagerly, through the drop-in API,
    while the step before it gives a clearly different gradient."""
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "CGS_BENCH_FORCE_DIST", "CGS_BENCH_REHEARSAL"):
        monkeypatch.delenv(k, raising=False)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    import bench
    K, Wm = 5, 2
    args = bench.parse_args(["--gpus", "1", "--steps", str(K), "--warmup", str(Wm), "--config", "cfg1",
                             "--dump-outputs", str(tmp_path / "d")])
    w = bench.Workload(args, bench.start_rank(args))
    pipe = bench.ViewPipeline(w)
    G = pipe.G
    assert pipe.use_graphs and pipe.vstreams.n == 3 and pipe.n_sets == 2 and G == 8
    calls = []
    run_views = pipe.run_views

    def spy(view_list, *a, **kw):
        s0 = pipe.step_no
        run_views(view_list, *a, **kw)
        calls.append((list(view_list), pipe.step_no - s0))
    monkeypatch.setattr(pipe, "run_views", spy)
    head = bench.time_headline(pipe)
    assert pipe.use_graphs and int(pipe.overflow_acc.item()) == 0     # no eager re-timing
    assert [n for _, n in calls] == [Wm, K]
    assert [id(c) for c in calls[1][0]] == [id(c) for c in w.my_cams[Wm * G:(Wm + K) * G]]
    dumped = head["dumped"]["arrays"]
    got = {n: np.load(tmp_path / "d" / (n + ".npy")) for n in dumped}
    assert not any("sampled" in e for e in dumped.values())

    def serial_step(cams):
        pipe.run_views(cams, serial=True, graphs=False)
        pipe.barrier()
        flat = pipe.last_step_gradient(serial=True)
        B = w.B
        return np.concatenate([flat[:12 * B].cpu().numpy(), flat[12 * B:14 * B].cpu().numpy()])

    rel = lambda x, y: float(np.linalg.norm(x - y) / max(np.linalg.norm(y), 1e-30))
    dumped_grad = np.concatenate([got[n].reshape(-1) for n in ("grad_curve_points", "grad_width", "grad_opacity")])
    last = serial_step(w.my_cams[(Wm + K - 1) * G:(Wm + K) * G])
    outs = {k: v.detach().float().cpu().numpy() for k, v in pipe.last_outputs.items()}
    assert rel(dumped_grad, last) < 1e-3        # the bench's own tolerance for schedule vs serial eager
    # (the drop-in path samples and projects in other kernels than the fused one: a last-ulp ceil may flip a radius by 1)
    dr = np.abs(got["last_view_radii"] - outs["radii"])
    assert dr.max() <= 1 and np.mean(dr > 0) < 1e-3
    for n in ("color", "invdepth", "all_map"):
        assert rel(got["last_view_" + n], outs[n]) < 1e-4, n
    before = serial_step(w.my_cams[(Wm + K - 2) * G:(Wm + K - 1) * G])
    assert rel(dumped_grad, before) > 1e-2
    del pipe, w
    torch.cuda.synchronize()


def test_connection_loss_matches_the_reference_block():
    """cgs_endpoint_connection_loss (O(B) memory, one sweep) against train.py:133-146 written out with torch.cdist:
    value, gradient w.r.t. the control points (only first and last points receive one), the no-pair case, and end points
    that coincide exactly (zero distance: counted, zero gradient)."""
    from curve_gaussian_amd.ops import regularizers as RG

    class G:
        pass
    g = torch.Generator().manual_seed(12)
    for B, spread in ((700, 0.25), (257, 0.12), (40, 5.0)):
        cp = (torch.rand(B, 4, 3, generator=g) * spread).to(DEV)
        if B == 257:
            cp[5, 0] = cp[9, 3]                     # coincident end points of different curves
            cp[7, 3] = cp[7, 0]                     # a closed curve: same-curve pairs are excluded
        a, b = G(), G()
        a._curve_points = cp.clone().requires_grad_(True)
        a.get_curve_points = a._curve_points
        b._curve_points = cp.clone().requires_grad_(True)
        ref = RG.connection_loss_reference(a, 0.1)
        ref.backward()
        val = RG.connection_loss(b, 0.1)
        (3.0 * val).backward()
        if B == 40:
            assert float(ref) == 0.0 and float(val) == 0.0 and not bool(b._curve_points.grad.any())
            continue
        assert float(ref) > 0
        np.testing.assert_allclose(float(val), float(ref), rtol=2e-5)
        np.testing.assert_allclose(b._curve_points.grad.cpu().numpy(), 3.0 * a._curve_points.grad.cpu().numpy(),
                                   rtol=2e-4, atol=1e-8)
        assert not bool(b._curve_points.grad[:, 1:3].any())


def test_graphed_train_step_crosses_the_connection_phase():
    """After conn_from_iter the end-point connection loss joins the regularisers (train.py:133); the graphed step
    re-captures at the switch and keeps following the eager trajectory (which uses the same fused op)."""
    from curve_gaussian_amd.train_step import GraphedTrainStep, TrainStep
    torch.manual_seed(0); ga, cams, gts = _train_fixture()
    torch.manual_seed(0); gb, _, _ = _train_fixture()
    kw = dict(seed=8, regularisers=True, conn_from_iter=4, lambda_points_conn=0.1)
    ea = TrainStep(ga, cams, gts, **kw)
    gs = GraphedTrainStep(gb, cams, gts, **kw)
    for _ in range(9):
        la = ea.step()[0]
        lb = gs.step()[0]
    gs.finish()
    assert gs.recaptures == 2 and gs._use_conn
    np.testing.assert_allclose(float(lb), float(la), rtol=1e-4)
    for n in ("_curve_points", "_width", "_opacity"):
        np.testing.assert_allclose(getattr(gb, n).detach().cpu().numpy(), getattr(ga, n).detach().cpu().numpy(),
                                   rtol=1e-3, atol=1e-5, err_msg=n)


@pytest.mark.parametrize("phase", ["plain", "regularisers", "late"])
def test_direct_eager_train_step_follows_the_autograd_one(phase):
    """TrainStep(direct=True): the eager iteration as plain library calls (no autograd, gradients added into the flat buffer
    by the kernels) -- same trajectory as the autograd form through the gate opening, the mask phase and the connection
    phase of train.py; the result dict still feeds the densification statistics."""
    from curve_gaussian_amd.train_step import TrainStep
    torch.manual_seed(0); ga, cams, gts = _train_fixture()
    torch.manual_seed(0); gb, _, _ = _train_fixture()
    kw = dict(seed=8)
    if phase != "plain":
        kw.update(regularisers=True)
    if phase == "late":
        kw.update(densify_until_iter=4, conn_from_iter=5, lambda_points_conn=0.1)
    ea = TrainStep(ga, cams, gts, **kw)
    eb = TrainStep(gb, cams, gts, direct=True, **kw)
    ea.reset_timestep = eb.reset_timestep = -3
    for _ in range(9):
        la, pa = ea.step()
        lb, pb = eb.step()
    np.testing.assert_allclose(float(lb), float(la), rtol=1e-4)
    for n in ("_curve_points", "_width", "_opacity", "_mask"):
        np.testing.assert_allclose(getattr(gb, n).detach().cpu().numpy(), getattr(ga, n).detach().cpu().numpy(),
                                   rtol=1e-3, atol=1e-5, err_msg=n)
    np.testing.assert_array_equal(pb["radii"].cpu().numpy(), pa["radii"].cpu().numpy())
    ga_m2d, gb_m2d = pa["viewspace_points"].grad.cpu().numpy(), pb["viewspace_points"].grad.cpu().numpy()
    np.testing.assert_allclose(gb_m2d, ga_m2d, rtol=2e-2, atol=2e-4 * np.abs(ga_m2d).max())
    vis = pb["radii"] > 0
    gb.add_densification_stats(pb["viewspace_points"], vis)          # what train.py:209 does with the dict
    assert float(gb.xyz_gradient_accum.sum()) > 0


@pytest.mark.parametrize("direct", [False, True])
def test_training_iteration_samples_the_curves_once(direct):
    """the eager training iteration ends with prepare_scaling_rot (train.py:242-243) and the next render samples
    the curves again inside the fused view forward -- two grid-wide norm passes (k_sample_f12) per iteration.  TrainStep makes
    the model's derived tensors lazy: ONE k_sample_f12 and no k_sample_f3 per iteration, and the derived tensors, once read,
    are the ones an eager prepare_scaling_rot gives."""
    from curve_gaussian_amd import _lib as L
    from curve_gaussian_amd.ops.curve_sampling import sample_curves
    from curve_gaussian_amd.train_step import TrainStep
    lib = L.load()
    torch.manual_seed(0); g, cams, gts = _train_fixture()
    ts = TrainStep(g, cams, gts, seed=8, direct=direct)
    assert g.lazy_derived
    for _ in range(3):
        ts.step()
    torch.cuda.synchronize()
    lib.cgs_prof_reset(); lib.cgs_prof_enable(1)
    n = 5
    for _ in range(n):
        ts.step()
    torch.cuda.synchronize()
    lib.cgs_prof_enable(0)
    prof = L.prof_collect()
    lib.cgs_prof_reset()
    assert prof["sample_f12"][1] == n, prof
    assert "sample_f3" not in prof, prof
    xyz, rot, scl = sample_curves(g._curve_points, g._width, g.is_bezier, g.n_gaussians)
    assert torch.equal(g.get_xyz, xyz) and torch.equal(g._rotation, rot) and torch.equal(g.get_scaling, scl)
    assert g.get_xyz.requires_grad                      # derived under the grad mode of the prepare_scaling_rot() call
    # deferred tensors are derived from the parameters as they are when first read, and the stamp says so
    g.prepare_scaling_rot()
    with torch.no_grad():
        g._width.add_(0.01)
    _x, _r, scl2 = sample_curves(g._curve_points, g._width, g.is_bezier, g.n_gaussians)
    assert torch.equal(g.get_scaling, scl2) and g._derived_from == g._param_stamp()
    assert g.get_xyz.shape[0] == g.n_splats


def test_shared_sampling_over_a_view_batch_gives_the_summed_gradient():
    """cgs_view_forward_shared / CGS_VIEW_SHARED + cgs_view_shared_begin / _end: the grid-wide norm pass and the last pass of the sampling
    backward once per view BATCH (same parameters for every view of it) instead of once per view.  The batch gradient must be
    the sum of the per-view gradients of the default mode -- that backward pass is linear in the per-splat gradients."""
    import ctypes as C
    from curve_gaussian_amd import _lib as L
    lib = L.load()
    curves = S.make_curves(700, 21)
    curves["width"] = curves["width"] + 0.6
    cams = [S.make_camera((0.5 + 1.8 * math.cos(a), 0.5 + 1.8 * math.sin(a), 0.8), (0.5, 0.5, 0.5), (0, 0, 1), 144, 176).to(DEV)
            for a in (0.2, 1.9, 3.7)]
    vc = _ViewCalls(curves["curve_points"], curves["width"], curves["opacity"], curves["is_bezier"], cams[0], 1024)
    dimgs = [torch.randn(1, vc.H, vc.W, generator=torch.Generator().manual_seed(30 + k)).to(DEV) for k in range(3)]
    pt, st = L.ptr, L.raw_stream(torch.device(DEV))

    def batch(shared):
        g = [vc.f32(vc.B, 4, 3), vc.f32(vc.B, 1), vc.f32(vc.B, 1)]
        if shared:
            L.check(lib.cgs_view_shared_begin(vc.B, vc.m, pt(vc.cp), pt(vc.isb), pt(vc.coef), pt(vc.norms), pt(vc.scratch), st),
                    "cgs_view_shared_begin")
        for cam, d in zip(cams, dimgs):
            vc.cam = cam
            vc.forward(shared=shared)
            vc.backward(d, *g, 3 if shared else 1)    # CGS_VIEW_ACCUMULATE [| CGS_VIEW_SHARED]
        if shared:
            L.check(lib.cgs_view_shared_end(vc.B, vc.m, pt(vc.cp), pt(vc.w), pt(vc.isb), pt(vc.coef), C.c_float(1e-8),
                                            pt(vc.norms), pt(vc.scratch), pt(g[0]), pt(g[1]), 0, st), "cgs_view_shared_end")
        torch.cuda.synchronize()
        return [t.cpu().double() for t in g]

    ref, got = batch(False), batch(True)
    for name, a, b in zip(("curve_points", "width", "opacity"), got, ref):
        assert float(b.abs().max()) > 0
        rel = float((a - b).norm() / b.norm())
        assert rel < 2e-4, f"shared sampling, dL/d{name}: relative L2 {rel:.2e} against the per-view sum"
