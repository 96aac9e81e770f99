"""GPU: the depth gate of the training render (cgs_view_forward_depth / cgs_view_forward_render_depth, k_view_fwd<true>).

1. the gated radii are where(hidden, 0, ungated radii), hidden by the chain's own rule on the forward's own centres;
2. planes that hide nothing change nothing, to the bit, outputs and gradients of both entries;
3. image and gradients equal the ungated route with exactly the hidden splats masked off (use_mask);
4. both bindings of the fused node agree under the gate;
5. GraphedTrainStep follows TrainStep(direct=True) under the gate, across a bucket overflow and a gate_from_iter switch;
6. on a solid with its hidden lines removed the gate lowers the photometric loss of every view that hides something.

The scene of 1 - 4 is train_gate_cases.py's: 40 x 24 pixels, three views, P = 240 and 264."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import train_gate_cases as TG
from util import assert_close, tanfov

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CAP = 1024


class _Calls:
    """The two forwards and their gated siblings through ctypes on caller-owned buffers, with the matching backwards:
    "fwd" = cgs_view_forward[_depth] + cgs_view_backward (with the model's derived splat tensors as outputs), "render" =
    cgs_view_forward_render[_depth] (sync-free, clamp and direction map on) + cgs_view_backward_render."""

    def __init__(self, curves, cam, mask=None):
        from curve_gaussian_amd import _lib as L
        from curve_gaussian_amd.ops import curve_sampling
        self.L, self.lib = L, L.load()
        lib = self.lib
        self.cam = cam.to(DEV)
        self.B, self.m = curves["curve_points"].shape[0], 12
        self.P = self.B * self.m
        self.H, self.W = cam.image_height, cam.image_width
        tiles = ((self.W + 15) // 16) * ((self.H + 15) // 16)
        self.tf = tanfov(cam)
        self.u8 = lambda n: torch.zeros(int(n), dtype=torch.uint8, device=DEV)
        self.f32 = lambda *sh: torch.zeros(*sh, dtype=torch.float32, device=DEV)
        self.cp, self.w, self.op = (curves[k].detach().to(DEV).contiguous() for k in ("curve_points", "width", "opacity"))
        self.mask = None if mask is None else mask.detach().to(DEV).float().contiguous()
        self.isb = curve_sampling._bezier_mask(curves["is_bezier"].to(DEV), DEV)
        self.coef = curve_sampling.sample_coefficients(self.m, DEV)
        self.nbin = int(lib.cgs_binning_bytes(CAP * tiles))
        self.bg = torch.zeros(3, device=DEV)
        self.off = int(lib.cgs_image_status_offset(self.W, self.H))

    def run(self, entry, dimg, gate=None):
        """One forward and its backward on fresh buffers -> {name: tensor} of every output and every gradient."""
        L, lib, pt, cf, cam = self.L, self.lib, self.L.ptr, C.c_float, self.cam
        st = L.raw_stream(torch.device(DEV))
        P, H, W, B, m = self.P, self.H, self.W, self.B, self.m
        norms = torch.empty(384, dtype=torch.float64, device=DEV)
        geom, img, binb = self.u8(lib.cgs_geometry_bytes(P)), self.u8(lib.cgs_image_bytes(W, H)), self.u8(self.nbin)
        o = dict(color=self.f32(1, H, W), invd=self.f32(1, H, W), omap=self.f32(4, H, W),
                 radii=torch.full((P,), -7, dtype=torch.int32, device=DEV))
        head = (B, m, pt(self.cp), pt(self.w), pt(self.isb), pt(self.coef), cf(1e-8), pt(norms), pt(self.op), pt(self.mask), cf(0.5))
        mid = (pt(geom), pt(binb), self.nbin, pt(img), CAP, pt(self.bg), W, H, pt(cam.world_view_transform),
               pt(cam.full_proj_transform), pt(cam.camera_center), self.tf[0], self.tf[1], pt(o["color"]), pt(o["invd"]),
               pt(o["omap"]), pt(o["radii"]))
        tail = (st,) if gate is None else (C.byref(gate), st)
        if entry == "fwd":
            o.update(xyz=self.f32(P, 3), rot=self.f32(P, 4), scl=self.f32(P, 3))
            fn = lib.cgs_view_forward if gate is None else lib.cgs_view_forward_depth
            L.check(fn(*head, None, *mid, pt(o["xyz"]), pt(o["rot"]), pt(o["scl"]), *tail), "view forward")
        else:
            o.update(clamped=self.f32(1, H, W), rend_dir=self.f32(3, H, W))
            fn = lib.cgs_view_forward_render if gate is None else lib.cgs_view_forward_render_depth
            L.check(fn(0, *head, *mid, pt(o["clamped"]), pt(o["rend_dir"]), *tail), "view forward render")
        torch.cuda.synchronize()
        status = img[self.off:self.off + 4 * int(lib.cgs_status_words())].view(torch.int32)
        assert int(status[2]) == 0, "bucket overflow: raise CAP"
        g = dict(g_cp=self.f32(B, 4, 3), g_w=self.f32(B, 1), g_op=self.f32(B, 1), g_m2d=self.f32(P, 3))
        if self.mask is not None:
            g["g_mask"] = self.f32(*self.mask.shape)
        scratch = self.f32(int(lib.cgs_view_backward_scratch_floats(B, m)))
        bhead = head + ((None,) if entry == "fwd" else ()) + (
            pt(geom), pt(binb), pt(img), pt(self.bg), W, H, pt(cam.world_view_transform), pt(cam.full_proj_transform),
            pt(cam.camera_center), self.tf[0], self.tf[1], pt(o["radii"]), pt(dimg))
        btail = (pt(g["g_m2d"]), pt(g["g_cp"]), pt(g["g_w"]), pt(g["g_op"]), pt(g.get("g_mask")), pt(scratch), 0, st)
        if entry == "fwd":
            L.check(lib.cgs_view_backward(*bhead, None, *btail), "view backward")
        else:
            L.check(lib.cgs_view_backward_render(*bhead, pt(o["color"]), *btail), "view backward render")
        torch.cuda.synchronize()
        o.update(g)
        return o


def _gate(cams, stack, slack=TG.SLACK):
    return TG.manual_gate(cams, stack, slack, device=torch.device(DEV))


def _host_cams(gate):
    return gate.intr.cpu().numpy(), gate.w2c.cpu().numpy()


def _same_bits(name, a, b):
    for k in a:
        x, y = a[k], b[k]
        assert x.dtype == y.dtype and x.shape == y.shape, (name, k)
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), \
            (name, k, float((x.float() - y.float()).abs().max()))


@pytest.fixture(scope="module")
def scene():
    """Per size B: curves, the three cameras, the ungated forwards (their xyz are the centres every rule is held against),
    the gate with the NaN and the +inf poked in, and hidden [3,P] by gate_view_host."""
    from curve_gaussian_amd.ops.edge_occlusion import gate_view_host
    cams = TG.cameras()
    dimg = torch.randn(1, TG.H, TG.W, generator=torch.Generator().manual_seed(3)).to(DEV)
    out = {}
    for B in TG.SIZES:
        curves = TG.curves(B)
        calls = [_Calls(curves, cam) for cam in cams]
        plain = [c.run("fwd", dimg) for c in calls]
        xyz = plain[0]["xyz"].cpu().numpy()
        for p in plain[1:]:
            assert torch.equal(p["xyz"], plain[0]["xyz"])        # the centres do not depend on the view
        gate = _gate(cams, TG.planes())
        K, M = _host_cams(gate)
        nan_cell, inf_cell = TG.poke(gate.planes, xyz, K, M)
        planes = gate.planes.cpu().numpy()
        views = [gate_view_host(xyz, K[v], M[v], planes[v], TG.SLACK) for v in range(3)]
        out[B] = dict(curves=curves, cams=cams, calls=calls, plain=plain, xyz=xyz, gate=gate, views=views, dimg=dimg,
                      nan_cell=nan_cell, inf_cell=inf_cell)
    return out


# ------------------------------------------------------------------------------------------------ 1. the radii, exactly
@pytest.mark.parametrize("B", TG.SIZES)
def test_gated_radii_are_the_ungated_radii_with_the_hidden_splats_zeroed(scene, B):
    from curve_gaussian_amd.ops.edge_occlusion import point_masks_depth
    s = scene[B]
    gate = s["gate"]
    xyz_dev = s["plain"][0]["xyz"]
    _m, kept, hidden_count = point_masks_depth(xyz_dev, gate.intr, gate.w2c, gate.planes, TG.SLACK, return_counts=True)
    view_idx = torch.zeros(1, dtype=torch.int32, device=DEV)
    seen_cases = dict(off_image=0, behind=0, nan=0, inf=0, hidden=0, all_hidden=False)
    for v in range(3):
        u, w, seen, hid = s["views"][v]
        # the GPU operator of the chain and the host statement of its rule agree on these centres
        assert int(hidden_count[v]) == int(hid.sum()) and int(kept[v]) == int(seen.sum()), v
        radii0 = s["plain"][v]["radii"].cpu().numpy()
        want = np.where(hid, 0, radii0)
        host = s["calls"][v].run("fwd", s["dimg"], gate.struct(v))
        view_idx.fill_(v)
        dev = s["calls"][v].run("fwd", s["dimg"], gate.struct(view_idx))
        rend = s["calls"][v].run("render", s["dimg"], gate.struct(v))
        assert np.array_equal(host["radii"].cpu().numpy(), want), (v, int((host["radii"].cpu().numpy() != want).sum()))
        assert np.array_equal(rend["radii"].cpu().numpy(), want), v
        _same_bits(f"view {v}: host view vs device view index", host, dev)
        # what the cases are there for
        M = gate.w2c.cpu().numpy()[v]
        c2 = s["xyz"].astype(np.float64) @ M[8:11] + M[11]
        kept_v = seen | hid
        seen_cases["off_image"] += int(((c2 > 0) & ~kept_v & (radii0 > 0) & (want > 0)).sum())   # drawn though the centre is off
        seen_cases["behind"] += int((c2 <= 0).sum())
        seen_cases["hidden"] += int((hid & (radii0 > 0)).sum())
        if v == 1:
            seen_cases["all_hidden"] = bool(hid.sum() > 0 and seen.sum() == 0 and (want[kept_v] == 0).all())
        if v == 0:
            cell = lambda rc: (np.floor(w) == rc[0]) & (np.floor(u) == rc[1]) & kept_v
            seen_cases["nan"] += int((cell(s["nan_cell"]) & ~hid & (want == radii0)).sum())
            seen_cases["inf"] += int((cell(s["inf_cell"]) & ~hid & (want == radii0)).sum())
    assert seen_cases["off_image"] > 0 and seen_cases["behind"] > 0 and seen_cases["hidden"] > 0, seen_cases
    assert seen_cases["nan"] > 0 and seen_cases["inf"] > 0 and seen_cases["all_hidden"], seen_cases
    # a device view index outside [0, V) reads nothing and hides nothing
    view_idx.fill_(7)
    stray = s["calls"][0].run("fwd", s["dimg"], gate.struct(view_idx))
    _same_bits("stray device view index", stray, s["plain"][0])


# ------------------------------------------------------------------------------------------------ 2. nothing hidden
@pytest.mark.parametrize("B", TG.SIZES)
def test_planes_that_hide_nothing_change_nothing(scene, B):
    s = scene[B]
    cams = s["cams"]
    inf_planes = np.full((3, TG.H, TG.W), np.inf, np.float32)
    far = np.full((3, TG.H, TG.W), 100.0, np.float32)
    gates = {"+inf planes": _gate(cams, inf_planes), "planes behind everything": _gate(cams, far),
             "slack = +inf": _gate(cams, TG.planes())}
    gates["slack = +inf"].slack = float("inf")       # (with the plane in front of everything in view 1)
    view_idx = torch.zeros(1, dtype=torch.int32, device=DEV)
    for v in range(3):      # view 1: centres off the image; view 2: centres behind the camera
        for entry in ("fwd", "render"):
            sibling = s["calls"][v].run(entry, s["dimg"])
            assert int((sibling["radii"] > 0).sum()) > 0 and float(sibling["g_cp"].abs().max()) > 0
            for name, gate in gates.items():
                view_idx.fill_(v)
                for view in (v, view_idx):
                    got = s["calls"][v].run(entry, s["dimg"], gate.struct(view))
                    _same_bits(f"{name}, view {v}, {entry}", got, sibling)


# ------------------------------------------------------------------------------------------------ 3. image and gradients
def _model(curves, mask=None):
    from curve_gaussian_amd.scene import GaussianCurveModel
    return GaussianCurveModel(0, 12, device=DEV).create_from_curves(curves["curve_points"], curves["width"], curves["opacity"],
                                                                    mask, curves["is_bezier"])


@pytest.mark.parametrize("B", TG.SIZES)
def test_gated_render_equals_the_ungated_render_of_the_visible_splats(scene, B):
    """The reference is the ungated fused route with a per-splat mask (use_mask) that switches off exactly the hidden splats
    (mask logit -20 under a threshold of 0.5: scale and opacity times 0); the criterion is the one test_render_route_gpu.py
    holds its two routes to -- assert_close with its default budgets for the maps, abs_floor=1e-6 for the screen-space
    gradient, relative L2 < 2e-5 for the parameter gradients."""
    from curve_gaussian_amd.gaussian_renderer import PipelineParams, render
    s = scene[B]
    gate, dimg = s["gate"], s["dimg"]
    bg = torch.zeros(3, device=DEV)
    for v in range(3):
        cam = s["cams"][v].to(DEV)
        hid = torch.from_numpy(s["views"][v][3])
        gm = _model(s["curves"])
        pg = render(cam, gm, PipelineParams(), bg, depth_gate=(gate, v))
        (pg["render"] * dimg).sum().backward()
        mask = torch.where(hid, -20.0, 20.0).reshape(B, 12, 1)
        gr = _model(s["curves"], mask)
        pr = render(cam, gr, PipelineParams(), bg, use_mask=True, mask_thr=0.5)
        (pr["render"] * dimg).sum().backward()
        hid_d = hid.to(DEV)
        assert torch.equal(pg["radii"] > 0, (pr["radii"] > 0) & ~hid_d) and bool((pg["radii"][hid_d] == 0).all())
        assert torch.equal(pg["visibility_filter"], (pg["radii"] > 0).nonzero())
        for k in ("render", "depth", "rend_dir", "rend_alpha"):
            assert_close(f"view {v} {k}", pg[k].detach().cpu().numpy(), pr[k].detach().cpu().numpy())
        g2, r2 = pg["viewspace_points"].grad, pr["viewspace_points"].grad
        assert float(g2[hid_d].abs().max() if hid.any() else 0.0) == 0.0        # rows of hidden splats: exactly 0
        assert_close(f"view {v} means2D grad", g2.cpu().numpy(), r2.cpu().numpy(), abs_floor=1e-6)
        for name in ("_curve_points", "_width", "_opacity"):
            a, b = getattr(gm, name).grad, getattr(gr, name).grad
            if float(b.norm()) == 0.0:      # (view 1: every in-image centre hidden, what is left may draw nothing)
                assert float(a.norm()) == 0.0, (v, name)
                continue
            rel = float((a - b).norm() / b.norm())
            assert rel < 2e-5, f"view {v} {name}: gated vs masked route relative L2 {rel:.2e}"
    # the general route has no gate
    with pytest.raises(ValueError, match="general route"):
        render(s["cams"][0].to(DEV), _model(s["curves"]), PipelineParams(), bg, fused=False, depth_gate=(gate, 0))


# ------------------------------------------------------------------------------------------------ 4. the two bindings
def test_both_bindings_of_the_fused_node_agree_under_the_gate(scene, monkeypatch):
    """Compared as test_render_route_gpu.py compares the two bindings: identical forward outputs, gradients equal to the
    rounding of the backward's atomics (rel = 2e-4)."""
    from curve_gaussian_amd import _lib as L
    from curve_gaussian_amd import diff_cur_rasterization as D
    from curve_gaussian_amd.gaussian_renderer import PipelineParams, render
    s = scene[TG.SIZES[1]]
    gate, dimg = s["gate"], s["dimg"]
    bg = torch.zeros(3, device=DEV)

    def use_binding(shim):
        if shim:
            monkeypatch.delenv("CGS_TORCH_SHIM", raising=False)
        else:
            monkeypatch.setenv("CGS_TORCH_SHIM", "0")
        monkeypatch.setattr(D._ExtProxy, "_impl", None)
    use_binding(True)
    if not L.use_shim():
        pytest.skip("CGS_LIB names an experiment build: the ctypes bindings are the only binding")
    mask = torch.randn(s["curves"]["curve_points"].shape[0], 12, 1, generator=torch.Generator().manual_seed(2)) * 3
    view_idx = torch.zeros(1, dtype=torch.int32, device=DEV)
    for v, use_mask, clamp, rend_dir, static, by_index in ((0, False, True, True, False, False), (0, True, False, False, True, True),
                                                           (2, True, True, True, True, False), (1, False, False, True, False, True)):
        case = f"view={v} mask={use_mask} clamp={clamp} rend_dir={rend_dir} static={static} by_index={by_index}"
        cam = s["cams"][v].to(DEV)
        view_idx.fill_(v)
        got = {}
        for shim in (True, False):
            use_binding(shim)
            gm = _model(s["curves"], mask)
            sink = []
            pkg = render(cam, gm, PipelineParams(), bg, use_mask=use_mask, mask_thr=0.3, clamp=clamp, compute_rend_dir=rend_dir,
                         static_bucket_cap=CAP if static else 0, status_sink=sink if static else None,
                         depth_gate=(gate, view_idx if by_index else v))
            node = pkg["render"].grad_fn.name()
            assert ("ViewRenderFn" in node) == shim and ("_ViewRender" in node) != shim, (case, node)
            if static:
                assert len(sink) == 1 and int(sink[0][2]) == 0, case
            (pkg["render"] * dimg).sum().backward()
            grads = {n: getattr(gm, n).grad for n in ("_curve_points", "_width", "_opacity", "_mask")}
            grads["viewspace_points"] = pkg["viewspace_points"].grad
            got[shim] = pkg, grads
        (ps, gs), (pc, gc) = got[True], got[False]
        hid = torch.from_numpy(s["views"][v][3]).to(DEV)
        assert bool((ps["radii"][hid] == 0).all()) and int(hid.sum()) > 0, case       # the gate did act
        for k in ("render", "depth", "rend_alpha", "rend_dir", "radii", "visibility_filter"):
            assert (ps[k] is None) == (pc[k] is None), (case, k)
            assert ps[k] is None or torch.equal(ps[k], pc[k]), (case, k)
        for n, a in gs.items():
            b = gc[n]
            assert (a is None) == (b is None), (case, n)
            if a is not None and float(b.abs().max()) > 0:
                assert_close(f"{case} {n}", b.cpu(), a.cpu(), rel=2e-4)


# ------------------------------------------------------------------------------------------------ 5. the training steps
def _train_fixture(n_curves=200, seed=11, H=64, W=96):
    from curve_gaussian_amd import synthetic as S
    from curve_gaussian_amd.gaussian_renderer import PipelineParams, render
    from curve_gaussian_amd.scene import GaussianCurveModel

    def model():
        c = S.make_curves(n_curves, seed)
        c["width"] = c["width"] + 0.8
        return GaussianCurveModel(0, 12, device=DEV).create_from_curves(c["curve_points"], c["width"], c["opacity"], None,
                                                                        c["is_bezier"])
    gm = model()
    cams = [S.make_camera((0.5 + 1.8 * math.cos(a), 0.5 + 1.8 * math.sin(a), 0.9), (0.5, 0.5, 0.5), (0, 0, 1), H, W).to(DEV)
            for a in (0.3, 1.7, 3.1, 4.4)]
    with torch.no_grad():
        tgt = model()
        tgt._curve_points.add_(0.01 * torch.randn_like(tgt._curve_points))
        tgt.prepare_scaling_rot()
        gts = [render(cm, tgt, PipelineParams(), torch.zeros(3, device=DEV))["render"].detach() for cm in cams]
    return gm, cams, gts


def test_graphed_step_follows_the_direct_step_under_the_gate():
    """The criterion of test_graphed_train_step_equals_eager_and_recovers_from_bucket_overflow: parameters within rtol 2e-4 /
    atol 2e-6 after 12 steps, the last loss within 1e-4.  The gate (a plane through the far third of the cloud, which hides
    about a third of the splats) starts at iteration 5: the graph re-captures there.  The third model starts its gated phase
    with buckets of 64 entries, far too small: that replay overflows, is skipped on the device and redone eagerly -- through
    the gate, which the spy on the gate's host-view calls sees."""
    from curve_gaussian_amd.train_step import GraphedTrainStep, TrainStep
    n, start = 12, 5
    models, gates = [], []
    for _ in range(3):
        torch.manual_seed(0)
        gm, cams, gts = _train_fixture()
        models.append(gm)
        H, W = cams[0].image_height, cams[0].image_width
        gates.append(TG.manual_gate(cams, np.full((4, H, W), 2.1, np.float32), slack=0.0, device=torch.device(DEV)))
    # the gate hides a real share of what is drawn, in every view
    from curve_gaussian_amd.ops.train_gate import splat_visibility
    seen, hidden, _dead = splat_visibility(models[0].get_xyz.detach(), gates[0])
    assert 0.15 < hidden.sum() / seen.sum() < 0.6, (hidden.sum(), seen.sum())
    kw = dict(seed=3, gate_from_iter=start)
    direct = TrainStep(models[0], cams, gts, direct=True, depth_gate=gates[0], **kw)
    la = [float(direct.step()[0]) for _ in range(n)]
    ungated = TrainStep(_train_fixture()[0], cams, gts, direct=True, seed=3)
    lu = [float(ungated.step()[0]) for _ in range(n)]
    # the gate starts AT iteration `start`: the same losses before it (to the rounding of the backward's atomics), another there
    np.testing.assert_allclose(la[:start - 1], lu[:start - 1], rtol=1e-4)
    assert abs(la[start - 1] - lu[start - 1]) > 1e-3 * abs(lu[start - 1]), (la[start - 1], lu[start - 1])
    graphed = GraphedTrainStep(models[1], cams, gts, depth_gate=gates[1], **kw)
    lb = [graphed.step()[0] for _ in range(n)][-1:]
    graphed.finish()
    assert graphed.recaptures == 2 and not graphed._inflight and graphed._use_gate     # the switch re-captured, once
    tol = dict(rtol=2e-4, atol=2e-6)
    np.testing.assert_allclose(float(lb[-1]), la[-1], rtol=1e-4)
    for name in ("_curve_points", "_width", "_opacity"):
        np.testing.assert_allclose(getattr(models[1], name).detach().cpu().numpy(),
                                   getattr(models[0], name).detach().cpu().numpy(), **tol)
    # the forced overflow inside the gated phase
    tiny = GraphedTrainStep(models[2], cams, gts, depth_gate=gates[2], **kw)
    host_views = []
    orig = gates[2].tensors
    gates[2].tensors = lambda view: (host_views.append(view) if not torch.is_tensor(view) else None, orig(view))[1]
    for it in range(1, n + 1):
        if it == start + 1:          # re-capture with buckets that cannot hold this scene
            tiny.finish()
            tiny._cap, tiny._graph, tiny._bufs = 64, None, None
            before = tiny.recaptures
        tiny.step()
        if it == start + 1:          # ONE overflow: seen and redone before the next step runs (replays that were queued behind
            tiny.finish()            # an overflowed one are redone after it, in another order than the eager loop's)
    tiny.finish()
    assert tiny.recaptures > before + 1 and models[2].optimizer.step_count == n        # overflowed, redone, re-captured
    assert len(host_views) >= 1 and all(isinstance(v, int) for v in host_views)        # the eager redo went through the gate
    for name in ("_curve_points", "_width", "_opacity"):
        np.testing.assert_allclose(getattr(models[2], name).detach().cpu().numpy(),
                                   getattr(models[0], name).detach().cpu().numpy(), **tol)
    with pytest.raises(ValueError, match="fused_view=True"):
        GraphedTrainStep(_train_fixture()[0], cams, gts, depth_gate=gates[0], fused_view=False)


# ------------------------------------------------------------------------------------------------ 6. what it is for
def test_the_gate_lowers_the_loss_of_every_view_that_hides_something():
    """solid_scan box, hidden lines removed, a model whose curves are the solid's ground-truth edges: in every view that
    hides at least one splat the photometric loss is strictly lower gated than ungated, in every other view the two are
    equal to the bit; at least a third of the views hide something (checked on the CPU, from the forward's own centres)."""
    from curve_gaussian_amd.gaussian_renderer import PipelineParams, render
    from curve_gaussian_amd.ops.edge_occlusion import gate_view_host
    from curve_gaussian_amd.ops.losses import photometric_loss
    from curve_gaussian_amd.ops.train_gate import TrainGate
    scan = TG.box_scan(backend="gpu", device=torch.device(DEV))
    gate = TrainGate(scan.cameras, occluder=scan.tris, device=torch.device(DEV))
    curves = TG.line_curves(scan.edges)
    gm = _model(curves)
    bg = torch.zeros(3, device=DEV)
    dimg = torch.zeros(1, 60, 80, device=DEV)
    xyz = _Calls(curves, scan.synth_cameras[0]).run("fwd", dimg)["xyz"].cpu().numpy()
    K, M = _host_cams(gate)
    planes = gate.planes.cpu().numpy()
    hides = [int(gate_view_host(xyz, K[v], M[v], planes[v], gate.slack)[3].sum()) for v in range(gate.V)]
    assert sum(h > 0 for h in hides) * 3 >= gate.V, hides
    for v, cam in enumerate(scan.synth_cameras):
        cam = cam.to(DEV)
        gt = torch.from_numpy(scan.maps[v]).float().div(255.0).reshape(1, 60, 80).to(DEV)
        with torch.no_grad():
            plain = render(cam, gm, PipelineParams(), bg, clamp=False)
            gated = render(cam, gm, PipelineParams(), bg, clamp=False, depth_gate=(gate, v))
            l_plain = photometric_loss(plain["render"], gt, 10.0, 0.1, clamp=True)
            l_gated = photometric_loss(gated["render"], gt, 10.0, 0.1, clamp=True)
        print(f"view {v}: hides {hides[v]} splats, loss ungated {float(l_plain):.6f} gated {float(l_gated):.6f}")
        assert int(((plain["radii"] > 0) & (gated["radii"] == 0)).sum()) <= hides[v]
        if hides[v] > 0:
            assert float(l_gated) < float(l_plain), (v, hides[v], float(l_gated), float(l_plain))
        else:
            assert torch.equal(l_gated, l_plain) and torch.equal(gated["render"], plain["render"]), v
