"""GPU: the held-out metric kernel (csrc/metrics.hip) and the evaluation API (curve_gaussian_amd.evaluation) against the
float64 restatement (tests/metrics_ref64.py) and the reference's own training_report (tests/golden/eval_metrics.npz);
then a synthetic Replica-like COLMAP scan read through Scene(eval=True), trained and reported -- the reports leave the
training trajectory of TrainStep and GraphedTrainStep unchanged."""
import ctypes
import os

import numpy as np
import pytest
import torch

import metrics_ref64 as M
from curve_gaussian_amd import _lib as L
from curve_gaussian_amd import evaluation as E
from curve_gaussian_amd import synthetic as S

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLDEN = np.load(os.path.join(os.path.dirname(__file__), "golden", "eval_metrics.npz"))


def _views(seed, shapes, lo=-0.3, hi=1.4):
    g = torch.Generator().manual_seed(seed)
    ims = [lo + (hi - lo) * torch.rand(1, H, W, generator=g) for H, W, _ in shapes]
    gts = [lo + (hi - lo) * torch.rand(C, H, W, generator=g) for H, W, C in shapes]
    return ims, gts


SHAPES = [(37, 53, 3), (8, 9, 1), (240, 321, 1), (129, 64, 3), (1, 1, 1), (300, 200, 3)]


@pytest.mark.parametrize("half", [False, True])
def test_kernel_matches_the_float64_restatement(half):
    ims, gts = _views(0, SHAPES)
    l1, mse = E.view_metrics([i.to(DEV) for i in ims], [g.to(DEV) for g in gts], half_width=half)
    assert l1.dtype == torch.float64 and l1.device.type == "cuda" and l1.shape == (len(SHAPES),)
    rl1, rmse = M.view_metrics([i.numpy() for i in ims], [g.numpy() for g in gts], half)
    np.testing.assert_allclose(l1.cpu().numpy(), rl1, rtol=1e-12)
    np.testing.assert_allclose(mse.cpu().numpy(), rmse, rtol=1e-12)


def test_kernel_is_bit_identical_across_runs_and_batches():
    ims, gts = _views(1, SHAPES)
    ims, gts = [i.to(DEV) for i in ims], [g.to(DEV) for g in gts]
    a = torch.stack(E.view_metrics(ims, gts), 1).cpu()
    b = torch.stack(E.view_metrics(ims, gts), 1).cpu()
    assert torch.equal(a, b)
    for k in range(len(SHAPES)):
        alone = torch.stack(E.view_metrics([ims[k]], [gts[k]]), 1).cpu()
        assert torch.equal(alone[0], a[k]), k
    rev = torch.stack(E.view_metrics(ims[::-1], gts[::-1]), 1).cpu()
    assert torch.equal(rev.flip(0), a)


def test_argument_errors_are_raised():
    im, gt = torch.rand(1, 8, 8, device=DEV), torch.rand(3, 8, 8, device=DEV)
    with pytest.raises(L.CurveGSError, match="GPU tensor"):
        E.view_metrics([im.cpu()], [gt.cpu()])
    with pytest.raises(ValueError, match="height or width"):
        E.view_metrics([im], [torch.rand(1, 8, 9, device=DEV)])
    with pytest.raises(ValueError, match="one channel"):
        E.view_metrics([gt], [gt])
    lib = L.load()
    ws = torch.empty(int(lib.cgs_view_metrics_workspace_bytes(1)), dtype=torch.uint8, device=DEV)
    out = torch.empty(1, 2, dtype=torch.float64, device=DEV)
    stream = L.raw_stream(DEV)

    def call(**kw):
        d = dict(image=im.data_ptr(), gt=gt.data_ptr(), channels=3, height=8, width=8, x0=0)
        d.update(kw)
        t = (L.MetricView * 1)(L.MetricView(**d))
        return lib.cgs_view_metrics(1, ctypes.cast(t, ctypes.c_void_p), L.ptr(ws), L.ptr(out), None, stream)

    assert call() == 0
    for bad in (dict(image=None), dict(gt=None), dict(channels=0), dict(height=0), dict(width=-1), dict(x0=8),
                dict(x0=-1)):
        assert call(**bad) == -1, bad
        assert b"invalid argument" in lib.cgs_last_error()
    assert lib.cgs_view_metrics(1, None, L.ptr(ws), L.ptr(out), None, stream) == -1
    assert lib.cgs_view_metrics(0, None, None, None, None, stream) == 0
    torch.cuda.synchronize()


class _Scene:
    def __init__(self, train, test, gaussians=None):
        self.train, self.test, self.gaussians = train, test, gaussians

    def getTrainCameras(self):
        return self.train

    def getTestCameras(self):
        return self.test


class _View:
    def __init__(self, idx, gt):
        self.idx, self.original_image, self.image_name = idx, gt, f"v{idx}"


@pytest.mark.parametrize("case", [str(c) for c in GOLDEN["cases"]])
def test_training_report_matches_the_reference_fixture(case, capsys):
    nt, ntr = int(GOLDEN[f"{case}_n_test"]), int(GOLDEN[f"{case}_n_train"])
    views = [_View(i, torch.from_numpy(GOLDEN[f"{case}_gt_{i}"]).to(DEV)) for i in range(nt + ntr)]
    renders = {i: torch.from_numpy(GOLDEN[f"{case}_render_{i}"]).to(DEV) for i in range(nt + ntr)}
    order = []

    def render_func(viewpoint, gaussians, *args):
        order.append(viewpoint.idx)
        return {"render": renders[viewpoint.idx]}

    half = bool(GOLDEN[f"{case}_train_test_exp"])
    out = E.training_report(None, 3000, None, None, None, 0.0, [3000], _Scene(views[nt:], views[:nt]), render_func, (),
                            half)
    assert order == GOLDEN[f"{case}_order"].tolist()
    assert list(out) == GOLDEN[f"{case}_configs"].tolist()
    printed = capsys.readouterr().out
    for k, name in enumerate(out):
        assert f"[ITER 3000] Evaluating {name}: L1 " in printed
        np.testing.assert_allclose(out[name]["l1"], GOLDEN[f"{case}_l1"][k], rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(out[name]["psnr"], GOLDEN[f"{case}_psnr"][k], rtol=1e-5)
        idx = [v.idx for v in ([views[i] for i in order[:nt]] if name == "test" else [views[i] for i in order[-5:]])]
        l1, ps = M.report([GOLDEN[f"{case}_render_{i}"] for i in idx], [GOLDEN[f"{case}_gt_{i}"] for i in idx], half)
        np.testing.assert_allclose(out[name]["l1"], l1, rtol=1e-12)
        np.testing.assert_allclose(out[name]["psnr"], ps, rtol=1e-12)
    assert E.training_report(None, 3001, None, None, None, 0.0, [3000], _Scene(views, views), render_func, (), half) == {}


def _model(B=600, seed=4):
    from curve_gaussian_amd.scene import GaussianCurveModel
    c = S.make_curves(B, seed, room_scale=True)
    return GaussianCurveModel(0, 12, device=DEV).create_from_curves(c["curve_points"], c["width"], c["opacity"], c["mask"],
                                                                    c["is_bezier"]), c


def test_evaluate_views_equals_the_torch_expression_on_the_same_renders():
    from curve_gaussian_amd.gaussian_renderer import PipelineParams, render
    gm, _ = _model()
    cams = [c.to(DEV) for c in S.room_cameras(4, 68, 120, 4)]
    g = torch.Generator().manual_seed(3)
    bg = torch.zeros(3, device=DEV)
    for c, i in zip(cams, range(4)):
        c.original_image = (torch.rand(3 if i % 2 else 1, 68, 120, generator=g) * 1.2 - 0.1).to(DEV)
    res = E.evaluate_views(cams, gm, PipelineParams(), bg)
    l1s, ps = [], []
    with torch.no_grad():
        for c in cams:
            img = torch.clamp(render(c, gm, PipelineParams(), bg)["render"], 0.0, 1.0)
            gt = torch.clamp(c.original_image, 0.0, 1.0)
            d = (img - gt).double()
            l1s.append(float(d.abs().mean()))
            ps.append(float(20 * torch.log10(1.0 / torch.sqrt((d * d).mean()))))
    assert res["views"] == 4
    with torch.no_grad():
        assert float(torch.stack([render(c, gm, PipelineParams(), bg)["render"] for c in cams]).max()) > 0
    np.testing.assert_allclose(res["l1"], np.mean(l1s), rtol=1e-12)
    np.testing.assert_allclose(res["psnr"], np.mean(ps), rtol=1e-12)


def _replica_scan(tmp_path):
    """cfg4 geometry at a small size: curves in the room box, cameras inside it (synthetic.room_cameras), edge maps
    rendered from the true curves, written as a COLMAP scan with the curve midpoints as points3D."""
    from curve_gaussian_amd.gaussian_renderer import PipelineParams, render
    from curve_gaussian_amd.scene import colmap_io as CI
    tgt, curves = _model(B=800, seed=4)
    cams = S.room_cameras(12, 68, 120, 4)
    with torch.no_grad():
        maps = [render(c.to(DEV), tgt, PipelineParams(), torch.zeros(3, device=DEV))["render"].cpu() for c in cams]
    pts = curves["curve_points"][::4].mean(1).numpy()
    CI.write_colmap(str(tmp_path / "room"), cams, maps, pts)
    return str(tmp_path / "room")


def _run(scan, graphed, report_at):
    from curve_gaussian_amd.gaussian_renderer import PipelineParams, render
    from curve_gaussian_amd.scene import GaussianCurveModel, Scene
    from curve_gaussian_amd.train_step import GraphedTrainStep, TrainStep
    gm = GaussianCurveModel(0, 12, device=DEV)
    scene = Scene(scan, gm, eval=True, device=DEV)
    assert len(scene.getTrainCameras()) == 12 and len(scene.getTestCameras()) == 2
    gts = [c.original_image[:1].contiguous() for c in scene.getTrainCameras()]
    ts = (GraphedTrainStep if graphed else TrainStep)(gm, scene.getTrainCameras(), gts, seed=5)
    losses, reports = [], []
    bg = torch.zeros(3, device=DEV)
    for it in range(1, 9):
        losses.append(float(ts.step()[0]))
        if it in (3, 6):
            if graphed:
                ts.finish()
            if report_at:
                reports.append(E.training_report(None, it, None, None, None, 0.0, [it], scene, render,
                                                 (PipelineParams(), bg), False))
    if graphed:
        ts.finish()
    return losses, reports, gm


@pytest.mark.parametrize("graphed", [False, True])
def test_replica_like_scan_trains_and_reports_without_changing_the_trajectory(tmp_path, graphed):
    scan = _replica_scan(tmp_path)
    plain, _, g0 = _run(scan, graphed, False)
    with_reports, reports, g1 = _run(scan, graphed, True)
    assert np.isfinite(plain).all()
    assert plain == with_reports
    # (the backward's float atomics may order the last step's gradient sums differently from run to run: the end state is
    # held to a tolerance, the loss sequence above to the bit)
    torch.testing.assert_close(g0._curve_points.detach(), g1._curve_points.detach(), rtol=0, atol=1e-5)
    assert [list(r) for r in reports] == [["test", "train"]] * 2
    for r in reports:
        for v in r.values():
            assert np.isfinite(v["l1"]) and np.isfinite(v["psnr"]) and 0 <= v["l1"] <= 1
