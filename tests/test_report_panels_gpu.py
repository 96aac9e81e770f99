"""GPU: the report panel kernels (csrc/report.hip) and curve_gaussian_amd.evaluation.report_panels against the numpy
restatements of tests/report_panels_ref64.py, on synthetic views of mixed sizes and on a real render(); the edge cases of
the C ABI; training_report writing its image summaries through a ReportDirWriter.

render, ground_truth and rend_alpha are one clamp and one multiply: bit-equal to the float32 restatement.  depth and rend_dir
are held to the float64 restatement everywhere except at exempt pixels (report_panels_ref64.compare: within 1e-3 of a
quantisation step in float64, not on it), which may take the neighbouring table entry / level and must stay below 2 % of a
panel."""
import ctypes
import os

import numpy as np
import pytest
import torch

import report_panels_ref64 as R
from curve_gaussian_amd import _lib as L
from curve_gaussian_amd import evaluation as E
from curve_gaussian_amd import synthetic as S

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
# (H, W, gt channels): odd W, H*W not a multiple of 4 (so that planes and panels lose their alignment), one pixel, 1600^2
MIXED = [(37, 53, 3), (8, 9, 1), (1, 1, 1), (129, 64, 3), (300, 201, 1), (1600, 1600, 3), (5, 7, 3)]


def _to_dev(v):
    return {k: torch.from_numpy(a).to(DEV) for k, a in v.items()}


def _pkg(d):
    return {"render": d["render"], "depth": d["depth"], "rend_dir": d.get("rend_dir"), "rend_alpha": d["rend_alpha"]}


def _check_view(name, got, v):
    """got: uint8 [5,H,W,3] numpy; v: the view's numpy inputs (missing / None entries: that panel is not compared)."""
    p32, _ = R.panels32(**v)
    p64, _, pre = R.panels64(**v)
    shares = {}
    for p, key in ((0, "render"), (1, "gt"), (4, "rend_alpha")):
        if v.get(key) is not None:
            bad = int((got[p] != p32[p]).any(-1).sum())
            print(f"{name} {R.PANELS[p]}: {bad} pixels differ from the float32 restatement")
            assert bad == 0
    for p, key in ((2, "depth"), (3, "rend_dir")):
        if v.get(key) is not None:
            wrong, share = R.compare(key, got[p], p64[p], pre[key])
            off32 = int((got[p] != p32[p]).any(-1).sum())
            print(f"{name} {key}: exempt share {share:.4%}, wrong {wrong}, pixels off the float32 restatement {off32}")
            assert wrong == 0
            assert share <= 0.02
            shares[key] = share
    return shares


def test_mixed_sizes_match_the_restatements():
    views = [R.synthetic_view(100 + k, H, W, C) for k, (H, W, C) in enumerate(MIXED)]
    dev = [_to_dev(v) for v in views]
    panels, written = E.report_panels([_pkg(d) for d in dev], [d["gt"] for d in dev])
    assert written == [(True,) * 5] * len(MIXED)
    for k, ((H, W, C), v) in enumerate(zip(MIXED, views)):
        assert panels[k].shape == (5, H, W, 3) and panels[k].dtype == torch.uint8 and panels[k].device.type == "cuda"
        _check_view(f"{H}x{W}x{C}", panels[k].cpu().numpy(), v)
    # exactly integral values are not exempt and match: zero depth, the maximum pixel, zero and axis-aligned directions
    big = panels[5].cpu().numpy()
    d = views[5]["depth"][0]
    tb = R.turbo8()
    assert (big[2][d == 0] == tb[0]).all() and (big[2][d == d.max()] == tb[255]).all()
    assert (big[3][(views[5]["rend_dir"] == 0).all(0)] == 127).all()
    assert big[3].reshape(-1, 3)[:6].tolist() == [[255, 127, 127], [127, 255, 127], [127, 127, 255], [0, 127, 127],
                                                   [127, 0, 127], [127, 127, 0]]


def test_ten_views_take_one_call_and_every_view_is_its_own(monkeypatch):
    shapes = [(40 + 3 * k, 61 + k, 3 if k % 2 else 1) for k in range(10)]
    views = [R.synthetic_view(200 + k, H, W, C) for k, (H, W, C) in enumerate(shapes)]
    dev = [_to_dev(v) for v in views]
    lib = L.load()
    calls = []

    class _Counting:
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if name != "cgs_report_panels":
                return fn
            return lambda *a: (calls.append(a[0]), fn(*a))[1]

    monkeypatch.setattr(L, "load", lambda: _Counting())
    panels, _ = E.report_panels([_pkg(d) for d in dev], [d["gt"] for d in dev])
    assert calls == [10]
    alone, _ = E.report_panels([_pkg(dev[7])], [dev[7]["gt"]])
    assert calls == [10, 1]
    assert torch.equal(alone[0], panels[7])
    for k, v in enumerate(views):
        _check_view(f"view {k}", panels[k].cpu().numpy(), v)


def _abi_call(lib, table, ws, out):
    rc = lib.cgs_report_panels(len(table), ctypes.cast(table, ctypes.c_void_p), L.ptr(ws), L.ptr(out), L.raw_stream(DEV))
    return rc


def _table(dev_views, offsets):
    t = (L.ReportView * len(dev_views))()
    for k, (d, off) in enumerate(zip(dev_views, offsets)):
        ptr = lambda key: None if d.get(key) is None else d[key].data_ptr()
        H, W = d["depth"].shape[1:] if d.get("depth") is not None else d["render"].shape[1:]
        t[k] = L.ReportView(ptr("render"), ptr("gt"), ptr("depth"), ptr("rend_dir"), ptr("rend_alpha"),
                            1 if d.get("gt") is None else int(d["gt"].shape[0]), int(H), int(W), 0, off)
    return t


def test_missing_inputs_leave_their_panels_untouched_and_the_workspace_is_reusable():
    lib = L.load()
    H, W = 33, 47
    full = R.synthetic_view(7, H, W, 3)
    part = {k: (None if k in ("gt", "rend_dir") else a) for k, a in R.synthetic_view(8, H, W, 3).items()}
    dv = [_to_dev(full), {k: (None if a is None else torch.from_numpy(a).to(DEV)) for k, a in part.items()}]
    n = 5 * H * W * 3
    stride = (n + 15) & ~15
    out = torch.full((2 * stride,), 0xAB, dtype=torch.uint8, device=DEV)
    # the workspace starts as garbage: the call itself must (re-)initialise whatever state its reduction keeps
    ws = torch.full((int(lib.cgs_report_panels_workspace_bytes(2)),), 0xFF, dtype=torch.uint8, device=DEV)
    t = _table(dv, [0, stride])
    assert _abi_call(lib, t, ws, out) == 0
    assert [t[0].written, t[1].written] == [0b11111, 0b10101]
    first = out.clone()
    got = [out[k * stride:k * stride + n].view(5, H, W, 3).cpu().numpy() for k in range(2)]
    _check_view("full", got[0], full)
    _check_view("partial", got[1], part)
    assert (got[1][1] == 0xAB).all() and (got[1][3] == 0xAB).all()          # NULL gt, NULL rend_dir: not a byte written
    assert (out[n:stride] == 0xAB).all()                                     # nor between the views
    # a second call on the same workspace, and a third after a larger depth went through it: identical bytes
    out.fill_(0xAB)
    assert _abi_call(lib, t, ws, out) == 0
    assert torch.equal(out, first)
    other = _to_dev(R.synthetic_view(9, H, W, 3))
    other["depth"] = other["depth"] * 100
    scratch = torch.empty_like(out)
    assert _abi_call(lib, _table([other, other], [0, stride]), ws, scratch) == 0
    out.fill_(0xAB)
    assert _abi_call(lib, t, ws, out) == 0
    assert torch.equal(out, first)
    # through the Python surface: the mask says the same
    _, written = E.report_panels([_pkg(dv[1])])
    assert written == [(True, False, True, False, True)]


def test_zero_depth_is_black_and_nan_pixels_are_black():
    H, W = 21, 30
    v = R.synthetic_view(11, H, W, 1)
    z = dict(v, depth=np.zeros((1, H, W), np.float32))
    nan = dict(v, depth=v["depth"].copy(), rend_dir=v["rend_dir"].copy(), render=v["render"].copy())
    nan["depth"][0, 3, 4] = np.nan
    nan["depth"][0, 0, 0] = np.nan
    nan["rend_dir"][1, 5, 6] = np.nan
    nan["render"][0, 2, 2] = np.nan
    allnan = dict(v, depth=np.full((1, H, W), np.nan, np.float32))
    panels, _ = E.report_panels([_pkg(_to_dev(x)) for x in (z, nan, allnan)])
    got = [p.cpu().numpy() for p in panels]
    assert (got[0][2] == 0).all()
    assert (got[1][2][3, 4] == 0).all() and (got[1][2][0, 0] == 0).all()
    assert (got[1][2] != 0).any(-1).sum() == H * W - 2            # the maximum skipped the NaNs: everything else is coloured
    assert (got[1][3][5, 6] == 0).all() and (got[1][0][2, 2] == 0).all()
    assert (got[2][2] == 0).all()
    for name, g, x in (("zero", got[0], z), ("nan", got[1], nan), ("allnan", got[2], allnan)):
        _check_view(name, g, {k: a for k, a in x.items() if k != "gt"})


def test_argument_errors_are_raised():
    d = _to_dev(R.synthetic_view(3, 8, 9, 3))
    with pytest.raises(ValueError, match="height or width"):
        E.report_panels([dict(_pkg(d), depth=torch.zeros(1, 8, 8, device=DEV))])
    with pytest.raises(ValueError, match="height or width"):
        E.report_panels([_pkg(d)], [torch.zeros(3, 9, 9, device=DEV)])
    with pytest.raises(ValueError, match=r"C in \(1, 3\)"):
        E.report_panels([_pkg(d)], [torch.zeros(2, 8, 9, device=DEV)])
    with pytest.raises(ValueError, match="floating-point"):
        E.report_panels([dict(_pkg(d), rend_alpha=torch.zeros(1, 8, 9, dtype=torch.int32, device=DEV))])
    with pytest.raises(L.CurveGSError, match="GPU tensor"):
        E.report_panels([dict(_pkg(d), depth=d["depth"].cpu())])
    half = {k: a.half() for k, a in d.items()}                    # other float types are converted, as view_metrics does
    a, _ = E.report_panels([_pkg(half)], [half["gt"]])
    b, _ = E.report_panels([_pkg({k: x.float() for k, x in half.items()})], [half["gt"].float()])
    assert torch.equal(a[0], b[0])
    lib = L.load()
    ws = torch.empty(int(lib.cgs_report_panels_workspace_bytes(2)), dtype=torch.uint8, device=DEV)
    out = torch.zeros(2 * 5 * 8 * 9 * 3, dtype=torch.uint8, device=DEV)
    n = 5 * 8 * 9 * 3
    assert _abi_call(lib, _table([d, d], [0, n]), ws, out) == 0
    for bad in ([0, n - 1], [n - 1, 0], [0, 0]):
        assert _abi_call(lib, _table([d, d], bad), ws, out) == -1
        assert b"overlap" in lib.cgs_last_error()
    t = _table([d], [0])
    t[0].gt_channels = 2
    assert _abi_call(lib, t, ws, out) == -1
    t = _table([d], [0])
    t[0].height = 0
    assert _abi_call(lib, t, ws, out) == -1 and b"invalid argument" in lib.cgs_last_error()
    assert lib.cgs_report_panels(1, ctypes.cast(_table([d], [0]), ctypes.c_void_p), None, L.ptr(out), L.raw_stream(DEV)) == -1
    torch.cuda.synchronize()


def test_the_call_can_be_captured_and_replayed_with_changed_inputs():
    shapes = [(45, 67, 3), (30, 31, 1)]
    first = [R.synthetic_view(300 + k, H, W, C) for k, (H, W, C) in enumerate(shapes)]
    second = [R.synthetic_view(400 + k, H, W, C) for k, (H, W, C) in enumerate(shapes)]
    second[0]["depth"] *= 3                                         # another maximum
    bufs = [_to_dev(v) for v in first]
    panels, _ = E.report_panels([_pkg(d) for d in bufs], [d["gt"] for d in bufs])     # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        panels, _ = E.report_panels([_pkg(d) for d in bufs], [d["gt"] for d in bufs])
    for inputs in (second, first):
        for d, v in zip(bufs, inputs):
            for k, a in v.items():
                d[k].copy_(torch.from_numpy(a))
        graph.replay()
        torch.cuda.synchronize()
        for k, v in enumerate(inputs):
            _check_view(f"replay view {k}", panels[k].cpu().numpy(), v)


def _model(B=600, seed=4):
    from curve_gaussian_amd.scene import GaussianCurveModel
    c = S.make_curves(B, seed, room_scale=True)
    return GaussianCurveModel(0, 12, device=DEV).create_from_curves(c["curve_points"], c["width"], c["opacity"], c["mask"],
                                                                    c["is_bezier"])


def _scene_cameras(n, seed=3):
    cams = [c.to(DEV) for c in S.room_cameras(n, 68, 120, 4)]
    g = torch.Generator().manual_seed(seed)
    for i, c in enumerate(cams):
        c.original_image = (torch.rand(3 if i % 2 else 1, 68, 120, generator=g) * 1.2 - 0.1).to(DEV)
        c.image_name = f"frame_{i:03d}"
    return cams


def test_a_real_render_matches_the_restatements():
    from curve_gaussian_amd.gaussian_renderer import PipelineParams, render
    gm = _model()
    cams = _scene_cameras(4)
    bg = torch.zeros(3, device=DEV)
    with torch.no_grad():
        pkgs = [render(c, gm, PipelineParams(), bg) for c in cams]
        panels, written = E.report_panels(pkgs, [c.original_image for c in cams])
    assert written == [(True,) * 5] * 4
    for k, (pkg, cam) in enumerate(zip(pkgs, cams)):
        v = {"render": pkg["render"], "gt": cam.original_image, "depth": pkg["depth"], "rend_dir": pkg["rend_dir"],
             "rend_alpha": pkg["rend_alpha"]}
        v = {key: t.detach().float().cpu().numpy() for key, t in v.items()}
        assert v["depth"].max() > 0 and (v["rend_alpha"] > 0).any()
        _check_view(f"render {k}", panels[k].cpu().numpy(), v)


class _Scene:
    def __init__(self, train, test, gaussians):
        self.train, self.test, self.gaussians = train, test, gaussians

    def getTrainCameras(self):
        return self.train

    def getTestCameras(self):
        return self.test


def test_training_report_writes_the_panels_and_keeps_the_metrics(tmp_path, capsys):
    from PIL import Image
    from curve_gaussian_amd.gaussian_renderer import PipelineParams, render
    gm = _model()
    cams = _scene_cameras(9)
    scene = _Scene(cams[2:], cams[:2], gm)
    bg = torch.zeros(3, device=DEV)
    args = (None, None, None, None, [7, 9], scene, render, (PipelineParams(), bg), False)
    plain = E.training_report(None, 7, *args)
    line = capsys.readouterr().out
    writer = E.ReportDirWriter(tmp_path / "rep")
    with_writer = E.training_report(writer, 7, *args)
    assert with_writer == plain and list(plain) == ["test", "train"]
    assert capsys.readouterr().out == line
    folder = tmp_path / "rep" / "images" / "iter_000007"
    shown = {"test": cams[:2], "train": [scene.train[i % 7] for i in range(5, 30, 5)]}
    expect = sorted(f"{cfg}_view_{c.image_name}__{kind}.png" for cfg, cs in shown.items() for c in cs for kind in R.PANELS)
    assert sorted(os.listdir(folder)) == sorted(set(expect))
    with torch.no_grad():
        for cfg, cs in shown.items():
            for c in cs:
                pkg = render(c, gm, PipelineParams(), bg)
                panels, _ = E.report_panels([pkg], [c.original_image])
                ref = panels[0].cpu().numpy()
                for p, kind in enumerate(R.PANELS):
                    png = np.asarray(Image.open(folder / f"{cfg}_view_{c.image_name}__{kind}.png"))
                    assert (png == ref[p]).all(), (cfg, c.image_name, kind)
    # a later test iteration: no ground truth; the scalars of both reports are in the file
    E.training_report(writer, 9, *args)
    later = os.listdir(tmp_path / "rep" / "images" / "iter_000009")
    assert len(later) == len(set(expect)) * 4 // 5 and not any("ground_truth" in f for f in later)
    import json
    tags = [json.loads(x)["tag"] for x in open(tmp_path / "rep" / "scalars.jsonl")]
    assert tags == ["total_points", "test/loss_viewpoint - l1_loss", "test/loss_viewpoint - psnr",
                    "train/loss_viewpoint - l1_loss", "train/loss_viewpoint - psnr"] * 2
