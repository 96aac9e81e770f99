"""CPU: the training report's image summaries without a GPU -- the committed colour map against matplotlib's, the two numpy
restatements of the panel arithmetic (tests/report_panels_ref64.py) against each other, ReportDirWriter's files, the tags
training_report hands to a writer against the reference's (train.py:346-364), and the driver's --report_dir."""
import json
import os

import numpy as np
import pytest
import torch

import report_panels_ref64 as R
import train_fakes as TF

SIZES = [(37, 53, 3), (8, 9, 1), (1, 1, 1), (129, 64, 3), (300, 201, 1)]


def test_turbo_table_is_matplotlibs():
    matplotlib = pytest.importorskip("matplotlib")
    ref = np.asarray(matplotlib.colormaps["turbo"].colors, np.float64)
    mine = R.turbo_table()
    assert mine.shape == (256, 3) and ref.shape == (256, 3)
    assert (mine == ref).all()
    # the 8-bit colours do not depend on the precision the table is quantised in
    assert (R.turbo8() == R.q(mine)).all()


def test_library_exports_the_report_symbols():
    from curve_gaussian_amd import _lib as L
    lib = L.load()
    assert lib.cgs_report_panels_workspace_bytes(10) >= 10 * 4
    assert lib.cgs_report_panels_workspace_bytes(0) == lib.cgs_report_panels_workspace_bytes(1)
    assert lib.cgs_report_panels(0, None, None, None, None) == 0
    for bad in (-1, L.REPORT_MAX_VIEWS + 1):
        assert lib.cgs_report_panels(bad, None, None, None, None) == -1
        assert b"invalid argument" in lib.cgs_last_error()
    assert lib.cgs_report_panels(1, None, None, None, None) == -1      # NULL table: rejected before any device work
    assert L.REPORT_PANELS == R.PANELS


@pytest.mark.parametrize("H,W,C", SIZES)
def test_float32_and_float64_restatements_agree(H, W, C):
    v = R.synthetic_view(H * 1000 + W, H, W, C)
    p32, w32 = R.panels32(**v)
    p64, w64, pre = R.panels64(**v)
    assert w32 == w64 == (True,) * 5
    for p in (0, 1, 4):     # one clamp, one multiply by 255 of a float32 value: the same bytes in either precision
        assert (p32[p] == p64[p]).all(), R.PANELS[p]
    for p, kind in ((2, "depth"), (3, "rend_dir")):
        wrong, share = R.compare(kind, p32[p], p64[p], pre[kind])
        print(f"{H}x{W} {kind}: exempt share {share:.4%}, wrong {wrong}")
        assert wrong == 0
        assert share <= 0.02
    # values that are integral in exact arithmetic are not exempt and agree: zero depth, the view's maximum, zero and
    # axis-aligned directions
    d = v["depth"][0]
    tb = R.turbo8()
    if d.max() > 0:
        assert (p32[2][d == 0] == tb[0]).all() and (p32[2][d == d.max()] == tb[255]).all()
    else:
        assert (p32[2] == 0).all()           # (the 1 x 1 view) an all-zero depth map is black
    zero = (v["rend_dir"] == 0).all(0)
    assert (p32[3][zero] == 127).all()
    flat = p32[3].reshape(-1, 3)
    if H * W >= 6:
        assert zero.any() and flat[0].tolist() == [255, 127, 127] and flat[4].tolist() == [127, 0, 127]


def test_restatement_edge_cases():
    z = np.zeros((1, 4, 5), np.float32)
    assert (R.panels32(depth=z)[0][2] == 0).all()                       # an all-zero view: black, not turbo[0]
    d = np.linspace(0, 3, 20, dtype=np.float32).reshape(1, 4, 5)
    d[0, 1, 2] = np.nan
    p, w = R.panels32(depth=d)
    assert w == (False, False, True, False, False)
    assert (p[2][1, 2] == 0).all() and (p[2][3, 4] == R.turbo8()[255]).all()     # the maximum skips the NaN
    assert (p[[0, 1, 3, 4]] == 0).all()
    a = np.array([[[-1.0, 0.0, 0.5, 1.0, 7.0, np.nan]]], np.float32)
    assert R.panels32(rend_alpha=a)[0][4][0, :, 0].tolist() == [0, 0, 127, 255, 255, 0]


def test_report_dir_writer_files(tmp_path):
    from PIL import Image
    from curve_gaussian_amd.evaluation import ReportDirWriter
    w = ReportDirWriter(tmp_path / "rep")
    g = torch.Generator().manual_seed(0)
    panel = torch.randint(0, 256, (7, 9, 3), generator=g, dtype=torch.uint8)
    w.add_images("test_view_r_0/depth", panel[None], global_step=300, dataformats="NHWC")
    w.add_scalar("test/loss_viewpoint - psnr", 21.5, 300)
    w.add_scalar("total_points", 1200, 300)
    path = tmp_path / "rep" / "images" / "iter_000300" / "test_view_r_0__depth.png"
    assert sorted(os.listdir(tmp_path / "rep")) == ["images", "scalars.jsonl"]
    assert os.listdir(path.parent) == [path.name]
    assert (np.asarray(Image.open(path)) == panel.numpy()).all()
    lines = [json.loads(x) for x in open(tmp_path / "rep" / "scalars.jsonl")]
    assert lines == [{"tag": "test/loss_viewpoint - psnr", "value": 21.5, "step": 300},
                     {"tag": "total_points", "value": 1200.0, "step": 300}]
    # a batch: image k > 0 gets its index; one channel is written as a grey image
    batch = torch.randint(0, 256, (2, 4, 6, 1), generator=g, dtype=torch.uint8)
    w.add_images("a/b", batch, global_step=1, dataformats="NHWC")
    for k, name in enumerate(("a__b.png", "a__b_1.png")):
        got = np.asarray(Image.open(tmp_path / "rep" / "images" / "iter_000001" / name))
        assert (got == batch[k, :, :, 0].numpy()).all()
    # anything else is refused, not reinterpreted: the default layout of a tensorboard writer, a float image
    with pytest.raises(ValueError, match="NHWC"):
        w.add_images("t", panel[None], 1)
    with pytest.raises(ValueError, match="uint8"):
        w.add_images("t", panel[None].float(), 1, dataformats="NHWC")


class _Recorder:
    """A writer that records its calls."""

    def __init__(self):
        self.scalars, self.images = [], []

    def add_scalar(self, tag, value, step=None):
        self.scalars.append((tag, step))

    def add_images(self, tag, img, global_step=None, dataformats="NCHW"):
        self.images.append((tag, tuple(img.shape), img.dtype, global_step, dataformats))


class _ScalarsOnly:
    def __init__(self):
        self.scalars = []

    def add_scalar(self, tag, value, step=None):
        self.scalars.append((tag, step))


class _Cam:
    def __init__(self, name):
        self.image_name = name
        self.original_image = torch.zeros(1, 4, 6)


class _Scene:
    def __init__(self, n_train, n_test):
        self.train = [_Cam(f"tr{i}") for i in range(n_train)]
        self.test = [_Cam(f"te{i}") for i in range(n_test)]
        self.gaussians = type("G", (), {"get_xyz": torch.zeros(11, 3)})()

    def getTrainCameras(self):
        return self.train

    def getTestCameras(self):
        return self.test


def _report_on_cpu(monkeypatch, writer, iteration, tests, scene, half=False, with_dir=True):
    """training_report with the two device calls replaced: report_panels by a stand-in that records its arguments and
    returns panels of the right shape, the metric reduction by constants."""
    from curve_gaussian_amd import evaluation as E
    calls = []

    def fake_panels(pkgs, gts=None):
        calls.append((len(pkgs), None if gts is None else len(gts)))
        has_dir = pkgs[0].get("rend_dir") is not None
        H, W = pkgs[0]["render"].shape[1:]
        return ([torch.zeros(5, H, W, 3, dtype=torch.uint8) for _ in pkgs],
                [(True, gts is not None, True, has_dir, True)] * len(pkgs))

    monkeypatch.setattr(E, "report_panels", fake_panels)
    monkeypatch.setattr(E, "_summarise", lambda images, gts, half_width: {"l1": 0.25, "psnr": 12.0, "views": len(images)})

    def render_func(viewpoint, gaussians, *args):
        m = torch.zeros(1, 4, 6)
        return {"render": m, "depth": m, "rend_alpha": m, "rend_dir": torch.zeros(3, 4, 6) if with_dir else None}

    out = E.training_report(writer, iteration, torch.tensor(0.5), torch.tensor(0.7), None, 0.01, tests, scene, render_func,
                            (), half)
    return out, calls


def _expected_tags(scene, first):
    kinds = ["render"] + (["ground_truth"] if first else []) + ["depth", "rend_dir", "rend_alpha"]
    train = [scene.train[i % len(scene.train)] for i in range(5, 30, 5)]
    return [f"{cfg}_view_{c.image_name}/{k}" for cfg, cams in (("test", scene.test[:5]), ("train", train[:5]))
            for c in cams for k in kinds]


def test_image_summaries_carry_the_reference_tags(monkeypatch, capsys):
    scene = _Scene(n_train=12, n_test=7)
    w = _Recorder()
    out, calls = _report_on_cpu(monkeypatch, w, 300, [300, 600], scene)
    assert out == {"test": {"l1": 0.25, "psnr": 12.0}, "train": {"l1": 0.25, "psnr": 12.0}}
    assert "[ITER 300] Evaluating test: L1 0.25 PSNR 12.0" in capsys.readouterr().out
    assert calls == [(5, 5), (5, 5)]                    # one report_panels call per config, at most five views, with gts
    assert [t for t, *_ in w.images] == _expected_tags(scene, first=True)
    assert len(w.images) == 2 * 5 * 5
    for tag, shape, dtype, step, fmt in w.images:
        assert shape == (1, 4, 6, 3) and dtype == torch.uint8 and step == 300 and fmt == "NHWC"
    assert [t for t, _ in w.scalars] == ["train_loss_patches/l1_loss", "train_loss_patches/total_loss", "iter_time",
                                         "total_points", "test/loss_viewpoint - l1_loss", "test/loss_viewpoint - psnr",
                                         "train/loss_viewpoint - l1_loss", "train/loss_viewpoint - psnr"]
    # a later test iteration: no ground truth, and report_panels is not given any
    w2 = _Recorder()
    out2, calls2 = _report_on_cpu(monkeypatch, w2, 600, [300, 600], scene)
    assert out2 == out and calls2 == [(5, None), (5, None)]
    assert [t for t, *_ in w2.images] == _expected_tags(scene, first=False)
    assert len(w2.images) == 2 * 5 * 4 and all(step == 600 for *_, step, _f in w2.images)


def test_image_summaries_respect_the_writer_and_the_schedule(monkeypatch):
    scene = _Scene(n_train=3, n_test=2)
    # not a test iteration: the per-iteration scalars only
    w = _Recorder()
    out, calls = _report_on_cpu(monkeypatch, w, 301, [300], scene)
    assert out == {} and calls == [] and w.images == [] and len(w.scalars) == 4
    # a writer without add_images keeps working and report_panels is never called
    s = _ScalarsOnly()
    out, calls = _report_on_cpu(monkeypatch, s, 300, [300], scene)
    assert calls == [] and len(s.scalars) == 8 and list(out) == ["test", "train"]
    # no writer: nothing but the metrics
    out_none, calls = _report_on_cpu(monkeypatch, None, 300, [300], scene)
    assert calls == [] and out_none == out
    # fewer than five views: all of them, the train config's five picks wrap around the three cameras
    w = _Recorder()
    _, calls = _report_on_cpu(monkeypatch, w, 300, [300], scene)
    assert calls == [(2, 2), (5, 5)]
    assert [t for t, *_ in w.images] == _expected_tags(scene, first=True)
    # train_test_exp: render and ground truth are summarised as their right halves, the other panels whole
    w = _Recorder()
    _report_on_cpu(monkeypatch, w, 300, [300], scene, half=True)
    shapes = {t.rsplit("/", 1)[1]: shape for t, shape, *_ in w.images}
    assert shapes == {"render": (1, 4, 3, 3), "ground_truth": (1, 4, 3, 3), "depth": (1, 4, 6, 3), "rend_dir": (1, 4, 6, 3),
                      "rend_alpha": (1, 4, 6, 3)}
    # a render function without a direction map: that tag is left out
    w = _Recorder()
    _report_on_cpu(monkeypatch, w, 300, [300], scene, with_dir=False)
    assert not any(t.endswith("/rend_dir") for t, *_ in w.images) and len(w.images) == 7 * 4


def test_report_panels_has_no_cpu_fallback():
    from curve_gaussian_amd import _lib as L
    from curve_gaussian_amd.evaluation import report_panels
    m = torch.zeros(1, 4, 4)
    with pytest.raises(L.CurveGSError, match="GPU tensor"):
        report_panels([{"render": m, "depth": m, "rend_alpha": m}])
    with pytest.raises(ValueError, match="no 'depth'"):
        report_panels([{"render": m, "rend_alpha": m}])
    with pytest.raises(ValueError, match="no views"):
        report_panels([])
    with pytest.raises(ValueError, match="1 views but 2 ground truths"):
        report_panels([{"render": m, "depth": m, "rend_alpha": m}], [m, m])


def test_driver_accepts_report_dir(tmp_path):
    from curve_gaussian_amd import train as T
    _, _, args = T.parse_args(["-s", "scan", "-m", "out", "--report_dir", str(tmp_path / "rep")])
    assert args.report_dir == str(tmp_path / "rep")
    assert T.parse_args(["-s", "scan", "-m", "out"])[2].report_dir is None


def _run_driver(tmp_path, **kw):
    from curve_gaussian_amd import train as T
    rec = TF.Recorder()
    model = TF.FakeModel(rec)
    scene = TF.FakeScene(rec, model)
    opt = T.OptimizationParams(iterations=1200, densify_from_iter=100, densification_interval=200, densify_until_iter=600,
                               opacity_reset_interval=500)
    step = TF.FakeStep(rec, model, opt.densify_until_iter)
    dataset = T.ModelParams(source_path="scan", model_path=str(tmp_path / "out"))
    out = T.training(dataset, opt, [300, 900], [600, 1200], [1200], None, quiet=True, scene=(scene, model), step=step,
                     save_ply=lambda g, path, it: rec.add("save"), save_checkpoint=lambda obj, path: rec.add("checkpoint"),
                     export=lambda g, d, o: rec.add("export"), **kw)
    return out["events"], rec.log


def test_driver_event_log_does_not_depend_on_the_writer(tmp_path, monkeypatch):
    from curve_gaussian_amd import train as T
    seen = []
    monkeypatch.setattr(T, "_report", lambda it, tests, scene, bg, writer=None: seen.append((it, writer)))
    base = _run_driver(tmp_path, report=lambda it, tests, sc, bg: None)
    none = _run_driver(tmp_path, report_writer=None)
    assert seen == [(300, None), (900, None)]
    w = _Recorder()
    with_writer = _run_driver(tmp_path, report_writer=w)
    assert seen[2:] == [(300, w), (900, w)]
    assert base == none == with_writer
    assert [(it, name) for it, name, _ in base[0] if name == "report"] == [(300, "report"), (900, "report")]
