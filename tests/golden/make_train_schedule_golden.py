#!/usr/bin/env python
"""Generates tests/golden/train_schedule.json: the call log of the reference's own training() (train.py:38-248) over its
whole schedule, by IMPORTING the reference's train.py and arguments/__init__.py and running training() on recording fakes
(tests/train_fakes.py) in place of the model, scene, render, losses, report, extract_curves and torch.save.  Runs only
where the reference checkout exists; the JSON (data only) travels.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_train_schedule_golden.py

Imported like the other make_*golden.py scripts: make_model_golden.import_reference, placeholders for the packages this
image lacks, poisoned before training() runs; ``.cuda()`` / ``.to("cuda")`` stay on the CPU (make_colmap_golden.CudaOnCpu)
and the module's ``torch`` is a proxy whose ``cuda.Event``, ``save`` and ``device="cuda"`` factories stay on the CPU.
Runs: the defaults (10 000 iterations), the Replica variant, a run resumed from chkpnt3000, and the shortened options
of the GPU test (5 000 iterations, densification 100 / 200 / 1000, opacity reset 500)."""
import contextlib
import io
import json
import os
import sys
import tempfile
import types

import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_colmap_golden import CudaOnCpu  # noqa: E402
from make_model_golden import _ARMED, import_reference  # noqa: E402

import train_fakes as TF  # noqa: E402

GPU_OPTIONS = ["--iterations", "5000", "--densify_from_iter", "100", "--densification_interval", "200",
               "--densify_until_iter", "1000", "--opacity_reset_interval", "500"]
GPU_LISTS = dict(test=[3000, 5000], save=[3000, 5000], checkpoint=[2000, 5000])


class _Event:
    def __init__(self, **k):
        pass

    def record(self):
        pass

    def elapsed_time(self, other):
        return 0.0


def _torch_proxy(rec):
    cuda = types.SimpleNamespace(Event=_Event, empty_cache=lambda: None)
    strip = lambda f: (lambda *a, **k: f(*a, **{kk: v for kk, v in k.items() if kk != "device"}))
    over = {"cuda": cuda, "save": lambda obj, path: rec.add("checkpoint"), "tensor": strip(torch.tensor),
            "rand": strip(torch.rand), "load": lambda p: torch.load(p, weights_only=False)}
    return types.SimpleNamespace(**{**{k: getattr(torch, k) for k in dir(torch) if not k.startswith("__")}, **over})


def run(T, ARG, opt_cls, argv, lists, checkpoint=None):
    from argparse import ArgumentParser
    rec = TF.Recorder()
    parser = ArgumentParser(conflict_handler="resolve")
    lp, op, pp = ARG.ModelParams(parser), opt_cls(parser), ARG.PipelineParams(parser)
    args = parser.parse_args(["-s", "scan", "-m", "out"] + argv)
    opt = op.extract(args)
    model = TF.FakeModel(rec)
    T.GaussianCurveModel = lambda *a, **k: model
    T.Scene = lambda dataset, gaussians: TF.FakeScene(rec, gaussians)
    T.render = TF.fake_render(rec)
    T.edge_aware_loss = lambda image, gt: (image - gt).abs().mean()
    T.fused_ssim = lambda a, b: a.mean() * 0 + 0.5
    T.prepare_output_and_logger = lambda dataset: None
    T.training_report = lambda tb, it, *a: rec.add("report") if it in a[4] else None
    T.extract_curves = lambda gaussians, opt, scene: rec.add("export")
    T.randint = __import__("random").Random(0).randint
    T.torch = _torch_proxy(rec)
    saves = list(lists["save"]) + [opt.iterations]          # train.py:404
    with CudaOnCpu(), contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        T.training(lp.extract(args), opt, pp.extract(args), lists["test"], saves, lists["checkpoint"], checkpoint, -1)
    rec.iteration = opt.iterations
    return TF.compress(TF.normalise(rec.log))


def main():
    T = import_reference("train")
    ARG = import_reference("arguments")
    _ARMED[0] = True
    torch.set_num_threads(1)
    defaults = dict(test=[3000, 10000], save=[3000, 10000], checkpoint=[10000])    # train.py:386-391
    out = {"source": "train.py:38-248 of the reference, run on tests/train_fakes.py", "runs": {}}
    out["runs"]["defaults"] = dict(argv=[], lists=defaults, log=run(T, ARG, ARG.OptimizationParams, [], defaults))
    out["runs"]["replica"] = dict(argv=[], lists=defaults, log=run(T, ARG, ARG.OptimizationParamsReplica, [], defaults))
    with tempfile.TemporaryDirectory() as d:
        ck = os.path.join(d, "chkpnt3000.pth")
        torch.save(({"fake": True}, 3000), ck)
        out["runs"]["resumed3000"] = dict(argv=[], lists=defaults, checkpoint=3000,
                                          log=run(T, ARG, ARG.OptimizationParams, [], defaults, checkpoint=ck))
    out["runs"]["gpu_options"] = dict(argv=GPU_OPTIONS, lists=GPU_LISTS,
                                      log=run(T, ARG, ARG.OptimizationParams, GPU_OPTIONS, GPU_LISTS))
    dst = os.path.join(HERE, "train_schedule.json")
    with open(dst, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
