#!/usr/bin/env python
"""Generates tests/golden/eval_metrics.npz by IMPORTING the reference's train.py and calling its ``training_report``
(train.py:321-376) on CPU with a stub scene and a stub ``renderFunc`` that hands back fixed renders; the printed
``[ITER i] Evaluating <config>: L1 <l1> PSNR <psnr>`` lines are captured (printed at full precision) and parsed.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_eval_golden.py

Imported through make_model_golden.import_reference (placeholders for the packages this image lacks, poisoned before
anything is called); ``.to("cuda")`` stays on the CPU under make_colmap_golden.CudaOnCpu.  Cases: a one-channel render
against three-channel and one-channel edge maps, values outside [0, 1] in both, views of different sizes,
``train_test_exp``, an exact match (PSNR inf), and a scene with no test cameras (the empty config is skipped).
Recorded per case: every render / edge map, the order in which the reference rendered the cameras, and the printed
values per config."""
import contextlib
import io
import os
import re
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_colmap_golden import CudaOnCpu  # noqa: E402
from make_model_golden import _ARMED, import_reference  # noqa: E402


class View:
    def __init__(self, idx, name, gt):
        self.idx, self.image_name, self.original_image = idx, name, gt


class StubScene:
    def __init__(self, train, test):
        self.train, self.test = train, test
        self.gaussians = object()

    def getTrainCameras(self):
        return self.train

    def getTestCameras(self):
        return self.test


def main():
    TR = import_reference("train")
    _ARMED[0] = True
    torch.set_printoptions(precision=17)
    g = torch.Generator().manual_seed(20261016)
    out = {}

    def view(idx, H, W, C, lo=-0.2, hi=1.3, exact=False):
        render = lo + (hi - lo) * torch.rand(1, H, W, generator=g)
        gt = lo + (hi - lo) * torch.rand(C, H, W, generator=g)
        if exact:
            gt = render.clone().repeat(C, 1, 1)
        return View(idx, f"v{idx}", gt), render

    cases = {
        # name: (test views, train views, train_test_exp)
        "rgb_gt": ([(12, 16, 3), (9, 20, 3), (12, 16, 1)], [(12, 16, 1), (10, 14, 3), (12, 16, 3), (8, 8, 1), (12, 16, 1),
                                                          (6, 10, 3), (12, 16, 1)], False),
        "half": ([(12, 17, 3), (9, 20, 1)], [(12, 16, 1), (12, 15, 3), (7, 9, 1)], True),
        "exact_no_test": ([], [(8, 12, 1, "exact"), (8, 12, 3, "exact")], False),
    }
    names = []
    for case, (test_spec, train_spec, tte) in cases.items():
        views, renders = [], {}
        for i, spec in enumerate(test_spec + train_spec):
            v, r = view(i, *spec[:3], exact=len(spec) > 3)
            views.append(v)
            renders[i] = r
        test, train = views[:len(test_spec)], views[len(test_spec):]
        order = []

        def render_func(viewpoint, gaussians, *args):
            order.append(viewpoint.idx)
            return {"render": renders[viewpoint.idx]}

        buf = io.StringIO()
        with CudaOnCpu(), contextlib.redirect_stdout(buf):
            TR.training_report(None, 7000, None, None, TR.l1_loss, 0.0, [7000], StubScene(train, test), render_func, (),
                               tte)
        printed = re.findall(r"Evaluating (\w+): L1 (?:tensor\()?([-+.\w]+)\S* PSNR (?:tensor\()?([-+.\w]+)", buf.getvalue())
        names.append(case)
        out[f"{case}_n_test"] = np.array(len(test))
        out[f"{case}_n_train"] = np.array(len(train))
        out[f"{case}_train_test_exp"] = np.array(tte)
        out[f"{case}_order"] = np.array(order)
        out[f"{case}_configs"] = np.array([p[0] for p in printed])
        out[f"{case}_l1"] = np.array([float(p[1]) for p in printed])
        out[f"{case}_psnr"] = np.array([float(p[2]) for p in printed])
        for i, v in enumerate(views):
            out[f"{case}_render_{i}"] = renders[i].numpy()
            out[f"{case}_gt_{i}"] = v.original_image.numpy()
        print(case, list(zip(out[f"{case}_configs"], out[f"{case}_l1"], out[f"{case}_psnr"])), "order", order)
    out["cases"] = np.array(names)
    np.savez_compressed(os.path.join(HERE, "eval_metrics.npz"), **out)


if __name__ == "__main__":
    main()
