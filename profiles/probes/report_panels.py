"""Cost of the training report's image panels: evaluation.report_panels -- two HIP launches for all views --
against the same panels written as the chain of torch ops the reference's loop amounts to on the device (clamp, max, divide,
table gather, normalize, quantise, one view and one panel at a time; the reference additionally goes through the host and
matplotlib for the depth panel, which is not timed here).

    python profiles/probes/report_panels.py [--sizes 1600x1600 680x1200] [--views 5] [--reps 20]

Device events around the whole call, median of --reps after a warm-up; the two kernels' own times from the library's
profiling hooks.  Bytes: per pixel 4 (render) + 4 Cg (gt) + 2 x 4 (depth, read by both kernels) + 12 (rend_dir) + 4 (alpha)
read and 15 written.  The outputs of the two routes are compared before anything is timed.  One JSON line per size."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import report_panels_ref64 as R  # noqa: E402
from curve_gaussian_amd import _lib as L  # noqa: E402
from curve_gaussian_amd import evaluation as E  # noqa: E402


def q(x):
    return (x * 255).clip(0, 255).to(torch.uint8)


def torch_panels(pkgs, gts, turbo):
    out = []
    for pkg, gt in zip(pkgs, gts):
        H, W = pkg["render"].shape[1:]
        grey = lambda x: q(x.clamp(0, 1)).permute(1, 2, 0).expand(H, W, 3)
        depth = pkg["depth"]
        idx = (depth[0] / depth.max() * 256).long().clamp(0, 255)
        n = torch.nn.functional.normalize(pkg["rend_dir"], dim=0) * 0.5 + 0.5
        out.append(torch.stack([grey(pkg["render"]), q(gt.clamp(0, 1)).permute(1, 2, 0).expand(H, W, 3), turbo[idx],
                                q(n).permute(1, 2, 0), grey(pkg["rend_alpha"])]))
    return out


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["1600x1600", "680x1200"])
    ap.add_argument("--views", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = L.load()
    turbo = torch.from_numpy(R.turbo8()).to(dev)
    for size in args.sizes:
        H, W = (int(a) for a in size.split("x"))
        views = [{k: torch.from_numpy(a).to(dev) for k, a in R.synthetic_view(v, H, W, 3).items()} for v in range(args.views)]
        pkgs, gts = views, [v["gt"] for v in views]
        mine, _ = E.report_panels(pkgs, gts)
        ref = torch_panels(pkgs, gts, turbo)
        differ = [int((a != b).any(-1).sum()) for a, b in zip(mine, ref)]
        hip = timed(lambda: E.report_panels(pkgs, gts), args.reps)
        tor = timed(lambda: torch_panels(pkgs, gts, turbo), args.reps)
        lib.cgs_prof_reset()
        lib.cgs_prof_enable(1)
        for _ in range(args.reps):
            E.report_panels(pkgs, gts)
        torch.cuda.synchronize()
        prof = {k: v for k, v in L.prof_collect().items() if k.startswith("report_")}
        lib.cgs_prof_enable(0)
        px = args.views * H * W
        kern = {k: round(ms / n, 4) for k, (ms, n) in prof.items()}
        moved = {"report_depth_max": 4 * px, "report_panels": (4 + 12 + 4 + 12 + 4 + 15) * px}
        print(json.dumps({"size": size, "views": args.views, "pixels_differing_from_torch_ops": differ,
                          "report_panels_call_ms": [round(t, 4) for t in hip],
                          "torch_ops_ms": [round(t, 4) for t in tor], "kernel_ms": kern,
                          "kernel_TBps": {k: round(moved[k] / (kern[k] * 1e9), 3) for k in kern if k in moved and kern[k] > 0}}),
              flush=True)


if __name__ == "__main__":
    main()
