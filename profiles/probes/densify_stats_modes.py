"""Densification-phase iteration time: the eager direct step with the reference's statistics lines (train.py:184-187, a
boolean-mask index and its host sync) against the same step with the statistics kernel (densification_stats=True), and
the graphed step without and with the captured kernel (run on the GPU box):
    python profiles/probes/densify_stats_modes.py [cfg2] [n] [warm-up steps]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from curve_gaussian_amd import synthetic as S  # noqa: E402
from curve_gaussian_amd.scene import GaussianCurveModel  # noqa: E402
from curve_gaussian_amd.train_step import GraphedTrainStep, TrainStep  # noqa: E402


def reference_lines(g, pkg):
    radii, grad = pkg["radii"], pkg["viewspace_points"].grad
    vis = radii > 0
    g.max_radii2D[vis] = torch.max(g.max_radii2D[vis], radii[vis])
    g.add_densification_stats(pkg["viewspace_points"], vis)


def timed(ts, n, after=None, graphed=False):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        _, pkg = ts.step()
        if after is not None:
            after(ts.g, pkg)
    if graphed:
        ts.finish()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def main():
    cfg = sys.argv[1] if len(sys.argv) > 1 else "cfg2"
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    warm = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    dev = torch.device("cuda:0")
    curves, cams = S.make_config(cfg, n_views=8)
    cams = [c.to(dev) for c in cams]
    H, W = cams[0].image_height, cams[0].image_width
    g = torch.Generator().manual_seed(1)
    gts = [((torch.rand(1, H, W, generator=g) > 0.97).float() * torch.rand(1, H, W, generator=g)).to(dev) for _ in cams]
    for mode in ("eager_reference_lines", "eager_kernel", "graphed_none", "graphed_kernel"):
        gm = GaussianCurveModel(0, 12, device=dev).create_from_curves(curves["curve_points"], curves["width"],
                                                                      curves["opacity"], curves["mask"], curves["is_bezier"])
        gm.training_setup()
        gm.densification_buffers()
        stats = mode.endswith("kernel")
        kw = dict(regularisers=True, densification_stats=stats, densify_until_iter=10 ** 6)
        graphed = mode.startswith("graphed")
        ts = GraphedTrainStep(gm, cams, gts, **kw) if graphed else TrainStep(gm, cams, gts, direct=True, **kw)
        after = reference_lines if mode == "eager_reference_lines" else None
        timed(ts, warm, after, graphed)
        ms = [timed(ts, n, after, graphed) for _ in range(3)]
        print(f"{cfg} {mode}: " + " ".join(f"{m:.4f}" for m in ms) + f" ms per iteration ({n} steps x 3 after {warm})")


if __name__ == "__main__":
    main()
