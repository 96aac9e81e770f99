"""python profiles/probes/edge_score_scan.py [--views 100] [--width 1600] [--height 1200] [--host_views 4] [--out FILE]

Times ``ops.edge_score.score_masks`` with each back end on synthetic masks (profiles/edge_score.md): the detected mask of a
view is a set of random polylines two pixels wide, the prediction the same polylines one pixel wide and moved by a pixel or
two, a fifth of them left out and a few added -- what an extraction that mostly works looks like.  The host back end is
timed on ``--host_views`` views and scaled to the view count."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def masks(seed, H, W, lines=60):
    from PIL import Image, ImageDraw
    rng = np.random.default_rng(seed)
    det, pred = Image.new("L", (W, H), 0), Image.new("L", (W, H), 0)
    dd, dp = ImageDraw.Draw(det), ImageDraw.Draw(pred)
    for k in range(lines):
        x, y = rng.uniform(0, W), rng.uniform(0, H)
        pts = [(x, y)]
        for _ in range(rng.integers(1, 4)):
            x, y = x + rng.uniform(-0.25, 0.25) * W, y + rng.uniform(-0.25, 0.25) * H
            pts.append((x, y))
        dd.line(pts, fill=1, width=2)
        if k % 5:
            ox, oy = rng.uniform(-2, 2, 2)
            dp.line([(px + ox, py + oy) for px, py in pts], fill=1, width=1)
    for _ in range(lines // 10):
        x, y = rng.uniform(0, W), rng.uniform(0, H)
        dp.line([(x, y), (x + rng.uniform(-0.2, 0.2) * W, y + rng.uniform(-0.2, 0.2) * H)], fill=1, width=1)
    return np.array(pred, np.uint8), np.array(det, np.uint8)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--views", type=int, default=100)
    p.add_argument("--width", type=int, default=1600)
    p.add_argument("--height", type=int, default=1200)
    p.add_argument("--host_views", type=int, default=4)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import torch
    from curve_gaussian_amd import _lib as L
    from curve_gaussian_amd.ops import edge_score as ES
    t0 = time.perf_counter()
    pairs = [masks(k, a.height, a.width) for k in range(a.views)]
    pred, det = np.stack([q[0] for q in pairs]), np.stack([q[1] for q in pairs])
    print(f"{a.views} views {a.width}x{a.height} drawn in {time.perf_counter() - t0:.1f} s; set pixels: pred "
          f"{pred.mean():.4f}, det {det.mean():.4f}", flush=True)
    result = {"views": a.views, "width": a.width, "height": a.height}
    lib = L.load()
    for run in range(3):        # the first device run pays the library load and the allocator's warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = ES.score_masks(pred, det, (1, 2, 4), backend="gpu")
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print(f"backend=gpu run {run}: {dt:.3f} s (masks uploaded from the host)", flush=True)
        result.setdefault("gpu_seconds", []).append(dt)
    result["aggregate"] = res["aggregate"]
    lib.cgs_prof_reset()
    lib.cgs_prof_enable(1)
    ES.score_masks(pred, det, (1, 2, 4), backend="gpu")
    torch.cuda.synchronize()
    prof = L.prof_collect()
    lib.cgs_prof_enable(0)
    for name, (ms, n) in sorted(prof.items()):
        print(f"  {name}: {ms:.3f} ms in {n} launches", flush=True)
    result["kernels_ms"] = {k: v[0] for k, v in prof.items()}
    hv = max(1, min(a.host_views, a.views))
    t0 = time.perf_counter()
    host = ES.score_masks(pred[:hv], det[:hv], (1, 2, 4), backend="host")
    dt = time.perf_counter() - t0
    print(f"backend=host: {dt:.2f} s for {hv} views, {dt / hv * a.views:.1f} s scaled to {a.views}", flush=True)
    result["host_seconds"], result["host_views"] = dt, hv
    for k in ("n_pred", "n_det", "pred_hits", "det_hits"):
        assert torch.equal(host[k], res[k][:hv]), k
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
