"""Novel-view rendering at a Replica-sized case: ~10^6 edge points, 1200x680, 200 COLMAP-like views.  Prints one JSON
line: GPU time per view (cgs_render_points alone, device events; and the driver's render + uint8 conversion + copy to
the host) and PNG-encoding time per view of edge_extraction.novel_view.render_views (16 writer threads).

    python profiles/probes/novel_view_replica.py [--views 200] [--points 1000000] [--out DIR]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from curve_gaussian_amd.edge_extraction import novel_view as NV  # noqa: E402


def scene(P, V, W, H, seed=0):
    g = np.random.default_rng(seed)
    # points along random line segments inside a 4 m room, 0.5 mm apart, as the 0.0005 sampling makes them
    n_edges = P // 2000
    a = g.uniform(-2, 2, (n_edges, 1, 3))
    d = g.normal(size=(n_edges, 1, 3))
    d /= np.linalg.norm(d, axis=2, keepdims=True)
    t = (np.arange(2000) * 0.0005)[None, :, None]
    pts = (a + t * d).reshape(-1, 3).astype(np.float32)
    cols = np.repeat(NV.fancy_colors(n_edges + 1)[:n_edges].numpy(), 2000, 0)
    cams = []
    for v in range(V):
        yaw = 2 * np.pi * v / V
        Rm = np.array([[np.cos(yaw), 0, -np.sin(yaw)], [0, 1, 0], [np.sin(yaw), 0, np.cos(yaw)]])
        cams.append(NV.NovelViewCamera(f"frame_{v:04d}.png", Rm, np.array([0.0, 0.0, 2.5]), 600.0, 600.0, W / 2, H / 2,
                                       W, H))
    return pts, cols, cams


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=200)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    W, H = 1200, 680
    pts, cols, cams = scene(a.points, a.views, W, H)
    dev = torch.device("cuda:0")
    dp, dc = torch.from_numpy(pts).to(dev), torch.from_numpy(cols).to(dev)
    intr, w2c = NV.camera_arrays(cams)
    per = max(1, NV.OUTPUT_BUDGET // (H * W * 12))
    NV.render_points(dp, dc, intr[:per], w2c[:per], H, W)           # warm-up
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    kept = 0
    for b in range(0, len(cams), per):
        _, k = NV.render_points(dp, dc, intr[b:b + per], w2c[b:b + per], H, W, return_kept=True)
        kept += int(k.sum())
    e1.record()
    torch.cuda.synchronize()
    kernel_ms = e0.elapsed_time(e1)
    out = a.out or tempfile.mkdtemp()
    t = time.perf_counter()
    st = NV.render_views(pts, cols, cams, out, [c.name for c in cams], dev)
    wall = time.perf_counter() - t
    print(json.dumps({"points": len(pts), "views": len(cams), "width": W, "height": H, "kept_per_view": kept / len(cams),
                      "render_points_ms_per_view": kernel_ms / len(cams),
                      "driver_gpu_ms_per_view": 1e3 * st["gpu_s"] / len(cams),
                      "png_write_ms_per_view": 1e3 * st["write_s"] / len(cams), "written": st["written"],
                      "driver_wall_s": wall}))


if __name__ == "__main__":
    main()
