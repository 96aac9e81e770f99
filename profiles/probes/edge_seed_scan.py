"""python profiles/probes/edge_seed_scan.py [--views 100] [--width 1600] [--height 1200] [--grids 128 256] [--host_grid 128]
                                           [--host_views 2] [--host_slab 2] [--trace_only] [--out FILE]

Times ``ops.edge_seed.seed_points`` with each back end (profiles/edge_seed.md).  The scan: ``--views`` cameras on a sphere
around the unit cube, every edge map a set of random polylines two pixels wide, as profiles/probes/edge_score_scan.py
draws its detected masks (the maps of different views are NOT consistent with one 3D scene: the kernels' cost does not
depend on that, the number of seeds does).  Per grid: three end-to-end runs (the first pays the library load and the
allocator's warm-up), then ``voxel_votes`` alone between device events, then the library's own per-kernel timers.
``--trace_only``: one warm-up and one run per grid and nothing else, for a ``rocprofv3 --kernel-trace --stats`` run.
The host back end is timed on ``--host_views`` views for the distance transform and packing, and on a slab of
``--host_slab`` z-layers of the ``--host_grid`` grid for the votes of all views; both are scaled, and said to be."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

# float64 operations of one (voxel, view) pair, counted from the definition: three rows ((a X + b Y) + c Z) + t = 9
# multiplications and 9 additions, two divisions, u = fx x + cx and v = fy y + cy = 2 and 2.  Comparisons, floor and
# conversions are not counted.  (The compiled loop issues 51 float64 vector instructions per pair: 13 mul, 11 add, 10 fma,
# 4 div_scale, 2 rcp, 2 div_fmas, 2 div_fixup, 2 floor, 5 compares -- an IEEE division is 11 of them.)
FLOP_PER_PAIR = 24
PEAK_FP64_VECTOR_TFLOPS = 78.6   # MI355X data sheet, an FMA counted as two; without contraction half of it is reachable


def edge_map(seed, H, W, lines=60):
    from PIL import Image, ImageDraw
    rng = np.random.default_rng(seed)
    det = Image.new("L", (W, H), 0)
    dd = ImageDraw.Draw(det)
    for _ in range(lines):
        x, y = rng.uniform(0, W), rng.uniform(0, H)
        pts = [(x, y)]
        for _ in range(rng.integers(1, 4)):
            x, y = x + rng.uniform(-0.25, 0.25) * W, y + rng.uniform(-0.25, 0.25) * H
            pts.append((x, y))
        dd.line(pts, fill=255, width=2)
    return np.array(det, np.uint8)


def cameras(n, H, W):
    import math
    from curve_gaussian_amd import synthetic as S
    from curve_gaussian_amd.edge_extraction.novel_view import NovelViewCamera
    out = []
    for k, c in enumerate(S.fibonacci_cameras(n, H, W)):
        w2c = c.world_view_transform.double().numpy().T
        out.append(NovelViewCamera(f"v{k}", np.ascontiguousarray(w2c[:3, :3]), w2c[:3, 3].copy(), W / (2 * math.tan(c.FoVx / 2)),
                                   H / (2 * math.tan(c.FoVy / 2)), W / 2.0, H / 2.0, W, H))
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--views", type=int, default=100)
    p.add_argument("--width", type=int, default=1600)
    p.add_argument("--height", type=int, default=1200)
    p.add_argument("--grids", type=int, nargs="+", default=[128, 256])
    p.add_argument("--host_grid", type=int, default=128)
    p.add_argument("--host_views", type=int, default=2)
    p.add_argument("--host_slab", type=int, default=2)
    p.add_argument("--trace_only", action="store_true")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import torch
    from curve_gaussian_amd import _lib as L
    from curve_gaussian_amd.edge_extraction.novel_view import camera_arrays
    from curve_gaussian_amd.ops import edge_score as ES
    from curve_gaussian_amd.ops import edge_seed as SD
    if not torch.cuda.is_available():
        raise SystemExit("edge_seed_scan: needs a GPU; nothing is measured without one")
    H, W, V = a.height, a.width, a.views
    bounds = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    t0 = time.perf_counter()
    maps = np.stack([edge_map(k, H, W) for k in range(V)])
    cams = cameras(V, H, W)
    print(f"{V} views {W}x{H} drawn in {time.perf_counter() - t0:.1f} s; detected pixels {(maps > 127).mean():.4f}", flush=True)
    result = {"views": V, "width": W, "height": H, "grids": {}}
    dev = torch.device("cuda", 0)
    lib = L.load()
    for grid in a.grids:
        entry = result["grids"].setdefault(str(grid), {})
        for run in range(2 if a.trace_only else 3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            seeds, info = SD.seed_points(cams, maps, "PidiNet", bounds, grid=grid, backend="gpu", device=dev)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print(f"grid {grid}: backend=gpu run {run}: {dt:.3f} s end to end (maps uploaded from the host, counts read back, "
                  f"selection and thinning on the host); {info}", flush=True)
            entry.setdefault("gpu_seconds", []).append(dt)
        entry["info"] = {k: (list(v) if isinstance(v, tuple) else v) for k, v in info.items()}
        if a.trace_only:
            continue
        # voxel_votes alone: the masks stay on the device, device events around `reps` calls
        intr, w2c = camera_arrays(cams)
        det = torch.from_numpy((maps > 127).astype(np.uint8)).to(dev)
        bits = SD.near_bits(ES.edt_squared(det, "gpu", dev), 2, backend="gpu", device=dev)
        del det
        dims = SD.grid_dims(bounds, grid)
        counts = SD.voxel_votes(bounds, dims, intr, w2c, bits, H, W, backend="gpu", device=dev)   # warm-up
        reps = 5
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(reps):
            SD.voxel_votes(bounds, dims, intr, w2c, bits, H, W, backend="gpu", device=dev)
        stop.record()
        torch.cuda.synchronize()
        ms = start.elapsed_time(stop) / reps
        pairs = dims[0] * dims[1] * dims[2] * V
        tflops = FLOP_PER_PAIR * pairs / (ms * 1e-3) / 1e12
        entry.update({"voxel_votes_ms": ms, "pairs": pairs, "voxel_votes_tflops_fp64": tflops,
                      "share_of_fp64_vector_peak": tflops / PEAK_FP64_VECTOR_TFLOPS,
                      "seen_mean": float(counts[0].cpu().numpy().mean())})
        print(f"grid {grid}: voxel_votes {ms:.3f} ms per call over {reps} calls (includes the upload of {V} cameras), {pairs} "
              f"pairs, {FLOP_PER_PAIR} float64 operations each: {tflops:.2f} TFLOP/s = {100 * tflops / PEAK_FP64_VECTOR_TFLOPS:.1f} % "
              f"of {PEAK_FP64_VECTOR_TFLOPS} TFLOP/s", flush=True)
        lib.cgs_prof_reset()
        lib.cgs_prof_enable(1)
        SD.seed_points(cams, maps, "PidiNet", bounds, grid=grid, backend="gpu", device=dev)
        torch.cuda.synchronize()
        prof = L.prof_collect()
        lib.cgs_prof_enable(0)
        for name, (kms, n) in sorted(prof.items()):
            print(f"  {name}: {kms:.3f} ms in {n} launches", flush=True)
        entry["kernels_ms"] = {k: v[0] for k, v in prof.items()}
        del bits, counts
    if not a.trace_only:
        hv, grid = max(1, min(a.host_views, V)), a.host_grid
        dims = SD.grid_dims(bounds, grid)
        t0 = time.perf_counter()
        bits_h = SD.near_bits(ES.edt_squared((maps[:hv] > 127).astype(np.uint8), "host"), 2, backend="host")
        t_maps = time.perf_counter() - t0
        slab = max(1, min(a.host_slab, dims[2]))
        step_z = (bounds[1][2] - bounds[0][2]) / dims[2]
        sub = (bounds[0], (bounds[1][0], bounds[1][1], bounds[0][2] + slab * step_z))
        intr, w2c = camera_arrays(cams)
        # the slab is voted by every view; the packed masks beyond the first `hv` views are the first ones repeated (the
        # cost of a gather does not depend on the mask's content)
        bits_all = bits_h[torch.arange(V) % hv]
        t0 = time.perf_counter()
        SD.voxel_votes(sub, (dims[0], dims[1], slab), intr, w2c, bits_all, H, W, backend="host")
        t_votes = time.perf_counter() - t0
        scaled = t_maps / hv * V + t_votes / slab * dims[2]
        print(f"backend=host, grid {grid}: distance transform + packing {t_maps:.2f} s for {hv} views; votes {t_votes:.2f} s for "
              f"{slab} of {dims[2]} z-layers over {V} views; SCALED to the scan: {t_maps / hv * V:.1f} s + "
              f"{t_votes / slab * dims[2]:.1f} s = {scaled:.1f} s", flush=True)
        result["host"] = {"grid": grid, "views_timed": hv, "maps_seconds": t_maps, "slab_layers": slab, "votes_seconds": t_votes,
                          "scaled_seconds": scaled}
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
