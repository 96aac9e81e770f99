"""python profiles/probes/edge_detect_scan.py [--views 100] [--width 1600] [--height 1200] [--dir DIR]

Times ``python -m curve_gaussian_amd.edge_detect`` with each back end on a synthetic EMAP scan: smooth colour fields with
polygons and a little noise (profiles/edge_detect.md).  The scan is written once; each run decodes the photographs, detects
and writes the PNGs, as a user's run does."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def photograph(seed, H, W):
    from PIL import Image, ImageDraw
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    planes = []
    for _ in range(3):
        f = np.zeros((H, W), np.float32)
        for _ in range(4):
            kx, ky, ph = rng.uniform(-0.02, 0.02), rng.uniform(-0.02, 0.02), rng.uniform(0, 6.28)
            f += rng.uniform(0.1, 0.3) * np.sin(kx * xx + ky * yy + ph)
        planes.append(np.clip(0.5 + 0.5 * f, 0, 1))
    img = Image.fromarray((np.stack(planes, -1) * 255).round().astype(np.uint8), mode="RGB")
    draw = ImageDraw.Draw(img)
    for _ in range(12):
        cx, cy = rng.uniform(0, W), rng.uniform(0, H)
        pts = [(cx + rng.uniform(-0.2, 0.2) * W, cy + rng.uniform(-0.2, 0.2) * H) for _ in range(rng.integers(3, 7))]
        draw.polygon(pts, fill=tuple(int(v) for v in rng.integers(0, 256, 3)))
    a = np.array(img, dtype=np.int16) + rng.integers(-2, 3, (H, W, 3))
    return Image.fromarray(np.clip(a, 0, 255).astype(np.uint8), mode="RGB")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--views", type=int, default=100)
    p.add_argument("--width", type=int, default=1600)
    p.add_argument("--height", type=int, default=1200)
    p.add_argument("--dir", default=None)
    a = p.parse_args()
    import torch
    from curve_gaussian_amd import edge_detect as tool
    from curve_gaussian_amd import synthetic as S
    from curve_gaussian_amd.scene import dataset_io as IO
    scan = a.dir or tempfile.mkdtemp(prefix="edge_detect_scan_")
    t0 = time.perf_counter()
    cams = S.room_cameras(a.views, 8, 8, 4)
    IO.write_emap(scan, cams, [torch.zeros(1, 8, 8)] * a.views)
    os.makedirs(os.path.join(scan, "color"), exist_ok=True)
    for k in range(a.views):
        photograph(k, a.height, a.width).save(os.path.join(scan, "color", f"{k}_colors.png"))
    print(f"scan of {a.views} views {a.width}x{a.height} written in {time.perf_counter() - t0:.1f} s", flush=True)
    result = {"views": a.views, "width": a.width, "height": a.height}
    for backend in ("gpu", "gpu", "host"):      # the first device run pays the library load and the allocator's warm-up
        t0 = time.perf_counter()
        tool.detect_scan(scan, backend=backend, overwrite=True)
        dt = time.perf_counter() - t0
        meta = json.load(open(os.path.join(scan, "edge_PidiNet", "detector.json")))
        print(f"backend={backend}: {dt:.2f} s, propagation rounds per call {meta['propagation_rounds']}", flush=True)
        result[backend] = {"seconds": dt, "rounds": meta["propagation_rounds"]}
    from curve_gaussian_amd import _lib as L
    from curve_gaussian_amd.ops import edge_detect as E
    from PIL import Image
    lib = L.load()
    chunk = [torch.from_numpy(np.array(Image.open(os.path.join(scan, "color", f"{k}_colors.png")))).cuda()
             for k in range(min(a.views, L.EDGE_MAX_VIEWS))]
    E.detect_edges(chunk)
    lib.cgs_prof_reset()
    lib.cgs_prof_enable(1)
    E.detect_edges(chunk)
    torch.cuda.synchronize()
    prof = L.prof_collect()
    lib.cgs_prof_enable(0)
    for name, (ms, n) in sorted(prof.items()):
        print(f"  {name}: {ms:.3f} ms in {n} launches ({len(chunk)} views on the device)")
    result["kernels_ms"] = {k: v[0] for k, v in prof.items()}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
