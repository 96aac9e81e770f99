"""Cost of draw_ellipsoids' parts: the two record kernels, the device-to-host copy of the mesh body and
the whole write_ellipsoid_mesh call, for random splats at the BASELINE sizes (cfg2 ~50 k splats, cfg3 200 004).

    python profiles/probes/ellipsoid_mesh.py [--splats 50000 200004] [--reps 5] [--dir /tmp]

Kernel times here are event-timed over one launch each; under ``rocprofv3 --kernel-trace --stats -- python ...`` the
per-kernel table gives the same figures without the launch gaps.  One JSON line per size."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from curve_gaussian_amd.scene.snapshot_viz import EllipsoidMesh, write_ellipsoid_mesh  # noqa: E402


def splats(P, dev, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    xyz = torch.rand(P, 3, generator=g)
    rot = torch.nn.functional.normalize(torch.randn(P, 4, generator=g))
    scale = torch.exp(torch.randn(P, 3, generator=g) - 5)
    rgb = torch.rand(P, 3, generator=g)
    return [t.to(dev) for t in (xyz, rot, scale, rgb)]


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--splats", type=int, nargs="+", default=[50_000, 200_004])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dir", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for P in args.splats:
        m = EllipsoidMesh(*splats(P, dev))
        vb, fb = m.chunk_bytes(P, m.V0 * 27), m.chunk_bytes(P, m.F0 * 13)
        vbuf = torch.empty(vb, dtype=torch.uint8, device=dev)
        fbuf = torch.empty(fb, dtype=torch.uint8, device=dev)
        kv = timed(lambda: m.vertices_into(vbuf, 0, P), args.reps)
        kf = timed(lambda: m.faces_into(fbuf, 0, P), args.reps)
        pin = torch.empty(vb + fb, dtype=torch.uint8, pin_memory=True)

        def d2h():
            pin[:vb].copy_(vbuf, non_blocking=True)
            pin[vb:].copy_(fbuf, non_blocking=True)
        copy = timed(d2h, args.reps)
        with tempfile.TemporaryDirectory(dir=args.dir) as d:
            path = os.path.join(d, "m.ply")
            walls = []
            for _ in range(max(2, args.reps // 2)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                write_ellipsoid_mesh(path, m.xyz, m.rot, m.scale, m.rgb)
                walls.append(time.perf_counter() - t0)
            size = os.path.getsize(path)
            raw = os.path.join(d, "raw.bin")       # the same bytes from host memory: the file system's share
            t0 = time.perf_counter()
            with open(raw, "wb") as fh:
                fh.write(memoryview(pin.numpy()))
            disk = time.perf_counter() - t0
        gbs = lambda nbytes, ms: nbytes / ms / 1e6
        print(json.dumps({"splats": P, "vertex_kernel_ms": round(kv, 3), "vertex_GBps": round(gbs(vb, kv), 1),
                          "face_kernel_ms": round(kf, 3), "face_GBps": round(gbs(fb, kf), 1), "body_bytes": vb + fb,
                          "d2h_copy_ms": round(copy, 2), "d2h_GBps": round(gbs(vb + fb, copy), 1),
                          "write_ellipsoid_mesh_s": [round(w, 3) for w in walls], "file_bytes": size,
                          "host_file_write_s": round(disk, 3)}), flush=True)
        del vbuf, fbuf, pin, m


if __name__ == "__main__":
    main()
