"""python profiles/probes/edge_seed_directions.py [--grid 128] [--seeds 20000] [--radii 6 15] [--reps 20] [--out FILE]

Times ``ops.edge_seed.voxel_moments`` on the GPU (profiles/edge_seed_directions.md).  The kept voxels: tubes of radius 1.5
voxels around random segments through a ``--grid``^3 grid; the centres: ``--seeds`` kept voxels drawn at random (with
repetition when there are fewer).  Per radius: one warm-up call, then ``--reps`` calls of the raw entry point between device
events (bits and centres resident), the result compared once with the host back end on the first 256 seeds; then the host
parts of ``seed_points(directions=True)`` -- ``keep_bits`` and ``seed_directions`` -- by the wall clock."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def tubes(grid, segments, rng):
    keep = np.zeros((grid, grid, grid), bool)   # [z][y][x]
    for _ in range(segments):
        a, b = rng.uniform(0, grid, 3), rng.uniform(0, grid, 3)
        t = np.linspace(0.0, 1.0, 4 * grid)[:, None]
        p = a[None, :] * (1 - t) + b[None, :] * t
        for off in np.ndindex(4, 4, 4):
            q = np.floor(p).astype(int) + (np.array(off) - 1)
            ok = ((q >= 0) & (q < grid)).all(1)
            near = (((q + 0.5 - p) ** 2).sum(1) <= 1.5 ** 2) & ok
            keep[q[near, 2], q[near, 1], q[near, 0]] = True
    return keep


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--grid", type=int, default=128)
    p.add_argument("--seeds", type=int, default=20000)
    p.add_argument("--segments", type=int, default=60)
    p.add_argument("--radii", type=int, nargs="+", default=[6, 15])
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    import torch
    from curve_gaussian_amd import _lib as L
    from curve_gaussian_amd.ops import edge_seed as SD
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    dims = (args.grid,) * 3
    keep = tubes(args.grid, args.segments, rng)
    kz, ky, kx = np.nonzero(keep)
    pick = rng.choice(len(kx), args.seeds, replace=len(kx) < args.seeds)
    centres = np.stack([kx[pick], ky[pick], kz[pick]], 1).astype(np.int64)
    t0 = time.perf_counter()
    bits = SD.keep_bits(keep.reshape(-1), dims)
    keep_bits_ms = (time.perf_counter() - t0) * 1e3
    result = {"grid": args.grid, "seeds": args.seeds, "kept_voxels": int(keep.sum()), "keep_bits_host_ms": keep_bits_ms,
              "device": torch.cuda.get_device_name(dev), "radii": {}}
    bits_d = bits.to(dev)
    cen_d = torch.from_numpy(centres.astype(np.int32)).to(dev)
    out = torch.empty((args.seeds, SD.MOMENT_VALUES), dtype=torch.int32, device=dev)
    lib, stream = L.load(), L.raw_stream(dev)
    for r in args.radii:
        call = lambda: L.check(lib.cgs_voxel_moments(*dims, L.ptr(bits_d), args.seeds, L.ptr(cen_d), r, L.ptr(out), stream),
                               "cgs_voxel_moments")
        call()
        torch.cuda.synchronize(dev)
        want = SD.voxel_moments(bits, dims, centres[:256], r, backend="host")
        assert torch.equal(out[:256].cpu(), want), "the kernel disagrees with the host back end"
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(args.reps):
            call()
        stop.record()
        torch.cuda.synchronize(dev)
        ms = start.elapsed_time(stop) / args.reps
        t0 = time.perf_counter()
        _, directed, _ = SD.seed_directions(out)
        host_ms = (time.perf_counter() - t0) * 1e3
        result["radii"][r] = {"voxel_moments_ms": ms, "mean_support": float(out[:, 0].double().mean()),
                              "seed_directions_host_ms": host_ms, "directed": int(directed.sum())}
        print(f"r = {r}: voxel_moments {ms:.4f} ms per call over {args.reps} calls ({args.seeds} seeds, mean support "
              f"{result['radii'][r]['mean_support']:.1f}), seed_directions on the host {host_ms:.1f} ms, directed {int(directed.sum())}")
    print(f"keep_bits on the host: {keep_bits_ms:.1f} ms for {args.grid}^3 voxels")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
