"""python profiles/probes/edge_seed_exclusive.py [--views 100] [--width 1600] [--height 1200] [--grid 128] [--reps 200]
                                                [--min_ratio 0.8] [--host_views 4] [--alt_lib FILE] [--out FILE]

Times the ray-exclusive claim pass of ``ops.edge_seed`` on the GPU (profiles/edge_seed_exclusive.md).  The scan: ``--views``
cameras on a sphere around the unit cube and the edge maps of ONE 3D scene -- 80 random segments, every sample drawn into
every view --, so that the vote keeps tubes of voxels and the list is what a scan gives (random maps keep nothing).

  1. the first sweep by hand (distance transform, packing, votes; chunked like ``seed_points``), the selection, the list
     (``--min_ratio`` below the default of 0.8 keeps fatter tubes: a longer list and more voxels per pixel)
  2. ``cgs_ray_claims`` (with its clear) and ``cgs_ray_wins`` alone, raw calls between device events, ``--reps`` calls each
     after a warm-up, everything resident; the results compared once with the host back end on the first ``--host_views``
     views
  3. the whole second sweep as ``seed_points`` runs it (upload of the list and cameras, allocation of ``best``, the two
     calls, the read-back, ``select_exclusive``) by the wall clock around a synchronise, three times
  4. ``seed_points`` end to end without and with the option, three runs each, alternating
  5. the host back end's second sweep on ``--host_views`` views, SCALED to the scan and said to be
  6. with ``--alt_lib``: a second build of the library (an experiment on k_ray_claims) timed against the default in
     alternating rounds in this process, on the same device buffers."""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def scene_maps(V, H, W, segments=80, samples=4000, seed=0):
    """(NovelViewCamera s, uint8 [V,H,W] PidiNet-style maps) of random segments in the unit cube."""
    from curve_gaussian_amd import synthetic as S
    from curve_gaussian_amd.edge_extraction.novel_view import NovelViewCamera
    rng = np.random.default_rng(seed)
    a, b = rng.uniform(0.1, 0.9, (segments, 1, 3)), rng.uniform(0.1, 0.9, (segments, 1, 3))
    t = np.linspace(0.0, 1.0, samples)[None, :, None]
    pts = (a * (1 - t) + b * t).reshape(-1, 3)
    cams, maps = [], np.zeros((V, H, W), np.uint8)
    for k, c in enumerate(S.fibonacci_cameras(V, H, W)):
        w2c = c.world_view_transform.double().numpy().T
        fx, fy = W / (2 * math.tan(c.FoVx / 2)), H / (2 * math.tan(c.FoVy / 2))
        cam = pts @ w2c[:3, :3].T + w2c[:3, 3]
        u, v = fx * cam[:, 0] / cam[:, 2] + W / 2.0, fy * cam[:, 1] / cam[:, 2] + H / 2.0
        ok = (cam[:, 2] > 0) & (u >= 0) & (u < W) & (v >= 0) & (v < H)
        maps[k, np.floor(v[ok]).astype(int), np.floor(u[ok]).astype(int)] = 255
        cams.append(NovelViewCamera(f"v{k}", np.ascontiguousarray(w2c[:3, :3]), w2c[:3, 3].copy(), fx, fy, W / 2.0, H / 2.0, W, H))
    return cams, maps


def events_ms(torch, call, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        call()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / reps


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--views", type=int, default=100)
    p.add_argument("--width", type=int, default=1600)
    p.add_argument("--height", type=int, default=1200)
    p.add_argument("--grid", type=int, default=128)
    p.add_argument("--reps", type=int, default=200)
    p.add_argument("--min_ratio", type=float, default=0.8)
    p.add_argument("--host_views", type=int, default=4)
    p.add_argument("--alt_lib", default=None)
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import torch
    from curve_gaussian_amd import _lib as L
    from curve_gaussian_amd.edge_extraction.novel_view import camera_arrays
    from curve_gaussian_amd.ops import edge_score as ES
    from curve_gaussian_amd.ops import edge_seed as SD
    if not torch.cuda.is_available():
        raise SystemExit("edge_seed_exclusive: needs a GPU; nothing is measured without one")
    dev = torch.device("cuda", 0)
    H, W, V = a.height, a.width, a.views
    bounds = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    t0 = time.perf_counter()
    cams, maps = scene_maps(V, H, W)
    print(f"{V} views {W}x{H} drawn in {time.perf_counter() - t0:.1f} s; detected pixels {(maps > 127).mean():.5f}", flush=True)
    result = {"views": V, "width": W, "height": H, "grid": a.grid, "min_ratio": a.min_ratio, "device": torch.cuda.get_device_name(dev)}

    # 1. the first sweep by hand, the near bits of every view kept on the device
    dims = SD.grid_dims(bounds, a.grid)
    intr, w2c = camera_arrays(cams)
    per = max(1, SD.BYTE_BUDGET // (SD.BYTES_PER_PIXEL * H * W))
    counts, parts = None, []
    for b in range(0, V, per):
        det = torch.from_numpy((maps[b:b + per] > 127).astype(np.uint8))
        bits = SD.near_bits(ES.edt_squared(det, backend="gpu", device=dev), 2, backend="gpu", device=dev)
        counts = SD.voxel_votes(bounds, dims, intr[b:b + per], w2c[b:b + per], bits, H, W, counts=counts, backend="gpu", device=dev)
        parts.append(bits)
    bits = torch.cat(parts)
    del parts
    seen, hit = (c.cpu().numpy() for c in counts)
    keep = SD.select_voxels(seen, hit, 3, a.min_ratio)
    index = np.nonzero(keep)[0].astype(np.int32)
    support = SD.voxel_support(seen, hit, index)
    M = int(index.size)
    print(f"grid {dims}: {M} kept voxels of {keep.size}; mean hit of the kept {hit[index].mean():.1f} of {V} views", flush=True)
    result.update({"dims": list(dims), "kept_voxels": M, "mean_hit": float(hit[index].mean())})

    # 2. the two kernels alone
    lib, stream = L.load(), L.raw_stream(dev)
    lo, hi = (np.asarray(x, np.float64) for x in bounds)
    lo_c, step_c = (C.c_double * 3)(*lo), (C.c_double * 3)(*((hi - lo) / np.array(dims, np.float64)))
    Kd, Md = torch.from_numpy(intr).to(dev), torch.from_numpy(np.ascontiguousarray(w2c.reshape(V, 12))).to(dev)
    idx_d, sup_d = torch.from_numpy(index).to(dev), support.to(dev)
    best = torch.empty((V, H, W), dtype=torch.int32, device=dev)
    wins = torch.empty(M, dtype=torch.uint16, device=dev)
    head = (dims[0], dims[1], dims[2], C.cast(lo_c, C.c_void_p), C.cast(step_c, C.c_void_p), M, L.ptr(idx_d), L.ptr(sup_d), V,
            L.ptr(Kd), L.ptr(Md), H, W, L.ptr(bits))
    claims = lambda library=lib, clear=1: L.check(library.cgs_ray_claims(*head, clear, L.ptr(best), stream), "cgs_ray_claims")
    count = lambda: L.check(lib.cgs_ray_wins(*head, L.ptr(best), SD.EXCL_WINDOW, SD.EXCL_MARGIN, 0, L.ptr(wins), stream),
                            "cgs_ray_wins")
    claims()
    count()
    torch.cuda.synchronize()
    hv = max(1, min(a.host_views, V))
    bits_h = bits[:hv].cpu()
    t0 = time.perf_counter()
    want_best = SD.ray_claims(bounds, dims, index, support, intr[:hv], w2c[:hv], bits_h, H, W, backend="host")
    t_host_claims = time.perf_counter() - t0
    t0 = time.perf_counter()
    want_wins = SD.ray_wins(bounds, dims, index, support, intr[:hv], w2c[:hv], bits_h, want_best, H, W, backend="host")
    t_host_wins = time.perf_counter() - t0
    assert torch.equal(best[:hv].cpu(), want_best), "cgs_ray_claims disagrees with the host back end"
    got = SD.ray_wins(bounds, dims, index, support, intr[:hv], w2c[:hv], bits[:hv], best[:hv], H, W, backend="gpu", device=dev)
    assert torch.equal(got.cpu(), want_wins), "cgs_ray_wins disagrees with the host back end"
    clear_ms = events_ms(torch, lambda: best.zero_(), a.reps)
    claims_ms = events_ms(torch, claims, a.reps)
    claims_noclear_ms = events_ms(torch, lambda: claims(lib, 0), a.reps)
    wins_ms = events_ms(torch, count, a.reps)
    claimed = int((best > 0).sum())
    print(f"cgs_ray_claims {claims_ms:.4f} ms per call with its clear of {best.numel() * 4 / 2 ** 20:.0f} MiB ({clear_ms:.4f} ms "
          f"for a zero_() alone), {claims_noclear_ms:.4f} ms without (every claim already in place); cgs_ray_wins {wins_ms:.4f} ms "
          f"per call; {a.reps} calls each; {claimed} pixels claimed", flush=True)
    result.update({"ray_claims_ms": claims_ms, "ray_claims_noclear_ms": claims_noclear_ms, "clear_ms": clear_ms,
                   "ray_wins_ms": wins_ms, "claimed_pixels": claimed})

    # 6. the other build of k_ray_claims, alternating with the default
    if a.alt_lib:
        alt = C.CDLL(os.path.abspath(a.alt_lib))
        alt.cgs_ray_claims.restype, alt.cgs_ray_claims.argtypes = L.SIGNATURES["cgs_ray_claims"]
        claims(alt)
        torch.cuda.synchronize()
        assert torch.equal(best[:hv].cpu(), want_best), "the other build disagrees with the host back end"
        rounds = {"default": [], "alt": []}
        for _ in range(a.rounds):
            rounds["default"].append(events_ms(torch, claims, a.reps))
            rounds["alt"].append(events_ms(torch, lambda: claims(alt), a.reps))
        for k, v in rounds.items():
            print(f"  k_ray_claims {k}: median {np.median(v):.4f} ms, min {min(v):.4f} ms, max {max(v):.4f} ms over {a.rounds} "
                  f"rounds of {a.reps} calls (clear included)", flush=True)
        result["claims_ab_ms"] = rounds
    del best, wins

    # 3. the second sweep as seed_points runs it
    sweep = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        b2 = SD.ray_claims(bounds, dims, index, support, intr, w2c, bits, H, W, backend="gpu", device=dev)
        w2 = SD.ray_wins(bounds, dims, index, support, intr, w2c, bits, b2, H, W, backend="gpu", device=dev)
        stay = SD.select_exclusive(w2, hit[index], SD.EXCL_WIN_RATIO)   # reads the wins back: a synchronise
        sweep.append(time.perf_counter() - t0)
        del b2, w2
    print(f"the second sweep as seed_points runs it: {[round(1e3 * s, 2) for s in sweep]} ms; {int(stay.sum())} of {M} voxels "
          f"stay", flush=True)
    result.update({"second_sweep_seconds": sweep, "exclusive_voxels": int(stay.sum())})
    del bits

    # 4. seed_points end to end, without and with the option
    runs = {"plain": [], "exclusive": []}
    for _ in range(3):
        for name, on in (("plain", False), ("exclusive", True)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            seeds, info = SD.seed_points(cams, maps, "PidiNet", bounds, grid=a.grid, min_ratio=a.min_ratio, backend="gpu", device=dev,
                                           exclusive=on)
            torch.cuda.synchronize()
            runs[name].append(time.perf_counter() - t0)
        print(f"seed_points end to end: plain {runs['plain'][-1]:.3f} s, exclusive {runs['exclusive'][-1]:.3f} s; {info}", flush=True)
    result["seed_points_seconds"] = runs
    lib.cgs_prof_reset()
    lib.cgs_prof_enable(1)
    SD.seed_points(cams, maps, "PidiNet", bounds, grid=a.grid, min_ratio=a.min_ratio, backend="gpu", device=dev, exclusive=True)
    torch.cuda.synchronize()
    prof = L.prof_collect()
    lib.cgs_prof_enable(0)
    for name, (kms, n) in sorted(prof.items()):
        print(f"  {name}: {kms:.3f} ms in {n} launches", flush=True)
    result["kernels_ms"] = {k: v[0] for k, v in prof.items()}

    # 5. the host back end, scaled
    scaled = (t_host_claims + t_host_wins) / hv * V
    print(f"backend=host: ray_claims {t_host_claims:.2f} s and ray_wins {t_host_wins:.2f} s for {hv} views of the same list; "
          f"SCALED to {V} views: {scaled:.1f} s", flush=True)
    result["host"] = {"views_timed": hv, "ray_claims_seconds": t_host_claims, "ray_wins_seconds": t_host_wins,
                      "scaled_seconds": scaled}
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
