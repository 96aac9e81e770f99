"""python profiles/probes/edge_thin.py [--views 100] [--width 1600] [--height 1200] [--distinct 10] [--segments 150]
                                        [--radii 1 2 4] [--reps 5] [--host_views 2] [--out FILE]

Times the thinning of detected masks, ``cgs_thin_masks`` (profiles/edge_thin.md).  The masks: ``--distinct`` different views
of ``--segments`` random one-pixel line segments each, repeated to ``--views`` views, dilated by a (2r+1) x (2r+1) square for
every r of ``--radii`` (strokes 3, 5 and 9 px wide at the defaults).  Per radius:

  1. the result of ``cgs_thin_masks`` on the first ``--host_views`` views compared with the host back end FIRST
     (``torch.equal``, and the iteration count), whose time is taken on the way and SCALED to the scan, said to be
  2. ``cgs_thin_masks`` on all views: ``--reps`` raw calls, each between device events on a fresh copy of the masks
     (the copy is outside the events), after a warm-up; its passes and iterations; the library's own event timers
     around the launches of one call
  3. ``edt_squared`` of the same views, thick and thinned, one call between device events, three times."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def segment_views(n, H, W, segments, seed=0):
    """uint8 [n,H,W]: random one-pixel line segments, 50 to 600 px long."""
    rng = np.random.default_rng(seed)
    out = np.zeros((n, H, W), np.uint8)
    for v in range(n):
        for _ in range(segments):
            y0, x0 = rng.uniform(0, H), rng.uniform(0, W)
            length, angle = rng.uniform(50, 600), rng.uniform(0, 2 * np.pi)
            t = np.linspace(0.0, 1.0, 2 * int(length) + 1)
            y, x = np.floor(y0 + t * length * np.sin(angle)).astype(int), np.floor(x0 + t * length * np.cos(angle)).astype(int)
            ok = (y >= 0) & (y < H) & (x >= 0) & (x < W)
            out[v, y[ok], x[ok]] = 1
    return out


def dilate(m, r):
    """[n,H,W] 0 / 1 dilated by a (2r+1) x (2r+1) square, one axis after the other."""
    rows = m.copy()
    for d in range(1, r + 1):
        rows[:, d:, :] |= m[:, :-d, :]
        rows[:, :-d, :] |= m[:, d:, :]
    out = rows.copy()
    for d in range(1, r + 1):
        out[:, :, d:] |= rows[:, :, :-d]
        out[:, :, :-d] |= rows[:, :, d:]
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--views", type=int, default=100)
    p.add_argument("--width", type=int, default=1600)
    p.add_argument("--height", type=int, default=1200)
    p.add_argument("--distinct", type=int, default=10)
    p.add_argument("--segments", type=int, default=150)
    p.add_argument("--radii", nargs="+", type=int, default=[1, 2, 4])
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--host_views", type=int, default=2)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import torch
    from curve_gaussian_amd import _lib as L
    from curve_gaussian_amd.ops import edge_score as ES
    from curve_gaussian_amd.ops import edge_thin as ET
    if not torch.cuda.is_available():
        raise SystemExit("edge_thin: needs a GPU; nothing is measured without one")
    dev = torch.device("cuda", 0)
    H, W, V = a.height, a.width, a.views
    lib, stream = L.load(), L.raw_stream(dev)
    thin_lines = segment_views(min(a.distinct, V), H, W, a.segments)
    result = {"views": V, "width": W, "height": H, "distinct": int(thin_lines.shape[0]), "segments": a.segments,
              "pass_iterations": L.THIN_PASS_ITERATIONS, "tile": [L.THIN_TILE_HEIGHT, L.THIN_TILE_WIDTH],
              "device": torch.cuda.get_device_name(dev), "radii": {}}
    hv = max(1, min(a.host_views, thin_lines.shape[0]))
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for r in a.radii:
        thick = dilate(thin_lines, r)
        reps_of_views = -(-V // thick.shape[0])
        src = torch.from_numpy(np.tile(thick, (reps_of_views, 1, 1))[:V]).to(dev)
        row = {"stroke_px": 2 * r + 1, "set_pixels": float(thick.mean())}

        # 1. equality first; the host's time on the way
        t0 = time.perf_counter()
        want, want_n = ET.thin_masks(thick[:hv], backend="host", return_iterations=True)
        t_host = time.perf_counter() - t0
        got, got_n = ET.thin_masks(src[:hv], backend="gpu", return_iterations=True)
        assert torch.equal(got.cpu(), want) and got_n == want_n, "cgs_thin_masks disagrees with the host back end"
        row["host"] = {"views_timed": hv, "seconds": t_host, "scaled_seconds": t_host / hv * V, "iterations": want_n}
        print(f"r = {r} ({2 * r + 1} px, {100 * thick.mean():.2f} % set): equal to the host back end on {hv} views "
              f"({want_n} iterations); backend=host {t_host:.2f} s, SCALED to {V} views: {t_host / hv * V:.1f} s", flush=True)

        # 2. the call
        work, scratch = torch.empty_like(src), torch.empty_like(src)
        flag = torch.empty((1,), dtype=torch.int32, device=dev)
        n = ctypes.c_int(0)

        def call():
            return L.check(lib.cgs_thin_masks(V, H, W, L.ptr(work), L.ptr(scratch), L.ptr(flag), 0, ctypes.byref(n), stream),
                           "cgs_thin_masks")
        work.copy_(src)
        passes = call()
        torch.cuda.synchronize()
        assert torch.equal(work[:hv].cpu(), want), "the call on all views disagrees with the host back end"
        ms = []
        for _ in range(a.reps):
            work.copy_(src)
            start.record()
            call()
            stop.record()
            torch.cuda.synchronize()
            ms.append(start.elapsed_time(stop))
        lib.cgs_prof_reset()
        lib.cgs_prof_enable(1)
        work.copy_(src)
        call()
        torch.cuda.synchronize()
        prof = L.prof_collect()
        lib.cgs_prof_enable(0)
        row.update({"thin_masks_ms": ms, "passes": passes, "iterations": n.value,
                    "kernels_ms": {k: list(v) for k, v in prof.items()}})
        print(f"  cgs_thin_masks: {[round(t, 3) for t in ms]} ms per call; {passes} passes, {n.value} iterations; "
              + ", ".join(f"{k}: {v[0]:.3f} ms in {v[1]} launches" for k, v in sorted(prof.items())), flush=True)

        # 3. the distance transform of the same views
        for name, masks in (("edt_squared_thick_ms", src), ("edt_squared_thinned_ms", work)):
            ES.edt_squared(masks, backend="gpu", device=dev)
            torch.cuda.synchronize()
            edt = []
            for _ in range(3):
                start.record()
                ES.edt_squared(masks, backend="gpu", device=dev)
                stop.record()
                torch.cuda.synchronize()
                edt.append(start.elapsed_time(stop))
            row[name] = edt
            print(f"  {name[:-3]}: {[round(t, 3) for t in edt]} ms per call (allocation of its outputs included)", flush=True)
        result["radii"][str(r)] = row
        del src, work, scratch
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
