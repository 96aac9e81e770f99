"""k_view_fwd with and without the training gate at cfg3 (profiles/train_gate.md): the library's own per-kernel timers
(cgs_prof_enable) around repeated cgs_view_forward / cgs_view_forward_depth calls, three rounds, one JSON line.

    python profiles/probes/train_gate.py [--lib PATH] [--rounds 3] [--iters 200]

--lib: another build of libcurvegs.so to time instead (the parent commit's, for the before / after comparison of the
ungated kernel); a library without the gated entry is timed ungated only.  The gate's planes are those of a sphere of
radius 0.4 around the cloud's centre, drawn by mesh_depth for the same cameras."""
import argparse
import ctypes as C
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from curve_gaussian_amd import _lib as L   # noqa: E402
from curve_gaussian_amd import synthetic as S   # noqa: E402

DEV = torch.device("cuda:0")
NAMES = ("cgs_view_forward", "cgs_view_forward_depth", "cgs_geometry_bytes", "cgs_image_bytes", "cgs_binning_bytes",
         "cgs_bucket_capacity_limit", "cgs_prof_enable", "cgs_prof_reset", "cgs_prof_collect", "cgs_last_error", "cgs_image_status_offset", "cgs_status_words")


def load(path):
    """A library by path with the signatures of the entries this probe calls (L.load() binds every declared entry, which
    an older build does not export)."""
    if path is None:
        return L.load()
    lib = C.CDLL(path)
    for n in NAMES:
        if hasattr(lib, n):
            fn = getattr(lib, n)
            fn.restype, fn.argtypes = L.SIGNATURES[n]
    return lib


def sphere(n_lat=48, n_lon=96, r=0.4, c=(0.5, 0.5, 0.5)):
    th = np.linspace(0.0, math.pi, n_lat + 1)
    ph = np.linspace(0.0, 2.0 * math.pi, n_lon + 1)
    p = lambda i, j: (c[0] + r * math.sin(th[i]) * math.cos(ph[j]), c[1] + r * math.sin(th[i]) * math.sin(ph[j]),
                      c[2] + r * math.cos(th[i]))
    tris = []
    for i in range(n_lat):
        for j in range(n_lon):
            a, b, d, e = p(i, j), p(i + 1, j), p(i + 1, j + 1), p(i, j + 1)
            tris += [(a, b, d), (a, d, e)]
    return np.asarray(tris, np.float32)


def collect(lib):
    cap = 64
    names, ms, n = (C.c_char_p * cap)(), (C.c_double * cap)(), (C.c_int64 * cap)()
    k = lib.cgs_prof_collect(names, ms, n, cap)
    return {names[i].decode(): (ms[i], int(n[i])) for i in range(min(k, cap))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--config", default="cfg3")
    args = ap.parse_args()
    lib = load(args.lib)
    from curve_gaussian_amd.ops.curve_sampling import _bezier_mask, sample_coefficients
    curves, cams = S.make_config(args.config, n_views=3)
    cam = cams[0].to(DEV)
    H, W = cam.image_height, cam.image_width
    B, m = curves["curve_points"].shape[0], 12
    P = B * m
    cap = min(4096, int(lib.cgs_bucket_capacity_limit()))   # (the per-splat kernel's time does not depend on it)
    tiles = ((W + 15) // 16) * ((H + 15) // 16)
    u8 = lambda k: torch.zeros(int(k), dtype=torch.uint8, device=DEV)
    f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=DEV)
    cp, w, op = (curves[k].to(DEV).contiguous() for k in ("curve_points", "width", "opacity"))
    isb, coef = _bezier_mask(curves["is_bezier"].to(DEV), DEV), sample_coefficients(m, DEV)
    norms = torch.empty(384, dtype=torch.float64, device=DEV)
    nbin = int(lib.cgs_binning_bytes(cap * tiles))
    geom, img, binb = u8(lib.cgs_geometry_bytes(P)), u8(lib.cgs_image_bytes(W, H)), u8(nbin)
    color, invd, omap = f32(1, H, W), f32(1, H, W), f32(4, H, W)
    radii = torch.empty(P, dtype=torch.int32, device=DEV)
    bg = torch.zeros(3, device=DEV)
    pt, cf = L.ptr, C.c_float
    tf = (math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5))
    st = L.raw_stream(DEV)
    base = (B, m, pt(cp), pt(w), pt(isb), pt(coef), cf(1e-8), pt(norms), pt(op), None, cf(0.01), None, pt(geom), pt(binb), nbin,
            pt(img), cap, pt(bg), W, H, pt(cam.world_view_transform), pt(cam.full_proj_transform), pt(cam.camera_center),
            tf[0], tf[1], pt(color), pt(invd), pt(omap), pt(radii), None, None, None)
    modes = {"view_fwd": lambda: lib.cgs_view_forward(*base, st)}
    out = {"lib": args.lib or "this build", "config": args.config, "P": P, "image": [W, H], "iters": args.iters, "rounds": []}
    if hasattr(lib, "cgs_view_forward_depth") and args.lib is None:
        from curve_gaussian_amd.ops.train_gate import TrainGate
        gate = TrainGate(cams, occluder=sphere(), device=DEV)
        vg = gate.struct(0)
        modes["view_fwd_depth"] = lambda: lib.cgs_view_forward_depth(*base, C.byref(vg), st)
        out["planes_bytes"] = gate.planes_bytes
    for name, call in modes.items():     # warm up, and how many splats each form draws
        assert call() == 0, lib.cgs_last_error()
        torch.cuda.synchronize()
        out[f"{name}_visible"] = int((radii > 0).sum())
    for _ in range(args.rounds):
        row = {}
        for name, call in modes.items():
            lib.cgs_prof_reset()
            lib.cgs_prof_enable(1)
            for _i in range(args.iters):
                call()
            torch.cuda.synchronize()
            lib.cgs_prof_enable(0)
            ms, n = collect(lib)[name]
            row[name + "_us"] = round(1000.0 * ms / n, 3)
        out["rounds"].append(row)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
