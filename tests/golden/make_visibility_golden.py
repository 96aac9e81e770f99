#!/usr/bin/env python
"""Generates the edge-map visibility fixture: a small synthetic scan under tests/golden/visibility/ (meta_data.json,
edge_DexiNed/ and edge_PidiNet/ single-channel 8-bit PNGs) and tests/golden/visibility/visibility.npz, by IMPORTING the
reference's edge_extraction/extract_para_edge.py and calling its functions on CPU (runs only where the reference
checkout exists; the fixture files travel, the reference does not).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_visibility_golden.py

What is called: get_edge_maps :21-57, compute_visibility :145-197 (with project2D / project2D_single :132-142) and
get_parametric_edge(True, ...) :200-249 (with process_geometry_data :60-129 and extract_uitl.bezier_curve_length).

How it is imported: through make_model_golden.import_reference, with placeholders for cv2, point_cloud_utils, open3d
and trimesh, poisoned before anything is called.  Exactly one substitution, everything else is the reference's
unmodified code: cv2.imread(path, 0) is np.array(Image.open(path)), asserted to be an 8-bit mode "L" PNG, for which both
readers return the file's stored values.

Per-edge counts come from the reference's own function: the count of edge e is the number of k in 0..F-1 for which
compute_visibility(..., edge_visibility_frames=k)[e] is True (its result is sum(cells) > k).

Planted cases (identity-rotation cameras, fx = fy = 256, principal point (48, 36), points at depth 0.25 or -0.25, so
that u = 1024 X + 48 and v = 1024 Y + 36 are exact): projections on k + 0.5, -0.5, w - 0.5 and h - 0.5 with the neighbouring
pixel bright whenever the right one is dark; mean ties over 2 and 4 points for both detectors; maxima at u8 127 and 128;
points behind the camera landing in the image; points at depth 0 (inf and 0/0); edges partly and fully out of bounds;
edges seen in exactly ceil(0.05 F) = 2 and 3 frames.  Six more frames have rotated cameras, and random edges and
random bright strokes fill the rest."""
import json
import math
import os
import shutil
import sys

import numpy as np
from PIL import Image

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_model_golden import _ARMED, _placeholder, import_reference  # noqa: E402

OUT = os.path.join(HERE, "visibility")
H, W = 72, 96
F_PLANTED = 18             # frames 0..17: identity rotation, the planted cases' pixels written explicitly
F = 24                     # frames 18..23: rotated cameras
FX, CX, CY = 256, 48, 36
Z0 = 0.25                  # depth of the planted points: u = 1024 X + 48, v = 1024 Y + 36
BRIGHT = (200, 30)         # (PidiNet u8, DexiNed u8): value 0.784 / 0.882
DARK = (0, 255)            # value 0 for both detectors


def _cv2():
    m = _placeholder("cv2")

    def imread(path, flag):                                                  # the one substitution
        assert flag == 0
        with Image.open(path) as img:
            assert img.format == "PNG" and img.mode == "L", (path, img.format, img.mode)
            return np.array(img)

    m.imread = imread
    return m


def _pt(u, v, z=Z0):
    """The 3D point that projects to (u, v) in every planted frame: u = FX X / z + CX, v = FX Y / z + CY."""
    return [(u - CX) * z / FX, (v - CY) * z / FX, z]


# name, kind, points [(u, v[, z]) or ("xyz", X, Y, Z)], pixel writes [((u, v), on (P, D), off (P, D))], frames on
CASES = []


def case(name, kind, pts, writes, on):
    P = [list(p[1:]) if p[0] == "xyz" else _pt(*p) for p in pts]
    assert len(P) == (4 if kind == "curve" else 2)
    CASES.append(dict(name=name, kind=kind, pts=np.array(P, np.float64), writes=writes, on=set(on)))


def _planted():
    B, D = BRIGHT, DARK
    # rounding half to even, and the image borders
    case("round_10.5", "line", [(10.5, 2), (10.5, 2)], [((10, 2), B, D), ((11, 2), D, B)], {0, 1, 2})
    case("round_11.5", "line", [(11.5, 4), (11.5, 4)], [((12, 4), B, D), ((11, 4), D, B)], {0, 1, 2, 3})
    case("u_-0.5", "line", [(-0.5, 6), (-0.5, 6)], [((0, 6), B, D)], {1, 2, 3})
    case("u_w-0.5", "line", [(W - 0.5, 8), (W - 0.5, 8)], [((W - 1, 8), B, B)], set())
    case("v_-0.5", "line", [(30, -0.5), (30, -0.5)], [((30, 0), B, D)], {4, 5, 6})
    case("v_h-0.5", "line", [(32, H - 0.5), (32, H - 0.5)], [((32, H - 1), B, B)], set())
    case("round_0.5", "line", [(0.5, 10), (0.5, 10)], [((0, 10), B, D), ((1, 10), D, B)], {2, 3, 4})
    case("round_curve", "curve", [(14.5, 12), (15.5, 12), (16.5, 12), (17.5, 12)],
         [((14, 12), B, D), ((16, 12), B, D), ((18, 12), B, D), ((15, 12), D, B), ((17, 12), D, B)], {5, 6, 7})
    # mean ties (sum 0.2 over 2 points, 0.4 over 4): PidiNet 25 + 26, DexiNed 229 + 230
    case("tie_2", "line", [(40, 14), (41, 14)], [((40, 14), (25, 229), D), ((41, 14), (26, 230), D)], range(6))
    case("tie_4", "curve", [(40, 16), (41, 16), (42, 16), (43, 16)],
         [((40, 16), (25, 229), D), ((41, 16), (25, 229), D), ((42, 16), (26, 230), D), ((43, 16), (26, 230), D)],
         range(6))
    # maxima at 127 / 128: PidiNet 127/255 < 0.5 < 128/255, DexiNed the other way round
    case("max_127", "line", [(50, 18), (51, 18)], [((50, 18), (127, 127), D), ((51, 18), D, D)], {0, 1, 2})
    case("max_128", "line", [(50, 20), (51, 20)], [((50, 20), (128, 128), D), ((51, 20), D, D)], {0, 1, 2})
    case("mean_no_max", "line", [(80, 38), (81, 38)], [((80, 38), (120, 135), D), ((81, 38), (120, 135), D)],
         {0, 1, 2})
    # behind the camera (z = -2: mirrored, in bounds) and at depth 0
    case("z_neg", "line", [(60, 22, -Z0), (61, 22, -Z0)], [((60, 22), B, D), ((61, 22), B, D)], {3, 4, 5})
    case("z_zero", "line", [("xyz", 0.125, 0.0, 0.0), ("xyz", 0.0, 0.0, 0.0)], [], set())
    case("z_zero_mixed", "curve", [("xyz", 0.0625, 0.03125, 0.0), (62, 24), (63, 24), ("xyz", 0.0, 0.0, 0.0)],
         [((62, 24), B, D), ((63, 24), B, D)], {0, 1, 2, 3})
    # out of bounds
    case("part_oob", "curve", [(-10, 26), (200, 26), (64, 26), (65, 26)], [((64, 26), B, D), ((65, 26), B, D)],
         {0, 1, 2, 3})
    case("full_oob_line", "line", [(150, 30), (-20, -5)], [], set())
    case("full_oob_curve", "curve", [(100, 10), (10, 100), (-3, -3), (W, H)], [], set())
    # the frame threshold: ceil(0.05 * 24) = 2, kept if seen in MORE frames
    case("frames_2", "line", [(70, 32), (71, 32)], [((70, 32), B, D), ((71, 32), B, D)], {6, 7})
    case("frames_3", "line", [(70, 34), (71, 34)], [((70, 34), B, D), ((71, 34), B, D)], {6, 7, 8})
    case("frames_3_curve", "curve", [(72, 36), (73, 36), (74, 36), (75, 36)],
         [((72, 36), B, D), ((73, 36), D, D), ((74, 36), B, D), ((75, 36), D, D)], {9, 10, 11})


def _cameras(rng):
    K, c2w = [], []
    for f in range(F):
        k = np.array([[FX, 0, CX, 0], [0, FX, CY, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float64)
        m = np.eye(4)
        if f >= F_PLANTED:
            a, b = rng.uniform(-0.35, 0.35, 2)
            Ry = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
            Rx = np.array([[1, 0, 0], [0, math.cos(b), -math.sin(b)], [0, math.sin(b), math.cos(b)]])
            m[:3, :3] = Ry @ Rx
            m[:3, 3] = rng.uniform(-0.05, 0.05, 3)
            k[0, 0], k[1, 1] = rng.uniform(224, 320, 2)
            k[0, 2], k[1, 2] = CX + rng.uniform(-2, 2), CY + rng.uniform(-2, 2)
        K.append(k)
        c2w.append(m)
    return np.array(K), np.array(c2w)


def _maps(rng, K, c2w):
    """uint8 maps [F,H,W] for both detectors: faint noise, random bright strokes, then the planted pixels."""
    P = rng.integers(0, 8, (F, H, W)).astype(np.uint8)
    D = (255 - rng.integers(0, 8, (F, H, W))).astype(np.uint8)
    for f in range(F):
        for _ in range(10):
            (u0, v0), (u1, v1) = rng.uniform([0, 0], [W, H], (2, 2))
            t = np.linspace(0, 1, 80)
            uu = np.clip(np.round(u0 + t * (u1 - u0)).astype(int), 0, W - 1)
            vv = np.clip(np.round(v0 + t * (v1 - v0)).astype(int), 0, H - 1)
            P[f, vv, uu] = rng.integers(100, 256)
            D[f, vv, uu] = rng.integers(0, 156)
    for c in CASES:
        for f in range(F_PLANTED):
            for (u, v), on, off in c["writes"]:
                P[f, v, u], D[f, v, u] = on if f in c["on"] else off
    # the rotated frames never show a planted edge: the pixels around its projected points are dark
    for f in range(F_PLANTED, F):
        w2c = np.linalg.inv(c2w[f])
        for c in CASES:
            x = K[f, :3, :3] @ (w2c[:3, :3] @ c["pts"].T + w2c[:3, 3:])
            with np.errstate(divide="ignore", invalid="ignore"):
                uv = (x[:2] / x[2:]).T
            for u, v in uv[np.isfinite(uv).all(1)]:
                for uu in (math.floor(u), math.ceil(u)):
                    for vv in (math.floor(v), math.ceil(v)):
                        if 0 <= uu < W and 0 <= vv < H:
                            P[f, vv, uu], D[f, vv, uu] = DARK
    return P, D


def _write_scan(K, c2w, P, D):
    if os.path.exists(OUT):
        shutil.rmtree(OUT)
    os.makedirs(os.path.join(OUT, "edge_DexiNed"))
    os.makedirs(os.path.join(OUT, "edge_PidiNet"))
    frames = []
    for f in range(F):
        rgb = f"{f:02d}_colors.jpg"     # DexiNed maps are read at rgb_path verbatim, PidiNet maps at rgb_path[:-4].png
        Image.fromarray(D[f], mode="L").save(os.path.join(OUT, "edge_DexiNed", rgb), format="PNG")
        Image.fromarray(P[f], mode="L").save(os.path.join(OUT, "edge_PidiNet", rgb[:-4] + ".png"), format="PNG")
        frames.append({"rgb_path": rgb, "camtoworld": c2w[f].tolist(), "intrinsics": K[f].tolist()})
    with open(os.path.join(OUT, "meta_data.json"), "w") as fh:
        json.dump({"height": H, "width": W, "frames": frames}, fh)


def main():
    sys.modules["cv2"] = _cv2()
    EP = import_reference("edge_extraction.extract_para_edge")
    _ARMED[0] = True
    rng = np.random.default_rng(20261015)
    _planted()
    K, c2w = _cameras(rng)
    P, D = _maps(rng, K, c2w)
    _write_scan(K, c2w, P, D)

    planted_curves = np.array([c["pts"] for c in CASES if c["kind"] == "curve"])
    planted_lines = np.array([c["pts"].reshape(6) for c in CASES if c["kind"] == "line"])
    # random edges in front of (and a few behind) the cameras
    rc = np.concatenate([rng.uniform([-0.07, -0.05, 0.25], [0.07, 0.05, 0.4], (36, 4, 3)),
                         rng.uniform([-0.05, -0.04, -0.4], [0.05, 0.04, -0.25], (4, 4, 3))])
    rl = np.concatenate([rng.uniform([-0.07, -0.05, 0.25], [0.07, 0.05, 0.4], (26, 2, 3)),
                         rng.uniform([-0.05, -0.04, -0.4], [0.05, 0.04, -0.25], (4, 2, 3))]).reshape(-1, 6)
    curves = np.concatenate([planted_curves, rc]).reshape(-1, 12)
    lines = np.concatenate([planted_lines, rl])
    edge_dict = {"lines_end_pts": lines.tolist(), "curves_ctl_pts": curves.tolist()}
    out = {"curves": curves.reshape(-1, 4, 3), "lines": lines.reshape(-1, 2, 3),
           "planted_curve_names": np.array([c["name"] for c in CASES if c["kind"] == "curve"]),
           "planted_line_names": np.array([c["name"] for c in CASES if c["kind"] == "line"])}

    for det in ("DexiNed", "PidiNet"):
        edges, intr, cw, h, w = EP.get_edge_maps(OUT, det)
        u8 = np.round((1 - edges[..., 0] if det == "DexiNed" else edges[..., 0]) * 255.0).astype(np.uint8)
        assert np.array_equal(1 - u8 / 255.0 if det == "DexiNed" else u8 / 255.0, edges[..., 0])
        out[f"{det}_u8"] = u8
        _, red = EP.process_geometry_data(edge_dict)
        cps, lps = red["curves_ctl_pts"], red["lines_end_pts"]
        n_edges = len(cps) + len(lps)
        counts = np.zeros(n_edges, np.int64)
        for k in range(F):
            counts += EP.compute_visibility(cps, lps, edges, intr, cw, h, w, 0.1, k).astype(np.int64)
        thr = math.ceil(0.05 * F)
        mask = EP.compute_visibility(cps, lps, edges, intr, cw, h, w, 0.1, thr)
        assert np.array_equal(mask, counts > thr)
        pts, ret = EP.get_parametric_edge(True, edge_dict, OUT, det)
        out[f"{det}_counts"], out[f"{det}_mask"] = counts, mask
        out[f"{det}_curves"] = np.asarray(ret["curves_ctl_pts"], np.float64).reshape(-1, 4, 3)
        out[f"{det}_lines"] = np.asarray(ret["lines_end_pts"], np.float64).reshape(-1, 6)
        out[f"{det}_points"] = pts
        names = [c["name"] for c in CASES if c["kind"] == "curve"] + [None] * len(rc) + \
                [c["name"] for c in CASES if c["kind"] == "line"] + [None] * len(rl)
        by_name = {n: int(counts[i]) for i, n in enumerate(names) if n}
        print(det, "threshold", thr, "kept", int(mask.sum()), "of", n_edges, by_name)
        assert by_name["frames_2"] == 2 and by_name["frames_3"] == 3 and by_name["frames_3_curve"] == 3
        for c in CASES:
            seen = {"DexiNed": {"max_127"}, "PidiNet": {"max_128"}}[det]
            lit = c["on"] if c["name"] in seen or not c["name"].startswith(("tie", "max", "mean")) else set()
            assert by_name[c["name"]] == len(lit), (c["name"], by_name[c["name"]], len(lit))
    np.savez_compressed(os.path.join(OUT, "visibility.npz"), **out)
    print("wrote", os.path.join(OUT, "visibility.npz"))


if __name__ == "__main__":
    main()
