#!/usr/bin/env python
"""Generates the novel-view fixture: two tiny scans under tests/golden/novel_view/ and tests/golden/novel_view/
novel_view.npz, by IMPORTING the reference's edge_extraction/eval_ABC.py and edge_extraction/eval_replica.py and calling
their functions on CPU (runs only where the reference checkout exists; the fixture files travel, the reference does not).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_novel_view_golden.py

What is called: eval_ABC.project_points_to_camera (:66-102) on the cameras of the reference's own
scene.dataset_readers.readCamerasFromTransforms (:251-287, transforms_video.json of abc/data/<scan>), and
eval_ABC.process_scan(render_mv=True) (:140-185) and eval_replica.process_scan (:100-212, the PINHOLE COLMAP scan
replica/<scan>), both with eval_utils.get_pred_points_and_directions and utils.vis_utils.get_fancy_color.  torch is seeded
(SEED) right before each process_scan, so its colour permutation torch.randperm(n) can be reproduced.

How it is imported: through make_model_golden.import_reference, with placeholders for open3d, cv2 and the other absent
packages, poisoned before anything is called.  Substitutions, everything else is the reference's unmodified code:
  1. seaborn is absent: seaborn.color_palette('hls', n) is its hls_palette(n) (hues linspace(0, 1, n + 1)[:-1] + 0.01
     mod 1, colorsys.hls_to_rgb(h, 0.6, 0.65)), restated here; matplotlib.colors (the colour map) is the real one.
  2. matplotlib.pyplot is a recording placeholder: figure / xlim / ylim / axis / close do nothing, scatter(x, y, c=...)
     and savefig(name) are recorded per figure.
  3. eval_replica.create_video_from_images (ffmpeg, out of scope) records its arguments and does nothing.

Planted cases (replica scan, camera 0: identity rotation, zero translation, PINHOLE fx = fy = 64, (cx, cy) = (32, 24),
64x48; points at depth 0.25, so u = 256 X + 32 and v = 256 Y + 24 are exact in float32 and float64): lines of length
0.001220703125 (0.3125 px), which the 0.0005 sampling turns into exactly their two end points, at u = 0, u = W - 2^-10,
u = W, v = 0, v = H - 2^-10, v = H; a point at depth 0 (its partner on the optical axis); a pair at depth -0.25 whose
mirrored projection lands inside the image; lines along viewing rays (every sample in one pixel, > 100 points).  Camera 1
looks away (every point culled), cameras 2-4 are random.  The ABC scan has random look-at cameras in the OpenGL
convention of transforms_video.json, one frame with an edge map of another size, and random points and edges."""
import colorsys
import json
import math
import os
import shutil
import sys
import types

import numpy as np
import torch
from PIL import Image

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.append(os.path.dirname(os.path.dirname(HERE)))   # the project (colmap_io writes the COLMAP scan)
from make_model_golden import _ARMED, import_reference  # noqa: E402

OUT = os.path.join(HERE, "novel_view")
SEED = 20261016
ABC_SCAN, REP_SCAN = "00000001", "room0"
W, H, FX, CX, CY, Z0 = 64, 48, 64.0, 32.0, 24.0, 0.25
STEP = 0.3125 / 256          # 0.3125 px at depth 0.25: a line of this length samples to its two end points

RECORD = {"figures": [], "videos": []}


def _seaborn():
    m = types.ModuleType("seaborn")

    def hls_palette(n_colors=6, h=.01, l=.6, s=.65):                         # substitution 1
        hues = np.linspace(0, 1, int(n_colors) + 1)[:-1]
        hues += h
        hues %= 1
        hues -= hues.astype(int)
        return [colorsys.hls_to_rgb(h_i, l, s) for h_i in hues]

    def color_palette(name, n):
        assert name == "hls"
        return hls_palette(n)

    m.color_palette = color_palette
    return m


def _pyplot():
    m = types.ModuleType("matplotlib.pyplot")                                 # substitution 2

    def figure(*a, **k):
        RECORD["figures"].append({})

    def scatter(x, y, c=None, s=None, alpha=None):
        RECORD["figures"][-1]["scatter"] = (np.array(x), np.array(y), np.array(c), s, alpha)

    def savefig(name, **k):
        RECORD["figures"][-1]["savefig"] = str(name)

    m.figure, m.scatter, m.savefig = figure, scatter, savefig
    m.xlim = m.ylim = m.axis = m.close = lambda *a, **k: None
    return m


def _xyz(u, v, z=Z0):
    return [(u - CX) * z / FX, (v - CY) * z / FX, z]


def _planted_lines():
    L = []
    for u, v in ((0.0, 10.0), (W - 2.0 ** -10, 12.0), (float(W), 14.0), (20.0, 0.0), (22.0, H - 2.0 ** -10),
                 (24.0, float(H)), (40.5, 30.25)):
        a = _xyz(u, v)
        b = list(a)
        b[0 if v in (0.0, 10.0, 12.0, 14.0, 30.25) else 1] += STEP * (-1 if u >= W - 1 or v >= H - 1 else 1)
        L.append([a, b])
    L.append([[0.0, 0.0, 0.0], [0.0, 0.0, STEP]])                            # depth 0, partner at (cx, cy)
    L.append([_xyz(10.0, 20.0, -Z0), [x + STEP * (i == 0) for i, x in enumerate(_xyz(10.0, 20.0, -Z0))]])
    for u, v in ((CX, CY), (50.5, 8.5)):                                       # every sample in one pixel
        L.append([[w * 0.5 for w in _xyz(u, v)], [w * 1.5 for w in _xyz(u, v)]])
    L = np.array(L, np.float64)
    assert np.array_equal(L.astype(np.float32).astype(np.float64), L)
    return L


def _write_replica(root, rng):
    from curve_gaussian_amd.scene import colmap_io as CIO
    scan = os.path.join(root, REP_SCAN)
    os.makedirs(os.path.join(scan, "sparse", "0"))
    cams = {1: CIO.ColmapCamera(1, "PINHOLE", W, H, np.array([FX, FX, CX, CY])),
            2: CIO.ColmapCamera(2, "PINHOLE", 80, 60, np.array([71.5, 69.25, 40.5, 29.75]))}
    qt = [((1.0, 0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 1), ((0.0, 0.0, 1.0, 0.0), (0.0, 0.0, -10.0), 1)]
    for k in range(3):
        q = rng.normal(size=4) * [0.1, 0.15, 0.15, 0.15] + [1, 0, 0, 0]
        qt.append((tuple(q / np.linalg.norm(q)), tuple(rng.uniform(-0.05, 0.05, 3)), 1 + (k == 1)))
    imgs = {}
    for i, (q, t, cid) in enumerate(qt):
        imgs[i + 1] = CIO.ColmapImage(i + 1, np.array(q), np.array(t), cid, f"frame_{i:03d}.jpg" if i != 3 else
                                      f"frame_{i:03d}.png", np.zeros((0, 2)), np.zeros(0, np.int64))
    CIO.write_cameras_binary(os.path.join(scan, "sparse", "0", "cameras.bin"), cams)
    CIO.write_images_binary(os.path.join(scan, "sparse", "0", "images.bin"), imgs)


def _look_at_c2w(eye, target):
    """OpenGL / Blender camera-to-world (x right, y up, z back), as in transforms_*.json."""
    z = eye - target
    z /= np.linalg.norm(z)
    x = np.cross([0.0, 0.0, 1.0], z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, y, z, eye
    return m


def _write_abc(root, rng):
    scan = os.path.join(root, ABC_SCAN)
    os.makedirs(os.path.join(scan, "edge_DexiNed"))
    frames = []
    for f in range(4):
        ang = 2 * math.pi * f / 4 + rng.uniform(-0.2, 0.2)
        eye = np.array([0.5 + 1.6 * math.cos(ang), 0.5 + 1.6 * math.sin(ang), 0.5 + rng.uniform(0.2, 0.9)])
        frames.append({"file_path": f"./train/r_{f}", "transform_matrix": _look_at_c2w(eye, np.full(3, 0.5)).tolist()})
        size = (72, 56) if f == 2 else (W, H)
        Image.fromarray(np.zeros(size[::-1], np.uint8), mode="L").save(os.path.join(scan, "edge_DexiNed", f"r_{f}.png"))
    with open(os.path.join(scan, "transforms_video.json"), "w") as fh:
        json.dump({"camera_angle_x": 0.6911112070083618, "frames": frames}, fh)


def _random_edges(rng, nc, nl, lo, hi):
    c = rng.uniform(lo, hi, (nc, 1, 3)) + np.cumsum(rng.normal(0, 0.04, (nc, 4, 3)), 1)
    ln = rng.uniform(lo, hi, (nl, 2, 3))
    return c, ln


def _edges_json(path, curves, lines):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump({"curves_ctl_pts": np.asarray(curves).reshape(-1, 12).tolist(),
                   "lines_end_pts": np.asarray(lines).reshape(-1, 6).tolist()}, fh)


def _figures():
    out, RECORD["figures"] = RECORD["figures"], []
    return out


def main():
    sys.modules["seaborn"] = _seaborn()
    sys.modules["matplotlib.pyplot"] = _pyplot()
    EA = import_reference("edge_extraction.eval_ABC")
    ER = import_reference("edge_extraction.eval_replica")
    DR = import_reference("scene.dataset_readers")
    CL = import_reference("scene.colmap_loader")
    ER.create_video_from_images = lambda *a, **k: RECORD["videos"].append(a)  # substitution 3
    _ARMED[0] = True
    rng = np.random.default_rng(SEED)
    if os.path.exists(OUT):
        shutil.rmtree(OUT)
    g = {}

    # ---------------------------------------------------------------------------------------------- ABC
    data = os.path.join(OUT, "abc", "data")
    _write_abc(data, rng)
    cams = DR.readCamerasFromTransforms(os.path.join(data, ABC_SCAN), "transforms_video.json")
    for k in ("R", "T", "FovX", "FovY", "width", "height"):
        g[f"abc_{k}"] = np.array([getattr(c, k) for c in cams])
    # eval_ABC.py:79-84, the intrinsics project_points_to_camera forms from a CameraInfo
    g["abc_fx"] = np.array([c.width / (2 * np.tan(c.FovX / 2)) for c in cams])
    g["abc_fy"] = np.array([c.height / (2 * np.tan(c.FovY / 2)) for c in cams])
    g["abc_cx"] = np.array([c.width / 2 for c in cams])
    g["abc_cy"] = np.array([c.height / 2 for c in cams])
    g["abc_names"] = np.array([c.image_name for c in cams])
    pts = np.concatenate([rng.uniform(-0.3, 1.3, (3000, 3)), rng.uniform(0.3, 0.7, (500, 3))]).astype(np.float32)
    cols = rng.uniform(0, 1, (len(pts), 3)).astype(np.float32)
    g["abc_points"], g["abc_colors"] = pts, cols
    for v, c in enumerate(cams):
        uv, pc = EA.project_points_to_camera(pts, cols, c)
        g[f"abc_uv_{v}"], g[f"abc_c_{v}"] = uv.reshape(-1, 2), pc.reshape(-1, 3)
    base = os.path.join(OUT, "abc", "pred")
    curves, lines = _random_edges(rng, 5, 4, 0.2, 0.8)
    _edges_json(os.path.join(base, ABC_SCAN, "parametric_edges.json"), curves, lines)
    torch.manual_seed(SEED)
    EA.process_scan(ABC_SCAN, base, os.path.dirname(data), {}, {}, True)
    figs = _figures()
    g["abc_saved"] = np.array([os.path.relpath(f["savefig"], base) for f in figs if "savefig" in f])
    for v, f in enumerate(figs):
        if "scatter" in f:
            x, y, c, s, a = f["scatter"]
            g[f"abc_mv_uv_{v}"], g[f"abc_mv_c_{v}"] = np.stack([x, y], 1), c
            assert s == 1 and a == 0.5

    # ---------------------------------------------------------------------------------------------- Replica
    rdata = os.path.join(OUT, "replica", "data")
    _write_replica(rdata, rng)
    planted = _planted_lines()
    curves, lines = _random_edges(rng, 3, 3, -0.1, 0.1)
    curves[:, :, 2] += 0.3
    lines[:, :, 2] += 0.3
    lines = np.concatenate([planted, lines])
    base = os.path.join(OUT, "replica", "pred")
    _edges_json(os.path.join(base, REP_SCAN, "parametric_edges.json"), curves, lines)
    extr = CL.read_extrinsics_binary(os.path.join(rdata, REP_SCAN, "sparse", "0", "images.bin"))
    intr = CL.read_intrinsics_binary(os.path.join(rdata, REP_SCAN, "sparse", "0", "cameras.bin"))
    g["rep_R"] = np.array([CL.qvec2rotmat(im.qvec) for im in extr.values()])
    g["rep_T"] = np.array([im.tvec for im in extr.values()])
    g["rep_intr"] = np.array([intr[im.camera_id].params[:4] for im in extr.values()])
    g["rep_W"] = np.array([intr[im.camera_id].width for im in extr.values()])
    g["rep_H"] = np.array([intr[im.camera_id].height for im in extr.values()])
    g["rep_names"] = np.array([im.name for im in extr.values()])
    g["rep_planted"] = planted
    torch.manual_seed(SEED)
    ER.process_scan(REP_SCAN, base, "exp", rdata)
    figs = _figures()
    assert len(figs) == len(extr)
    g["rep_saved"] = np.array([os.path.relpath(f["savefig"], base) for f in figs if "savefig" in f])
    for v, f in enumerate(figs):
        if "scatter" in f:
            x, y, c, s, a = f["scatter"]
            g[f"rep_uv_{v}"], g[f"rep_c_{v}"] = np.stack([x, y], 1), c
            assert s == 1 and a == 0.5
    assert "rep_uv_1" not in g, "camera 1 must cull every point"
    assert len(RECORD["videos"]) == 1
    g["seed"] = np.array(SEED)
    for d in ("abc", "replica"):   # the reference's makedirs left empty output directories behind
        for root, dirs, files in os.walk(os.path.join(OUT, d, "pred"), topdown=False):
            if not dirs and not files:
                os.rmdir(root)
    np.savez_compressed(os.path.join(OUT, "novel_view.npz"), **g)
    print("saved:", sorted(g["abc_saved"]), sorted(g["rep_saved"]))
    print({k: v.shape for k, v in g.items() if k.startswith(("rep_uv", "abc_uv", "abc_mv_uv"))})


if __name__ == "__main__":
    main()
