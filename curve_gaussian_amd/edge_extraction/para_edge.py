"""The extraction step's edge-map visibility check (edge_extraction/extract_para_edge.py:21-57, 145-257 of the
reference): which fitted curves and lines the 2D edge detector actually saw.

``get_edge_maps`` reads a scan's edge maps on the host as raw 8-bit values; ``compute_visibility`` counts, in the HIP
kernel ``cgs_edge_visibility``, the frames in which every edge is seen and applies the reference's thresholds;
``get_parametric_edge`` is the reference's entry point of the same name, with its signature and return value."""
import json
import math
import os

import numpy as np
import torch

from .. import _lib as L
from ..scene.dataset_io import DETECTOR_DIRS, sample_edge_points

# The reference's hard-coded thresholds (extract_para_edge.py:189-192, 212-214)
EDGE_VISIBILITY_THRESHOLD = 0.1      # mean of the edge-map values at the projected points
EDGE_MAX_THRESHOLD = 0.5             # max of the same values
EDGE_VISIBILITY_FRAMES_RATIO = 0.05  # an edge is kept if seen in more than ceil(0.05 * frames) frames

# Image modes converted to 8-bit grayscale when a map is not already one (see get_edge_maps)
_CONVERTIBLE_MODES = ("1", "P", "LA", "RGB", "RGBA")


def edge_visibility_frames(n_frames):
    """extract_para_edge.py:215-217: the number of frames an edge must be seen in MORE than."""
    return math.ceil(EDGE_VISIBILITY_FRAMES_RATIO * n_frames)


def edge_map_paths(scan_dir, detector):
    """The edge-map file of every frame of ``meta_data.json``, by the extraction step's rules (get_edge_maps :27-45):
    DexiNed maps are ``edge_DexiNed/<rgb_path>``, PidiNet maps ``edge_PidiNet/<rgb_path[:-4]>.png`` (training's
    read_emap takes rgb_path verbatim for both).  Returns (meta, paths); an unknown detector raises ValueError."""
    with open(os.path.join(scan_dir, "meta_data.json"), encoding="UTF-8") as f:
        meta = json.load(f)
    if detector == "DexiNed":
        paths = [os.path.join(scan_dir, DETECTOR_DIRS[detector], fr["rgb_path"]) for fr in meta["frames"]]
    elif detector == "PidiNet":
        paths = [os.path.join(scan_dir, DETECTOR_DIRS[detector], fr["rgb_path"][:-4] + ".png") for fr in meta["frames"]]
    else:
        raise ValueError(f"Unknown detector: {detector}")
    return meta, paths


def read_edge_map_u8(path):
    """One edge map as uint8 [H,W]: an 8-bit grayscale (mode "L") PNG gives its stored values, as cv2.imread(path, 0)
    does.  Other images (the reference decodes them with OpenCV, which is not available here) are converted with PIL's
    ``convert("L")``, L = (299 R + 587 G + 114 B) / 1000 rounded, alpha and palette resolved first: UNPINNED against
    the reference.  Modes with more than 8 bits per channel raise ValueError."""
    from PIL import Image
    if not os.path.isfile(path):
        raise FileNotFoundError(f"edge map not found: {path}")
    with Image.open(path) as img:
        if img.mode != "L":
            if img.mode not in _CONVERTIBLE_MODES:
                raise ValueError(f"edge map {path}: unsupported image mode {img.mode!r}")
            img = img.convert("L")
        return np.array(img, dtype=np.uint8)


def get_edge_maps(scan_dir, detector):
    """extract_para_edge.py:21-57 without the float conversion: (maps uint8 [F,H,W], intrinsics [F,..], camtoworld
    [F,4,4], h, w), with h, w the meta's ``height`` / ``width``.  The kernel turns a gathered byte u into the
    reference's value, 1 - u/255.0 (DexiNed) or u/255.0 (PidiNet).  Raises ValueError for an unknown detector, a scan
    without frames and a map whose size is not (h, w); FileNotFoundError, naming the path, for a missing map."""
    meta, paths = edge_map_paths(scan_dir, detector)
    h, w = int(meta["height"]), int(meta["width"])
    if not paths:
        raise ValueError(f"scan {scan_dir} has no frames in meta_data.json")
    maps = np.empty((len(paths), h, w), dtype=np.uint8)
    for i, p in enumerate(paths):
        m = read_edge_map_u8(p)
        if m.shape != (h, w):
            raise ValueError(f"edge map {p} is {m.shape[0]}x{m.shape[1]}, meta_data.json says {h}x{w}")
        maps[i] = m
    intrinsics = np.stack([np.array(fr["intrinsics"]) for fr in meta["frames"]])
    camtoworld = np.stack([np.array(fr["camtoworld"])[:4, :4] for fr in meta["frames"]])
    return maps, intrinsics, camtoworld, h, w


def _host64(x):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=np.float64)


def edge_visibility_counts(curves, lines, maps_u8, intrinsics, camtoworld, detector):
    """Per edge (curves first, then lines), the number of frames in which it is seen (``cgs_edge_visibility``):
    int32 [Nc + Nl] on the maps' device.  curves [Nc,4,3] (or [Nc,12]), lines [Nl,2,3] (or [Nl,6]) and maps_u8 uint8
    [F,H,W] are GPU tensors on one device; intrinsics [F,>=3,>=3] and camtoworld [F,4,4] are host arrays (or tensors):
    K = intrinsics[:3,:3] and w2c = np.linalg.inv(camtoworld) are formed on the host, frame by frame, as the
    reference does (:173-176)."""
    if detector == "DexiNed":
        invert = 1
    elif detector == "PidiNet":
        invert = 0
    else:
        raise ValueError(f"Unknown detector: {detector}")
    for t, name in ((curves, "curves"), (lines, "lines"), (maps_u8, "maps_u8")):
        L.require_gpu_tensor(t, name)
    dev = maps_u8.device
    for t, name in ((curves, "curves"), (lines, "lines"), (intrinsics, "intrinsics"), (camtoworld, "camtoworld")):
        if isinstance(t, torch.Tensor) and t.device != dev:
            raise L.CurveGSError(f"{name} is on {t.device}, maps_u8 on {dev}: all tensors must be on one device")
    if maps_u8.dtype != torch.uint8 or maps_u8.dim() != 3:
        raise L.CurveGSError(f"maps_u8 must be uint8 [F,H,W] (got {maps_u8.dtype} {tuple(maps_u8.shape)})")
    F, H, W = (int(s) for s in maps_u8.shape)
    K = _host64(intrinsics)
    c2w = _host64(camtoworld)
    if K.shape[0] != F or c2w.shape[0] != F or K.shape[1] < 3 or K.shape[2] < 3 or c2w.shape[1:] != (4, 4):
        raise L.CurveGSError(f"intrinsics / camtoworld must be [F,3+,3+] / [F,4,4] with F = {F} "
                             f"(got {K.shape}, {c2w.shape})")
    K = np.ascontiguousarray(K[:, :3, :3])
    w2c = np.stack([np.linalg.inv(c2w[f])[:3, :4] for f in range(F)]) if F else np.zeros((0, 3, 4))
    lib = L.load()
    with L.device_guard(dev):
        c = curves.to(torch.float64).reshape(-1, 12).contiguous()
        ln = lines.to(torch.float64).reshape(-1, 6).contiguous()
        maps = maps_u8.contiguous()
        nc, nl = c.shape[0], ln.shape[0]
        counts = torch.empty((nc + nl,), dtype=torch.int32, device=dev)
        if nc + nl > 0:
            Kd = torch.from_numpy(K).to(dev)
            Md = torch.from_numpy(np.ascontiguousarray(w2c)).to(dev)
            rc = lib.cgs_edge_visibility(nc, L.ptr(c), nl, L.ptr(ln), F, L.ptr(Kd), L.ptr(Md), H, W, L.ptr(maps),
                                         invert, L.ptr(counts), L.raw_stream(dev))
            L.check(rc, "cgs_edge_visibility")
    return counts


def compute_visibility(curves, lines, maps_u8, intrinsics, camtoworld, detector):
    """extract_para_edge.py:145-197 on the GPU, with the thresholds of get_parametric_edge: an edge is visible in a
    frame if the edge-map values at its projected control / end points have mean > 0.1 and max > 0.5, and it is kept
    if it is visible in more than ceil(0.05 * F) frames.  Arguments as edge_visibility_counts.  Returns
    (curve_mask bool [Nc], line_mask bool [Nl]) on the maps' device."""
    counts = edge_visibility_counts(curves, lines, maps_u8, intrinsics, camtoworld, detector)
    keep = counts > edge_visibility_frames(int(maps_u8.shape[0]))
    nc = int(curves.reshape(-1, 12).shape[0])
    return keep[:nc], keep[nc:]


def _edge_arrays(edge_dict):
    curves = np.array(edge_dict["curves_ctl_pts"]).reshape(-1, 12).reshape(-1, 4, 3)
    lines = np.array(edge_dict["lines_end_pts"]).reshape(-1, 6)
    return curves, lines


def get_parametric_edge(visible_checking, merged_edge_dict, meta_data_dir=None, detector=None):
    """extract_para_edge.py:200-257: (pred_points float32 [N,3], return_edge_dict) with return_edge_dict =
    {"curves_ctl_pts": [n,4,3], "lines_end_pts": [n,6]} and the points sampled every 5 mm along its edges.  With
    visible_checking=True only the edges that compute_visibility keeps are returned (maps of `detector` read from
    `meta_data_dir`, the check on the current GPU) and the reference's "before / after visible checking" counts are
    printed; meta_data_dir is then required (the reference's train.py never passes it)."""
    curves, lines = _edge_arrays(merged_edge_dict)
    if visible_checking:
        if meta_data_dir is None:
            raise ValueError("get_parametric_edge(visible_checking=True) needs meta_data_dir, the scan directory "
                             "holding meta_data.json and the edge maps")
        maps, intrinsics, camtoworld, _, _ = get_edge_maps(meta_data_dir, detector)
        dev = torch.device("cuda", torch.cuda.current_device())
        cm, lm = compute_visibility(torch.from_numpy(curves).to(dev), torch.from_numpy(lines).to(dev),
                                    torch.from_numpy(maps).to(dev), intrinsics, camtoworld, detector)
        cm, lm = cm.cpu().numpy(), lm.cpu().numpy()
        print("before visible checking: ", len(curves) + len(lines), "after visible checking: ",
              int(cm.sum()) + int(lm.sum()))
        curves, lines = curves[cm], lines[lm]
    return sample_edge_points(curves, lines), {"curves_ctl_pts": curves.tolist(), "lines_end_pts": lines.tolist()}
