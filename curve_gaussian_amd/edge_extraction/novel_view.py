"""Multi-view projection of the extracted edges (the reference's eval_ABC.py --render_mv, :66-138 and :180-185, and
eval_replica.py process_scan, :100-212): the ``parametric_edges.json`` edges, sampled densely and coloured per edge, are
projected into every camera of a scan and drawn one pixel per point, one image per view.

``project_points`` and ``render_points`` run in the HIP kernels ``cgs_project_points`` / ``cgs_render_points`` (there is
no CPU path: CPU tensors raise).  The camera loaders and the per-edge colours are host-side float64 numpy, computed as
the reference computes them.  Deviations: the output is the camera's pixel grid (a kept point covers pixel
(floor(u), floor(v)), alpha-composited in point order) rather than a matplotlib figure; the colour permutation is seeded;
SIMPLE_PINHOLE cameras are read as (f, f, cx, cy).

The depth gate (opt-in; ``ops.edge_occlusion``): ``project_points_depth`` and ``render_points_depth`` drop a
point that its view's depth plane hides (``cgs_project_points_depth`` / ``cgs_render_points_depth``, the occlusion rule
``nv_hidden`` of the 2D score), ``render_views(depth=)`` takes a scan's ``ChunkDepth``, and the two scan drivers take
``occluder`` / ``depth_dir`` and then write to ``novel_view_visible/`` beside ``novel_view/``: the picture a user looks at is
the one the depth-gated score was computed on.  Hidden means dropped -- nothing is drawn dashed or dimmed.  UNTUNED: only the
drawn solids of scene/solid_scan.py have been checked, no real scan."""
import colorsys
import json
import logging
import os
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path
from typing import NamedTuple

import numpy as np
import torch

from .. import _lib as L
from ..ops import edge_occlusion as EO
from ..ops import edge_score as ES
from ..ops.edge_score import _cameras, cameras_on
from ..ops.view_chunks import camera_arrays, view_chunks
from ..scene import colmap_io
from ..scene.dataset_io import focal2fov, fov2focal
from .abc import pred_points_and_directions

log = logging.getLogger(__name__)

ALPHA = 0.5                        # plt.scatter(..., alpha=0.5)
BACKGROUND = (1.0, 1.0, 1.0)       # matplotlib's white figure
REPLICA_SAMPLE_RESOLUTION = 0.0005  # eval_replica.py:113
WORKSPACE_BUDGET = 1 << 30          # bytes of kernel scratch per render_points call (views are chunked to fit)
OUTPUT_BUDGET = 1 << 30             # bytes of float32 images per driver batch
MAX_WRITERS = 16                    # image-encoding threads
VISIBLE_DIR = "novel_view_visible"  # where the scan drivers write with a depth source (novel_view/ is never touched)


class NovelViewCamera(NamedTuple):
    name: str          # output file name (ABC: the frame's stem; Replica: the COLMAP image name)
    R: np.ndarray      # [3,3] float64 world -> camera rotation, applied as R @ X
    T: np.ndarray      # [3] float64
    fx: float
    fy: float
    cx: float
    cy: float
    width: int
    height: int


# ------------------------------------------------------------------------------------------------ camera loaders
def transforms_video_cameras(scan_dir, detector="DexiNed"):
    """The cameras of ``<scan_dir>/transforms_video.json`` as readCamerasFromTransforms (scene/dataset_readers.py:251-287)
    builds them and project_points_to_camera (eval_ABC.py:66-81) turns them into intrinsics: c2w[:3,1:3] flipped, w2c =
    inv(c2w), fx = W / (2 tan(FovX / 2)), FovY = focal2fov(fov2focal(FovX, W), H), fy = H / (2 tan(FovY / 2)),
    (cx, cy) = (W / 2, H / 2).  W and H are the size of the edge map the reference opens, found by its path rule
    (``<scan_dir>/<file_path>.png`` with 'ABC-NEF/' -> 'ABC-NEF_Edge/data/' and 'train' -> 'edge_<detector>'); a missing
    file raises FileNotFoundError naming the path."""
    from PIL import Image
    path = os.path.abspath(scan_dir)
    with open(os.path.join(path, "transforms_video.json")) as f:
        contents = json.load(f)
    fovx = contents["camera_angle_x"]
    cams = []
    for frame in contents["frames"]:
        cam_name = os.path.join(path, frame["file_path"] + ".png")
        c2w = np.array(frame["transform_matrix"])
        c2w[:3, 1:3] *= -1
        w2c = np.linalg.inv(c2w)
        image_path = os.path.join(path, cam_name)
        edge_path = image_path.replace("ABC-NEF/", "ABC-NEF_Edge/data/").replace("train", "edge_" + detector)
        if not os.path.isfile(edge_path):
            raise FileNotFoundError(f"edge map not found: {edge_path}")
        with Image.open(edge_path) as img:
            W, H = img.size
        fovy = focal2fov(fov2focal(fovx, W), H)
        cams.append(NovelViewCamera(Path(cam_name).stem, np.ascontiguousarray(w2c[:3, :3]), w2c[:3, 3].copy(),
                                    W / (2 * np.tan(fovx / 2)), H / (2 * np.tan(fovy / 2)), W / 2, H / 2, W, H))
    return cams


def colmap_cameras(scan_dir):
    """Every image of ``<scan_dir>/sparse/0/{images,cameras}.bin``, in file order, as eval_replica.py:136-157 reads them:
    R = qvec2rotmat(qvec), T = tvec, PINHOLE (fx, fy, cx, cy) = params[0:4].  SIMPLE_PINHOLE is read as (f, f, cx, cy)
    (the reference would index past its 3 parameters); any other model raises ValueError."""
    sparse = os.path.join(scan_dir, "sparse", "0")
    imgs = colmap_io.read_images_binary(os.path.join(sparse, "images.bin"))
    intr = colmap_io.read_cameras_binary(os.path.join(sparse, "cameras.bin"))
    cams = []
    for _, im in imgs.items():
        c = intr[im.camera_id]
        if c.model == "PINHOLE":
            fx, fy, cx, cy = (float(v) for v in c.params[:4])
        elif c.model == "SIMPLE_PINHOLE":
            fx, cx, cy = (float(v) for v in c.params[:3])
            fy = fx
        else:
            raise ValueError(f"{sparse}: camera {c.id} has model {c.model}; novel views need PINHOLE or SIMPLE_PINHOLE")
        cams.append(NovelViewCamera(im.name, colmap_io.qvec2rotmat(im.qvec), np.asarray(im.tvec, np.float64), fx, fy, cx,
                                    cy, int(c.width), int(c.height)))
    return cams


# ------------------------------------------------------------------------------------------------ per-edge colours
def _hls_palette(n, h=0.01, l=0.6, s=0.65):
    """seaborn.color_palette('hls', n)."""
    hues = np.linspace(0, 1, int(n) + 1)[:-1]
    hues += h
    hues %= 1
    hues -= hues.astype(int)
    return [colorsys.hls_to_rgb(h_i, l, s) for h_i in hues]


def fancy_cmap_lut(N=256):
    """The [N,3] float64 lookup table of utils/vis_utils.get_fancy_cmap: gold, then the 'hls' palette of 100 colours
    rotated by 3, through LinearSegmentedColormap.from_list (N = 256 entries, linear interpolation, gamma 1)."""
    pal = _hls_palette(100)
    colors = np.array([(1.0, 215 / 255, 0.0)] + pal[3:] + pal[:2], np.float64)   # 'gold' = #FFD700
    x = np.linspace(0, 1, len(colors)) * (N - 1)
    xind = (N - 1) * np.linspace(0, 1, N) ** 1.0
    ind = np.searchsorted(x, xind)[1:-1]
    distance = (xind[1:-1] - x[ind - 1]) / (x[ind] - x[ind - 1])
    lut = np.concatenate([colors[:1], distance[:, None] * (colors[ind] - colors[ind - 1]) + colors[ind - 1],
                          colors[-1:]])
    return np.clip(lut, 0.0, 1.0)


def fancy_colors(num):
    """utils/vis_utils.get_fancy_color(num): float32 [num,3], the colour map at linspace(0, 1, num + 1)[1:]."""
    lut = fancy_cmap_lut()
    N = lut.shape[0]
    xa = torch.linspace(0, 1, num + 1)[1:].numpy().copy()
    xa *= N
    xa[xa == N] = N - 1
    return torch.from_numpy(lut[xa.astype(int)]).float()


def edge_point_colors(pred, seed=0):
    """Per-point colours of get_pred_points_and_directions (eval_utils.py:387-388, 414, 482): edge e (curves, then lines)
    gets fancy_colors(n + 1)[perm][e], perm = torch.randperm(n) drawn from a generator seeded with `seed` (the reference's
    permutation is unseeded), repeated over the edge's samples.  float32 [N,3] in the order of pred.points."""
    n = int(pred.num_curves) + int(pred.num_lines)
    g = torch.Generator().manual_seed(int(seed))
    cols = fancy_colors(n + 1)[torch.randperm(n, generator=g)].numpy()
    counts = np.concatenate([np.asarray(pred.curve_counts, np.int64), np.asarray(pred.line_counts, np.int64)])
    return np.repeat(cols, counts, axis=0).reshape(-1, 3).astype(np.float32)


# ------------------------------------------------------------------------------------------------ GPU ops
def _points(points, name="points"):
    L.require_gpu_tensor(points, name)
    if points.dim() != 2 or points.shape[1] != 3:
        raise L.CurveGSError(f"{name} must be [P,3] (got {tuple(points.shape)})")
    return points.to(torch.float32).contiguous()


def project_points(points, intrinsics, w2c, height, width):
    """(u, v) of every point in every view, float64 [V,P,2] on the points' device, NaN for a dropped point (behind the
    camera, c2 <= 0, or outside 0 <= u < width, 0 <= v < height).  points: float32 [P,3] GPU tensor; intrinsics [V,4]
    (fx, fy, cx, cy) and w2c [V,3,4] float64 host arrays or tensors (``cgs_project_points``)."""
    pts = _points(points)
    dev = pts.device
    V, K, M = _cameras(intrinsics, w2c, L.CurveGSError)
    with L.device_guard(dev):
        K, M = cameras_on(dev, K, M)
        P = pts.shape[0]
        uv = torch.empty((V, P, 2), dtype=torch.float64, device=dev)
        rc = L.load().cgs_project_points(P, L.ptr(pts), V, L.ptr(K), L.ptr(M), int(height), int(width), L.ptr(uv),
                                         L.raw_stream(dev))
        L.check(rc, "cgs_project_points")
    return uv


def render_points(points, colors, intrinsics, w2c, height, width, alpha=ALPHA, background=BACKGROUND,
                  workspace_bytes=None, return_kept=False):
    """float32 [V,height,width,3] images of the points (``cgs_render_points``): a kept point covers pixel
    (floor(u), floor(v)), the points of a pixel are composited in ascending index with constant `alpha` over
    `background`.  points / colors float32 [P,3] GPU tensors on one device; cameras as project_points.  The views are
    processed in chunks that fit `workspace_bytes` of scratch (default: WORKSPACE_BUDGET; the result does not depend on
    it).  With return_kept, also the int32 [V] number of kept points per view."""
    pts = _points(points)
    col = _points(colors, "colors")
    dev = pts.device
    if col.device != dev or col.shape[0] != pts.shape[0]:
        raise L.CurveGSError(f"colors must be [P,3] on {dev} (got {tuple(col.shape)} on {col.device})")
    bg = np.ascontiguousarray(np.asarray(background, np.float64).reshape(3))
    lib = L.load()
    V, K, M = _cameras(intrinsics, w2c, L.CurveGSError)
    with L.device_guard(dev):
        K, M = cameras_on(dev, K, M)
        P, H, W = pts.shape[0], int(height), int(width)
        out = torch.empty((V, max(H, 0), max(W, 0), 3), dtype=torch.float32, device=dev)
        kept = torch.zeros((V,), dtype=torch.int32, device=dev)
        if V > 0:
            need = lib.cgs_render_points_workspace_bytes(P, V, H, W)
            one = lib.cgs_render_points_workspace_bytes(P, 1, H, W)
            budget = WORKSPACE_BUDGET if workspace_bytes is None else int(workspace_bytes)
            nbytes = max(min(need, budget), one)
            ws = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=dev)
            rc = lib.cgs_render_points(P, L.ptr(pts), L.ptr(col), V, L.ptr(K), L.ptr(M), H, W, float(alpha),
                                       bg.ctypes.data_as(L.C.c_void_p), L.ptr(out), L.ptr(kept), L.ptr(ws), nbytes,
                                       L.raw_stream(dev))
            L.check(rc, "cgs_render_points")
    return (out, kept) if return_kept else out


def _depth_planes(what, depth, V):
    """``depth`` as a float32 [V,H,W] tensor (where it is) and its (H, W)."""
    d = depth if torch.is_tensor(depth) else torch.from_numpy(np.array(depth, order="C"))   # (a copy: may be read-only)
    if d.dim() != 3:
        raise ValueError(f"{what}: depth must be float32 [V,H,W] (got {tuple(d.shape)})")
    H, W = int(d.shape[1]), int(d.shape[2])
    return EO._as_depth(d, V, H, W, what), H, W


def project_points_depth(points, intrinsics, w2c, depth, slack=EO.DEPTH_SLACK, return_hidden=False, backend="gpu",
                         device=None):
    """``project_points`` with the depth gate: float64 [V,P,2], NaN for a dropped point -- behind the camera, outside the
    image (``depth``'s size), or HIDDEN: c2 > float64(depth[v][floor(v_px)][floor(u_px)]) + slack (``nv_hidden``).  depth:
    float32 [V,H,W], camera z, +inf where there is no surface.  With return_hidden, also uint8 [V,P]: 1 iff the projection
    kept the point and the gate hid it.  ``backend="gpu"``: ``cgs_project_points_depth``; points and planes are uploaded when
    they are not on a GPU, the results stay on the device.  ``"host"``: ``ops.edge_occlusion.gate_view_host`` per view, CPU
    tensors; the two agree bit for bit."""
    ES._check_backend(backend)
    what = "project_points_depth"
    slack = EO._check_slack(what, slack)
    V, K, M = _cameras(intrinsics, w2c)
    d, H, W = _depth_planes(what, depth, V)
    pts = points if torch.is_tensor(points) else torch.from_numpy(np.ascontiguousarray(points, np.float32).reshape(-1, 3))
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise ValueError(f"points must be [P,3] (got {tuple(pts.shape)})")
    pts = pts.detach().to(torch.float32)
    P = int(pts.shape[0])
    if backend == "host":
        uv = np.full((V, P, 2), np.nan, np.float64)
        hidden = np.zeros((V, P), np.uint8)
        host_pts, planes = ES._host(pts), ES._host(d)
        for i in range(V):
            u, v, seen, hid = EO.gate_view_host(host_pts, K[i], M[i], planes[i], slack)
            uv[i, seen, 0], uv[i, seen, 1] = u[seen], v[seen]
            hidden[i] = hid
        uv, hidden = torch.from_numpy(uv), torch.from_numpy(hidden)
        return (uv, hidden) if return_hidden else uv
    dev = ES._device_for([pts, d], what, device)
    with L.device_guard(dev):
        pts, d = pts.to(dev).contiguous(), d.to(dev)
        Kd, Md = cameras_on(dev, K, M)
        uv = torch.empty((V, P, 2), dtype=torch.float64, device=dev)
        hidden = torch.empty((V, P), dtype=torch.uint8, device=dev) if return_hidden else None
        if V > 0 and P > 0:
            rc = L.load().cgs_project_points_depth(P, L.ptr(pts), V, L.ptr(Kd), L.ptr(Md), H, W, L.ptr(d), slack, L.ptr(uv),
                                                   L.ptr(hidden) if return_hidden else None, L.raw_stream(dev))
            L.check(rc, "cgs_project_points_depth")
    return (uv, hidden) if return_hidden else uv


def render_points_depth(points, colors, intrinsics, w2c, depth, slack=EO.DEPTH_SLACK, alpha=ALPHA, background=BACKGROUND,
                        workspace_bytes=None, return_counts=False):
    """``render_points`` with the depth gate (``cgs_render_points_depth``; GPU only, like ``render_points``): float32
    [V,H,W,3] images, (H, W) the size of ``depth`` (float32 [V,H,W], camera z, +inf where there is no surface; uploaded when
    it is not on the points' device).  A point that its view hides -- ``project_points_depth``'s rule -- is dropped: it is in
    no pixel.  With return_counts, also (kept, hidden) int32 [V]: the drawn points and the hidden ones; kept + hidden is
    ``render_points``'s kept.  The result does not depend on ``workspace_bytes``."""
    what = "render_points_depth"
    pts = _points(points)
    col = _points(colors, "colors")
    dev = pts.device
    if col.device != dev or col.shape[0] != pts.shape[0]:
        raise L.CurveGSError(f"colors must be [P,3] on {dev} (got {tuple(col.shape)} on {col.device})")
    slack = EO._check_slack(what, slack)
    bg = np.ascontiguousarray(np.asarray(background, np.float64).reshape(3))
    lib = L.load()
    V, K, M = _cameras(intrinsics, w2c, L.CurveGSError)
    d, H, W = _depth_planes(what, depth, V)
    if d.is_cuda and d.device != dev:
        raise L.CurveGSError(f"{what}: depth is on {d.device}, the points on {dev}: all tensors must be on one device")
    with L.device_guard(dev):
        K, M = cameras_on(dev, K, M)
        d = d.to(dev)
        P = pts.shape[0]
        out = torch.empty((V, H, W, 3), dtype=torch.float32, device=dev)
        kept = torch.zeros((V,), dtype=torch.int32, device=dev)
        hidden = torch.zeros((V,), dtype=torch.int32, device=dev)
        if V > 0:
            need = lib.cgs_render_points_workspace_bytes(P, V, H, W)
            one = lib.cgs_render_points_workspace_bytes(P, 1, H, W)
            budget = WORKSPACE_BUDGET if workspace_bytes is None else int(workspace_bytes)
            nbytes = max(min(need, budget), one)
            ws = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=dev)
            rc = lib.cgs_render_points_depth(P, L.ptr(pts), L.ptr(col), V, L.ptr(K), L.ptr(M), H, W, L.ptr(d), slack,
                                             float(alpha), bg.ctypes.data_as(L.C.c_void_p), L.ptr(out), L.ptr(kept),
                                             L.ptr(hidden), L.ptr(ws), nbytes, L.raw_stream(dev))
            L.check(rc, "cgs_render_points_depth")
    return (out, kept, hidden) if return_counts else out


# ------------------------------------------------------------------------------------------------ drivers
def _write_images(jobs, pool):
    """jobs: (path, uint8 [H,W,3]); PIL picks the format from the extension, as savefig does."""
    from PIL import Image

    def one(job):
        path, img = job
        Image.fromarray(img, "RGB").save(path)
    list(pool.map(one, jobs))


def render_views(points, colors, cams, out_dir, file_names, device=None, alpha=ALPHA, background=BACKGROUND, depth=None):
    """Renders `points` into every camera and writes <out_dir>/<file_names[v]> for each view with at least one kept
    point (the reference saves nothing for an empty view): round(255 * image) as uint8 RGB.  Views of one size are
    rendered together, OUTPUT_BUDGET bytes of images at a time.  Returns {"views", "written", "gpu_s", "write_s"}: the
    GPU time (render, conversion and copy to the host, synchronised) and the encoding time, in seconds.  ``depth``: None, or
    the scan's ``ops.edge_occlusion.ChunkDepth`` (built for `cams`): every chunk's planes are built on the GPU, a point its
    view hides is not drawn (``render_points_depth``), the budget of a chunk counts the planes' bytes per pixel beside the
    image's, and the stats gain "hidden", the hidden (point, view) pairs."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    pts = torch.from_numpy(np.ascontiguousarray(points, np.float32).reshape(-1, 3)).to(dev)
    col = torch.from_numpy(np.ascontiguousarray(colors, np.float32).reshape(-1, 3)).to(dev)
    stats = {"views": len(cams), "written": 0, "gpu_s": 0.0, "write_s": 0.0}
    gated = depth is not None and depth.gated
    if gated:
        depth.to("gpu", dev)
        stats["hidden"] = 0
    os.makedirs(out_dir, exist_ok=True)
    with ThreadPoolExecutor(max_workers=MAX_WRITERS) as pool:
        # 12 bytes: a float32 RGB pixel
        for H, W, sel, intr, w2c in view_chunks(cams, 12 + (depth.bytes_per_pixel if gated else 0), OUTPUT_BUDGET):
            t0 = time.perf_counter()
            if gated:
                img, kept, hid = render_points_depth(pts, col, intr, w2c, depth.planes(H, W, sel, intr, w2c), depth.slack,
                                                     alpha, background, return_counts=True)
                stats["hidden"] += int(hid.sum().item())
            else:
                img, kept = render_points(pts, col, intr, w2c, H, W, alpha, background, return_kept=True)
            u8 = torch.round(img * 255.0).clamp_(0, 255).to(torch.uint8).cpu().numpy()
            kept = kept.cpu().numpy()
            t1 = time.perf_counter()
            jobs = [(os.path.join(out_dir, file_names[v]), u8[k]) for k, v in enumerate(sel) if kept[k] > 0]
            _write_images(jobs, pool)
            stats["gpu_s"] += t1 - t0
            stats["write_s"] += time.perf_counter() - t1
            stats["written"] += len(jobs)
    return stats


def _scan_points(base_dir, scan, sample_resolution, seed):
    path = os.path.join(base_dir, scan, "parametric_edges.json")
    if not os.path.exists(path):
        log.info(f"Invalid prediction at {scan}")
        return None
    pred = pred_points_and_directions(path, sample_resolution)
    pts = pred.points
    if len(pts) == 0:
        log.info(f"Invalid prediction at {scan}")
        return None
    return pts, edge_point_colors(pred, seed)


def scan_depth(what, scan_dir, cams, occluder=None, depth_dir=None, depth_slack=EO.DEPTH_SLACK,
               depth_window=EO.DEPTH_WINDOW, near_clip=None):
    """The ``ChunkDepth`` of one scan for the scan drivers, or None without a depth source.  ``occluder``: the name of a mesh
    file inside the scan directory (``mesh.ply``); ``depth_dir``: the name of a directory inside it holding one
    ``<image stem>.npy`` depth map per camera (``reprojection.scan_depth_maps``), as the score takes them.  Both together, and
    ``near_clip`` without an occluder, are ValueErrors."""
    if occluder is not None and depth_dir is not None:
        raise ValueError(f"{what}: give an occluder or a depth_dir, not both")
    if near_clip is not None and occluder is None:
        raise ValueError(f"{what}: near_clip needs an occluder (depth maps need no clipping)")
    if occluder is not None:
        return EO.ChunkDepth(what, cams, os.path.join(scan_dir, occluder), None, depth_slack, depth_window, near_clip)
    if depth_dir is not None:
        from .reprojection import scan_depth_maps   # (reprojection imports this module)
        return EO.ChunkDepth(what, cams, None, scan_depth_maps(os.path.join(scan_dir, depth_dir), cams), depth_slack,
                             depth_window)
    return None


def render_abc_novel_views(base_dir, dataset_dir, detector="DexiNed", seed=0, device=None, occluder=None, depth_dir=None,
                           depth_slack=EO.DEPTH_SLACK, depth_window=EO.DEPTH_WINDOW, near_clip=None):
    """eval_ABC.py main with --render_mv (:180-185): for every scan directory of `dataset_dir` (sorted) with a
    <base_dir>/<scan>/parametric_edges.json, the edges sampled every 0.005 are drawn into every camera of
    <dataset_dir>/<scan>/transforms_video.json and written to <base_dir>/<scan>/novel_view/<frame stem>.png.
    Returns {scan: stats of render_views}.  With ``occluder`` or ``depth_dir`` (``scan_depth``; ``depth_slack``,
    ``depth_window``, ``near_clip`` as ``score_edges``) the hidden samples are not drawn and the images go to
    <base_dir>/<scan>/novel_view_visible/ instead: novel_view/ is never touched, so the two sit side by side."""
    out = {}
    for scan in sorted(f.name for f in os.scandir(dataset_dir) if f.is_dir()):
        log.info(f"Processing: {scan}")
        got = _scan_points(base_dir, scan, 0.005, seed)
        if got is None:
            continue
        cams = transforms_video_cameras(os.path.join(dataset_dir, scan), detector)
        depth = scan_depth("render_abc_novel_views", os.path.join(dataset_dir, scan), cams, occluder, depth_dir, depth_slack,
                           depth_window, near_clip)
        out[scan] = render_views(*got, cams, os.path.join(base_dir, scan, "novel_view" if depth is None else VISIBLE_DIR),
                                 [c.name + ".png" for c in cams], device, depth=depth)
    return out


def replica_scans(dataset_dir, scans_file=None):
    """The scan names of a Replica run: the lines of `scans_file` (the reference reads edge_extraction/Replica_scans.txt),
    or every directory of `dataset_dir` holding sparse/0, sorted."""
    if scans_file is not None:
        with open(scans_file) as f:
            return [ln.strip() for ln in f if ln.strip()]
    return sorted(f.name for f in os.scandir(dataset_dir)
                  if f.is_dir() and os.path.isdir(os.path.join(f.path, "sparse", "0")))


def render_replica_novel_views(base_dir, dataset_dir, scans=None, seed=0, device=None, occluder=None, depth_dir=None,
                               depth_slack=EO.DEPTH_SLACK, depth_window=EO.DEPTH_WINDOW, near_clip=None):
    """eval_replica.py process_scan (:100-212) for every scan in `scans` (default: replica_scans(dataset_dir)): the edges
    sampled every 0.0005 are drawn into every COLMAP camera of <dataset_dir>/<scan>/sparse/0 and written to
    <base_dir>/<scan>/novel_view/<image name> (format from the extension).  The comparison video is not made.
    Returns {scan: stats of render_views}.  The depth arguments as ``render_abc_novel_views``: with a depth source the
    images go to <base_dir>/<scan>/novel_view_visible/."""
    out = {}
    for scan in (replica_scans(dataset_dir) if scans is None else scans):
        print(f"Processing: {scan}")
        got = _scan_points(base_dir, scan, REPLICA_SAMPLE_RESOLUTION, seed)
        if got is None:
            continue
        cams = colmap_cameras(os.path.join(dataset_dir, scan))
        depth = scan_depth("render_replica_novel_views", os.path.join(dataset_dir, scan), cams, occluder, depth_dir,
                           depth_slack, depth_window, near_clip)
        out[scan] = render_views(*got, cams, os.path.join(base_dir, scan, "novel_view" if depth is None else VISIBLE_DIR),
                                 [c.name for c in cams], device, depth=depth)
    return out
