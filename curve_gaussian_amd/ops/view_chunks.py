"""The driver that every multi-view edge-map operator shares (``score_edges``, ``edge_support``, ``seed_points``,
``render_views``): one stored uint8 map per camera, the views grouped by size and cut into chunks that fit a byte budget,
the cameras of a chunk as arrays and its stored bytes as detected masks.  Plain functions over numpy and torch: nothing
here loads the library, and a caller keeps its own bytes-per-pixel constant and default budget -- they document its
working set."""
import numpy as np
import torch


def camera_arrays(cams):
    """(intrinsics [V,4] = (fx, fy, cx, cy), w2c [V,3,4] = [R | T]) float64 host arrays of a list of cameras."""
    intr = np.array([[c.fx, c.fy, c.cx, c.cy] for c in cams], np.float64).reshape(-1, 4)
    w2c = np.array([np.concatenate([c.R, c.T[:, None]], 1) for c in cams], np.float64).reshape(-1, 3, 4)
    return intr, w2c


def detected_lut(detector, edge_threshold):
    """bool [256]: is a stored byte u a detected edge pixel?  e > edge_threshold with e = 1 - u/255.0 (DexiNed) or u/255.0
    (PidiNet) in float64, the conversions of para_edge / cgs_edge_visibility."""
    u = np.arange(256, dtype=np.float64)
    if detector == "DexiNed":
        e = 1 - u / 255.0
    elif detector == "PidiNet":
        e = u / 255.0
    else:
        raise ValueError(f"Unknown detector: {detector}")
    return e > float(edge_threshold)


def check_edge_maps(what, cameras, edge_maps_u8):
    """(cameras, maps) as lists: one uint8 [H,W] array per camera, each of its camera's size; ValueError otherwise."""
    cameras = list(cameras)
    maps = [np.asarray(m) for m in edge_maps_u8]
    if len(maps) != len(cameras):
        raise ValueError(f"{what}: {len(cameras)} cameras and {len(maps)} edge maps")
    for c, m in zip(cameras, maps):
        if m.dtype != np.uint8 or m.shape != (c.height, c.width):
            raise ValueError(f"{what}: the edge map of {c.name} must be uint8 [{c.height},{c.width}] (got {m.dtype} "
                             f"{m.shape})")
    return cameras, maps


def check_budget(what, budget_bytes, default):
    budget = default if budget_bytes is None else int(budget_bytes)
    if budget <= 0:
        raise ValueError(f"{what}: budget_bytes must be positive (got {budget})")
    return budget


def view_chunks(cameras, bytes_per_pixel, budget):
    """Yields (H, W, sel, intr, w2c): the views grouped by size, the sizes in first-seen order and the views of a size in
    camera order, ``max(1, budget // (bytes_per_pixel * H * W))`` of them at a time.  ``sel`` lists the chunk's indices
    into ``cameras``; intr, w2c are its ``camera_arrays``."""
    by_size = {}
    for v, c in enumerate(cameras):
        by_size.setdefault((c.height, c.width), []).append(v)
    for (H, W), idx in by_size.items():
        per = max(1, budget // (bytes_per_pixel * H * W))
        for b in range(0, len(idx), per):
            sel = idx[b:b + per]
            yield (H, W, sel) + camera_arrays([cameras[v] for v in sel])


def detected_masks(lut, maps, sel):
    """uint8 [len(sel),H,W] CPU tensor: the detected masks of the views ``sel`` (of one size) through ``detected_lut``."""
    return torch.from_numpy(lut[np.stack([maps[v] for v in sel])].astype(np.uint8))
