"""python -m curve_gaussian_amd.stereo_depth --scan DIR [--images images] [--detector PidiNet] [--out DIR] [--bounds ...]
                                             [--hypotheses D --patch_radius R --sources S ...] [--backend gpu|host] [--overwrite]

Depth maps from a scan's own photographs, so that the depth gate works on a scan that holds only photographs and poses:

    python -m curve_gaussian_amd.edge_detect --scan SCAN
    python -m curve_gaussian_amd.stereo_depth --scan SCAN
    ... --depth_dir depth_stereo --depth_slack <recommended_slack of SCAN/depth_stereo/stereo.json>

Plane-sweep stereo of ``ops.stereo_depth`` (no counterpart in the reference; not a substitute for a dense reconstruction in
quality, and EVERY DEFAULT IS UNTUNED).  The photographs are listed the way ``edge_detect`` lists them (COLMAP: every image
of ``sparse/0`` in ``<images>/``; EMAP: ``color/<rgb_path>`` of every frame) and the cameras are those that
``edge_extraction.reprojection`` forms for the scan (``colmap_scan_cameras`` / ``emap_cameras``, which read the scan through
its ``--detector`` edge maps: run ``edge_detect`` first), so a map has its camera's size and pose.  A photograph whose
size is not its camera's is a ValueError.

Output: ``<out>/<image stem>.npy`` per view -- float32 [H,W], camera z, 0 where stereo gives nothing, which
``--depth_dir`` / ``--init_depth_dir`` take as they are -- and ``<out>/stereo.json`` with every parameter, the per-view
coverage, ``depth_step_max`` and ``recommended_slack``.  ``<out>`` defaults to ``<scan>/depth_stereo``; an existing folder is
left alone without ``--overwrite``."""
import argparse
import json
import os
import sys

import numpy as np

from .ops import stereo_depth as SD

OUT_DIR = "depth_stereo"
SLACK_NOTE = ("the depth gate's default slack (0.001) is far below what stereo resolves: pass recommended_slack as "
              "--depth_slack with these maps")


def scan_photographs(scan_dir, images=None, detector="PidiNet"):
    """(cameras, photograph paths) of a scan: the cameras of ``edge_extraction.reprojection`` and, per camera, the
    photograph ``edge_detect._scan_files`` lists under the same image stem."""
    from .edge_detect import _scan_files
    from .edge_extraction import reprojection as RP
    pairs, _ = _scan_files(scan_dir, images)
    if os.path.exists(os.path.join(scan_dir, "sparse")):
        cams, _ = RP.colmap_scan_cameras(scan_dir, detector)
    else:
        cams, _ = RP.emap_cameras(scan_dir, detector)
    stem = lambda p: os.path.splitext(os.path.basename(p))[0]
    by_stem = {stem(src): src for src, _ in pairs}
    missing = [c.name for c in cams if stem(c.name) not in by_stem]
    if missing:
        raise FileNotFoundError(f"stereo_depth: no photograph for {missing[0]} in {scan_dir}")
    return cams, [by_stem[stem(c.name)] for c in cams]


def stereo_scan(scan_dir, images=None, detector="PidiNet", out=None, overwrite=False, backend="gpu", **params):
    """Writes the depth map of every view of the scan and ``stereo.json`` (see the module's text); returns the files
    written.  ``params``: the keyword arguments of ``ops.stereo_depth.stereo_depth``."""
    from .edge_detect import _decode
    out_dir = os.path.join(scan_dir, OUT_DIR) if out is None else out
    if os.path.exists(out_dir) and not overwrite:
        raise FileExistsError(f"stereo_depth: {out_dir} exists and is left untouched; pass --overwrite (overwrite=True) to "
                              "write into it")
    cams, paths = scan_photographs(scan_dir, images, detector)
    gray = []
    for c, p in zip(cams, paths):
        g = SD.luminance(_decode(p))
        if g.shape != (c.height, c.width):
            raise ValueError(f"stereo_depth: the photograph {p} is {g.shape[1]}x{g.shape[0]} and its camera "
                             f"{c.width}x{c.height}")
        gray.append(g)
    maps, info = SD.stereo_depth(gray, cams, backend=backend, return_info=True, **params)
    os.makedirs(out_dir, exist_ok=True)
    written = []
    for c, m in zip(cams, maps):
        written.append(os.path.join(out_dir, os.path.splitext(os.path.basename(c.name))[0] + ".npy"))
        np.save(written[-1], m)
    defaults = dict(bounds=SD.BOUNDS, hypotheses=SD.HYPOTHESES, patch_radius=SD.PATCH_RADIUS, sources=SD.SOURCES,
                    max_angle_deg=SD.MAX_ANGLE_DEG, min_var=SD.MIN_VAR, max_cost=SD.MAX_COST, min_sources=SD.MIN_SOURCES,
                    consistency_steps=SD.CONSISTENCY_STEPS, min_consistent=SD.MIN_CONSISTENT)
    defaults.update(params)
    report = {"method": "plane_sweep", "backend": backend, "detector": detector, "z_floor": SD.STEREO_Z_FLOOR}
    report.update({k: (np.asarray(v, np.float64).tolist() if k == "bounds" else v) for k, v in defaults.items()})
    report.update({"views": [{"name": c.name, "coverage": cov, "swept": s}
                             for c, cov, s in zip(cams, info["coverage"], info["swept"])],
                   "depth_step_max": info["depth_step_max"], "recommended_slack": info["recommended_slack"],
                   "note": SLACK_NOTE})
    with open(os.path.join(out_dir, "stereo.json"), "w") as f:
        json.dump(report, f, indent=1)
    return written


def main(argv=None):
    p = argparse.ArgumentParser(prog="python -m curve_gaussian_amd.stereo_depth",
                                description="Depth maps from a scan's photographs by plane-sweep stereo, in the format "
                                            "--depth_dir reads.  Every default is untuned.")
    p.add_argument("--scan", required=True, help="the scan: a COLMAP folder (sparse/0 + images) or an EMAP one (meta_data.json + color)")
    p.add_argument("--images", default=None, help="COLMAP only: the image folder (default: images)")
    p.add_argument("--detector", default="PidiNet", help="the edge maps through which the scan's cameras are read")
    p.add_argument("--out", default=None, help=f"the folder to write (default: <scan>/{OUT_DIR})")
    p.add_argument("--bounds", type=float, nargs=6, default=None, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"),
                   help="the box the scene lies in; the hypotheses span its depth range (default: the unit cube)")
    p.add_argument("--hypotheses", type=int, default=SD.HYPOTHESES)
    p.add_argument("--patch_radius", type=int, default=SD.PATCH_RADIUS)
    p.add_argument("--sources", type=int, default=SD.SOURCES)
    p.add_argument("--max_angle_deg", type=float, default=SD.MAX_ANGLE_DEG)
    p.add_argument("--min_var", type=float, default=SD.MIN_VAR)
    p.add_argument("--max_cost", type=float, default=SD.MAX_COST)
    p.add_argument("--min_sources", type=int, default=SD.MIN_SOURCES)
    p.add_argument("--consistency_steps", type=float, default=SD.CONSISTENCY_STEPS)
    p.add_argument("--min_consistent", type=int, default=SD.MIN_CONSISTENT)
    p.add_argument("--backend", choices=("gpu", "host"), default="gpu")
    p.add_argument("--overwrite", action="store_true", help="write into an existing output folder")
    a = p.parse_args(argv)
    bounds = SD.BOUNDS if a.bounds is None else (tuple(a.bounds[:3]), tuple(a.bounds[3:]))
    written = stereo_scan(a.scan, images=a.images, detector=a.detector, out=a.out, overwrite=a.overwrite, backend=a.backend,
                          bounds=bounds, hypotheses=a.hypotheses, patch_radius=a.patch_radius, sources=a.sources,
                          max_angle_deg=a.max_angle_deg, min_var=a.min_var, max_cost=a.max_cost, min_sources=a.min_sources,
                          consistency_steps=a.consistency_steps, min_consistent=a.min_consistent)
    print(f"stereo_depth: wrote {len(written)} depth maps" + (f" into {os.path.dirname(written[0])}" if written else ""))
    return 0


if __name__ == "__main__":
    sys.exit(main())
