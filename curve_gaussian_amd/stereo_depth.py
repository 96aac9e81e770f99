"""python -m curve_gaussian_amd.stereo_depth --scan DIR [--images images] [--detector PidiNet] [--out DIR] [--bounds ...]
                                             [--hypotheses D --patch_radius R --sources S ...] [--backend gpu|host] [--overwrite]
                                             [--fuse [--fuse_sources F] [--fuse_support N]] [--fuse_from DIR]

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
left alone without ``--overwrite``.

``--fuse`` (OFF BY DEFAULT; ``--fuse_sources`` and ``--fuse_support`` are UNTUNED): the filtered maps are fused across views
(``ops.stereo_depth.fuse_depth``: a pixel that its own view failed to match gets the depth its neighbours agree on) and
written to ``<scan>/depth_stereo_fused`` instead; ``stereo.json`` then also holds ``"fused": true``, the two parameters and
the fusion's figures.  The chain becomes

    python -m curve_gaussian_amd.stereo_depth --scan SCAN --fuse
    ... --depth_dir depth_stereo_fused --depth_slack <recommended_slack of SCAN/depth_stereo_fused/stereo.json>

``--fuse_from DIR`` fuses the maps of that folder (the caller's own, one ``<image stem>.npy`` per view as ``--depth_dir``
reads them) without sweeping: no photograph is read; the tolerance comes from ``--bounds``, ``--hypotheses`` and
``--consistency_steps``.  Without these flags every file written is byte for byte what it was."""
import argparse
import json
import os
import sys

import numpy as np

from .ops import stereo_depth as SD

OUT_DIR = "depth_stereo"
FUSED_DIR = "depth_stereo_fused"
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


def _check_out(out_dir, overwrite):
    if os.path.exists(out_dir) and not overwrite:
        raise FileExistsError(f"stereo_depth: {out_dir} exists and is left untouched; pass --overwrite (overwrite=True) to "
                              "write into it")


def _write_maps(out_dir, cams, maps):
    os.makedirs(out_dir, exist_ok=True)
    written = []
    for c, m in zip(cams, maps):
        written.append(os.path.join(out_dir, os.path.splitext(os.path.basename(c.name))[0] + ".npy"))
        np.save(written[-1], m)
    return written


def fuse_scan(scan_dir, fuse_from, detector="PidiNet", out=None, overwrite=False, backend="gpu", fuse_sources=SD.FUSE_SOURCES,
              fuse_support=SD.FUSE_SUPPORT, bounds=SD.BOUNDS, hypotheses=SD.HYPOTHESES, max_angle_deg=SD.MAX_ANGLE_DEG,
              consistency_steps=SD.CONSISTENCY_STEPS):
    """``--fuse_from``: fuses the maps of ``fuse_from`` (a folder, inside the scan unless it is absolute) and writes them and
    ``stereo.json``; returns the files written.  Nothing is swept and no photograph is read."""
    from .edge_extraction import reprojection as RP
    out_dir = os.path.join(scan_dir, FUSED_DIR) if out is None else out
    _check_out(out_dir, overwrite)
    if os.path.exists(os.path.join(scan_dir, "sparse")):
        cams, _ = RP.colmap_scan_cameras(scan_dir, detector)
    else:
        cams, _ = RP.emap_cameras(scan_dir, detector)
    maps, info = SD.fuse_depth(RP.scan_depth_maps(os.path.join(scan_dir, fuse_from), cams), cams, bounds, hypotheses, max_angle_deg, consistency_steps,
                               fuse_sources, fuse_support, backend, return_info=True)
    written = _write_maps(out_dir, cams, maps)
    report = {"method": "map_fusion", "backend": backend, "detector": detector, "fuse_from": fuse_from, "fused": True,
              "fuse_sources": int(fuse_sources), "fuse_support": int(fuse_support),
              "bounds": np.asarray(bounds, np.float64).tolist(), "hypotheses": int(hypotheses),
              "max_angle_deg": max_angle_deg, "consistency_steps": consistency_steps,
              "views": [{"name": c.name, "coverage": cov} for c, cov in zip(cams, info["coverage"])], "fusion": info}
    with open(os.path.join(out_dir, "stereo.json"), "w") as f:
        json.dump(report, f, indent=1)
    return written


def stereo_scan(scan_dir, images=None, detector="PidiNet", out=None, overwrite=False, backend="gpu", fuse=False,
                fuse_sources=SD.FUSE_SOURCES, fuse_support=SD.FUSE_SUPPORT, **params):
    """Writes the depth map of every view of the scan and ``stereo.json`` (see the module's text); returns the files
    written.  ``params``: the keyword arguments of ``ops.stereo_depth.stereo_depth`` but those of the fusion, which are
    ``fuse``, ``fuse_sources`` and ``fuse_support`` here."""
    from .edge_detect import _decode
    out_dir = os.path.join(scan_dir, FUSED_DIR if fuse else OUT_DIR) if out is None else out
    _check_out(out_dir, overwrite)
    cams, paths = scan_photographs(scan_dir, images, detector)
    gray = []
    for c, p in zip(cams, paths):
        g = SD.luminance(_decode(p))
        if g.shape != (c.height, c.width):
            raise ValueError(f"stereo_depth: the photograph {p} is {g.shape[1]}x{g.shape[0]} and its camera "
                             f"{c.width}x{c.height}")
        gray.append(g)
    fusion = dict(fuse=True, fuse_sources=fuse_sources, min_support=fuse_support) if fuse else {}
    maps, info = SD.stereo_depth(gray, cams, backend=backend, return_info=True, **params, **fusion)
    written = _write_maps(out_dir, cams, maps)
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
    if fuse:
        report.update({"fused": True, "fuse_sources": int(fuse_sources), "fuse_support": int(fuse_support),
                       "fusion": info["fusion"]})
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
    p.add_argument("--fuse", action="store_true",
                   help=f"fuse the maps across views before writing them (default folder: <scan>/{FUSED_DIR}); off by default")
    p.add_argument("--fuse_sources", type=int, default=SD.FUSE_SOURCES, help="the views warped into each view (untuned)")
    p.add_argument("--fuse_support", type=int, default=SD.FUSE_SUPPORT,
                   help="the agreeing depths a fused pixel needs, its own included (untuned)")
    p.add_argument("--fuse_from", default=None, metavar="DIR",
                   help="fuse the maps of this folder (one <image stem>.npy per view) instead of sweeping")
    a = p.parse_args(argv)
    bounds = SD.BOUNDS if a.bounds is None else (tuple(a.bounds[:3]), tuple(a.bounds[3:]))
    if a.fuse_from is not None:
        written = fuse_scan(a.scan, a.fuse_from, detector=a.detector, out=a.out, overwrite=a.overwrite, backend=a.backend,
                            fuse_sources=a.fuse_sources, fuse_support=a.fuse_support, bounds=bounds, hypotheses=a.hypotheses,
                            max_angle_deg=a.max_angle_deg, consistency_steps=a.consistency_steps)
        print(f"stereo_depth: wrote {len(written)} fused depth maps" + (f" into {os.path.dirname(written[0])}" if written else ""))
        return 0
    fusion = dict(fuse=True, fuse_sources=a.fuse_sources, fuse_support=a.fuse_support) if a.fuse else {}
    written = stereo_scan(a.scan, images=a.images, detector=a.detector, out=a.out, overwrite=a.overwrite, backend=a.backend,
                          bounds=bounds, hypotheses=a.hypotheses, patch_radius=a.patch_radius, sources=a.sources,
                          max_angle_deg=a.max_angle_deg, min_var=a.min_var, max_cost=a.max_cost, min_sources=a.min_sources,
                          consistency_steps=a.consistency_steps, min_consistent=a.min_consistent, **fusion)
    print(f"stereo_depth: wrote {len(written)} depth maps" + (f" into {os.path.dirname(written[0])}" if written else ""))
    return 0


if __name__ == "__main__":
    sys.exit(main())
