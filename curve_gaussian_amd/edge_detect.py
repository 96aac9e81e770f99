"""python -m curve_gaussian_amd.edge_detect --scan DIR [--images images] [--sigma S --low L --high H --no_thin]
                                           [--backend gpu|host] [--overwrite]

Edge maps from a scan's photographs, so that a scan that holds only photographs and poses can be trained on:

    python -m curve_gaussian_amd.edge_detect --scan SCAN
    python -m curve_gaussian_amd.train -s SCAN -m OUT --detector PidiNet

The detector is the classical one of ``ops.edge_detect`` (Gaussian smoothing, Sobel gradient, thinning, hysteresis, soft
response): no counterpart in the reference, and not a substitute for the learned detectors (DexiNed, PidiNet) in quality.
Its defaults are untuned.  The scan layout is told apart the way ``Scene`` does it:

  COLMAP (a ``sparse/`` folder)   reads every image named in ``sparse/0`` from ``<images>/``, writes the file
                                  ``colmap_io.edge_map_path(scan, images, name, "PidiNet")`` names
  EMAP (``meta_data.json``)       reads ``color/<rgb_path>`` of every frame, writes ``edge_PidiNet/<rgb_path>``, the name
                                  ``read_emap`` opens; an ``rgb_path`` that does not end in ``.png`` is refused (the two
                                  readers of that folder disagree on the name then)

The maps go into the ``edge_PidiNet`` slot because there bright means edge for every reader: training and the visibility
check of the extraction read such a file the same way.  The ``edge_DexiNed`` slot is not offered: the reference trains on
its files as they are but inverts them in the visibility check.  Output: 8-bit grayscale PNGs, value round(255 e), and
a ``detector.json`` with the parameters next to them.  An existing output folder is left alone without ``--overwrite``."""
import argparse
import json
import os
import sys

import numpy as np
import torch

from . import _lib as L
from .ops.edge_detect import detect_edges, gaussian_taps, _check_backend, _check_thresholds

SLOT = "PidiNet"


def _scan_files(scan_dir, images):
    """``(pairs, out_dir)``: (photograph, edge map) paths of every view, and the folder ``detector.json`` goes to."""
    if os.path.exists(os.path.join(scan_dir, "sparse")):
        from .scene import colmap_io
        _, extrinsics = colmap_io.read_model(os.path.join(scan_dir, "sparse/0"))
        folder = "images" if images is None else images
        pairs = [(os.path.join(scan_dir, folder, e.name), colmap_io.edge_map_path(scan_dir, images, e.name, SLOT))
                 for e in extrinsics.values()]
        out_dir = os.path.dirname(colmap_io.edge_map_path(scan_dir, images, "x.png", SLOT))
    else:
        from .scene.dataset_io import DETECTOR_DIRS
        with open(os.path.join(scan_dir, "meta_data.json")) as f:
            meta = json.load(f)
        pairs = []
        for frame in meta["frames"]:
            rgb_path = frame["rgb_path"]
            if not rgb_path.endswith(".png"):
                raise ValueError(f"edge_detect: rgb_path {rgb_path!r} does not end in .png: the loader and the extraction would "
                                 "look for its edge map under different names")
            pairs.append((os.path.join(scan_dir, "color", rgb_path), os.path.join(scan_dir, DETECTOR_DIRS[SLOT], rgb_path)))
        out_dir = os.path.join(scan_dir, DETECTOR_DIRS[SLOT])
    for src, dst in pairs:
        if os.path.abspath(src) == os.path.abspath(dst):
            raise ValueError(f"edge_detect: the edge map of {src} would replace the photograph itself (the image folder's "
                             "name must contain 'images')")
    return pairs, out_dir


def _decode(path):
    from PIL import Image
    with Image.open(path) as im:
        if im.mode not in ("L", "RGB", "RGBA"):
            im = im.convert("RGB")
        return torch.from_numpy(np.array(im, dtype=np.uint8))


def detect_scan(scan_dir, images=None, sigma=1.4, low=0.05, high=0.15, thin=True, backend="gpu", overwrite=False):
    """Writes the edge map of every view of the scan (see the module's text) and returns the list of files written.  Views
    are decoded with PIL and processed ``_lib.EDGE_MAX_VIEWS`` at a time; of each chunk only the 8-bit maps come back to
    the host."""
    from PIL import Image
    _check_backend(backend)
    _check_thresholds(low, high)
    gaussian_taps(sigma)
    pairs, out_dir = _scan_files(scan_dir, images)
    if os.path.exists(out_dir) and not overwrite:
        raise FileExistsError(f"edge_detect: {out_dir} exists and is left untouched; pass --overwrite (overwrite=True) to "
                              "write into it")
    stats = {}
    written = []
    for first in range(0, len(pairs), L.EDGE_MAX_VIEWS):
        chunk = pairs[first:first + L.EDGE_MAX_VIEWS]
        maps = detect_edges([_decode(src) for src, _ in chunk], sigma, low, high, thin, backend, stats)
        for (_, dst), e in zip(chunk, maps):
            q = torch.round(e[0] * 255.0).to(torch.uint8).cpu().numpy()
            os.makedirs(os.path.dirname(dst), exist_ok=True)
            Image.fromarray(q, mode="L").save(dst)
            written.append(dst)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "detector.json"), "w") as f:
        json.dump({"detector": "canny", "sigma": float(sigma), "low": float(low), "high": float(high), "thin": bool(thin),
                   "backend": backend, "views": len(written), "propagation_rounds": stats.get("rounds", [])}, f, indent=1)
    return written


def main(argv=None):
    p = argparse.ArgumentParser(prog="python -m curve_gaussian_amd.edge_detect", description="Edge maps from a scan's photographs: a classical Canny detector with a soft response; "
                                            "the maps go into the scan's edge_PidiNet folder.  The defaults are untuned.")
    p.add_argument("--scan", required=True, help="the scan: a COLMAP folder (sparse/0 + images) or an EMAP one (meta_data.json + color)")
    p.add_argument("--images", default=None, help="COLMAP only: the image folder (default: images)")
    p.add_argument("--sigma", type=float, default=1.4, help="Gaussian smoothing, 0..4 (0: none)")
    p.add_argument("--low", type=float, default=0.05, help="hysteresis: candidates have a thinned magnitude >= low")
    p.add_argument("--high", type=float, default=0.15, help="hysteresis: strong pixels have one >= high; the response saturates there")
    p.add_argument("--no_thin", action="store_true", help="skip non-maximum suppression")
    p.add_argument("--backend", choices=("gpu", "host"), default="gpu")
    p.add_argument("--overwrite", action="store_true", help="write into an existing output folder")
    a = p.parse_args(argv)
    written = detect_scan(a.scan, images=a.images, sigma=a.sigma, low=a.low, high=a.high, thin=not a.no_thin, backend=a.backend,
                          overwrite=a.overwrite)
    print(f"edge_detect: wrote {len(written)} edge maps" + (f" into {os.path.dirname(written[0])}" if written else ""))
    return 0


if __name__ == "__main__":
    sys.exit(main())
