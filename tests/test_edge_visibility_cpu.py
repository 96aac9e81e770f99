"""CPU side of the edge-map visibility check against the reference-generated fixture
(tests/golden/make_visibility_golden.py): the float64 restatement (tests/visibility_ref64.py) reproduces the
reference's counts, masks, filtered edges and points; get_edge_maps follows the reference's path rules and rejects
what the reference cannot read; get_parametric_edge(False) is today's writer output; the C ABI rejects bad arguments
before any launch."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

from curve_gaussian_amd import _lib
from curve_gaussian_amd import edge_extraction as EE
from curve_gaussian_amd.scene import dataset_io as IO

import visibility_ref64 as R

GOLD = os.path.join(os.path.dirname(__file__), "golden", "visibility")
G = np.load(os.path.join(GOLD, "visibility.npz"))
DETECTORS = ("DexiNed", "PidiNet")


def _edge_dict():
    return {"lines_end_pts": G["lines"].reshape(-1, 6).tolist(), "curves_ctl_pts": G["curves"].tolist()}


@pytest.mark.parametrize("det", DETECTORS)
def test_restatement_reproduces_the_reference(det):
    maps, intr, c2w, h, w = EE.get_edge_maps(GOLD, det)
    counts = R.visibility_counts(G["curves"], G["lines"], R.map_values(maps, det), intr, c2w, h, w)
    np.testing.assert_array_equal(counts, G[f"{det}_counts"])
    pts, d, cm, lm = R.parametric_edges(G["curves"], G["lines"], counts, len(maps))
    np.testing.assert_array_equal(np.concatenate([cm, lm]), G[f"{det}_mask"])
    np.testing.assert_array_equal(np.asarray(d["curves_ctl_pts"]).reshape(-1, 4, 3), G[f"{det}_curves"])
    np.testing.assert_array_equal(np.asarray(d["lines_end_pts"]).reshape(-1, 6), G[f"{det}_lines"])
    np.testing.assert_array_equal(pts, G[f"{det}_points"])
    assert pts.dtype == np.float32


def test_fixture_covers_the_threshold_and_both_sides_of_it():
    for det in DETECTORS:
        c = G[f"{det}_counts"]
        assert (c == 2).any() and (c == 3).any() and (c == 0).any()
        assert 0 < int(G[f"{det}_mask"].sum()) < len(c)


@pytest.mark.parametrize("det", DETECTORS)
def test_get_edge_maps_reads_the_fixture(det):
    maps, intr, c2w, h, w = EE.get_edge_maps(GOLD, det)
    assert maps.dtype == np.uint8 and maps.shape == (24, 72, 96) and (h, w) == (72, 96)
    np.testing.assert_array_equal(maps, G[f"{det}_u8"])
    meta = json.load(open(os.path.join(GOLD, "meta_data.json")))
    np.testing.assert_array_equal(intr, np.array([f["intrinsics"] for f in meta["frames"]]))
    np.testing.assert_array_equal(c2w, np.array([f["camtoworld"] for f in meta["frames"]])[:, :4, :4])


def test_pidinet_path_rule():
    _, dex = EE.para_edge.edge_map_paths(GOLD, "DexiNed")
    _, pid = EE.para_edge.edge_map_paths(GOLD, "PidiNet")
    assert dex[0] == os.path.join(GOLD, "edge_DexiNed", "00_colors.jpg")      # rgb_path verbatim
    assert pid[0] == os.path.join(GOLD, "edge_PidiNet", "00_colors.png")      # rgb_path[:-4] + ".png"


def _copy_scan(tmp_path):
    dst = str(tmp_path / "scan")
    shutil.copytree(GOLD, dst, ignore=shutil.ignore_patterns("*.npz"))
    return dst


def test_get_edge_maps_errors(tmp_path):
    with pytest.raises(ValueError, match="Unknown detector"):
        EE.get_edge_maps(GOLD, "HED")
    scan = _copy_scan(tmp_path)
    missing = os.path.join(scan, "edge_PidiNet", "05_colors.png")
    os.remove(missing)
    with pytest.raises(FileNotFoundError, match="05_colors.png"):
        EE.get_edge_maps(scan, "PidiNet")
    from PIL import Image
    Image.fromarray(np.zeros((72, 95), np.uint8), mode="L").save(os.path.join(scan, "edge_DexiNed", "03_colors.jpg"),
                                                                format="PNG")
    with pytest.raises(ValueError, match="03_colors.jpg"):
        EE.get_edge_maps(scan, "DexiNed")
    meta = json.load(open(os.path.join(scan, "meta_data.json")))
    meta["frames"] = []
    json.dump(meta, open(os.path.join(scan, "meta_data.json"), "w"))
    with pytest.raises(ValueError, match="no frames"):
        EE.get_edge_maps(scan, "DexiNed")


def test_non_grayscale_maps_are_converted(tmp_path):
    from PIL import Image
    scan = _copy_scan(tmp_path)
    p = os.path.join(scan, "edge_PidiNet", "00_colors.png")
    g = np.array(Image.open(p))
    Image.fromarray(np.stack([g, g, g], -1), mode="RGB").save(p)
    maps, *_ = EE.get_edge_maps(scan, "PidiNet")
    np.testing.assert_array_equal(maps[0], g)                     # equal channels: the conversion keeps the value
    np.testing.assert_array_equal(maps[1:], G["PidiNet_u8"][1:])


def test_get_parametric_edge_without_checking_is_todays_writer_output():
    d = _edge_dict()
    pts, ret = EE.get_parametric_edge(False, d)
    curves = np.array(d["curves_ctl_pts"]).reshape(-1, 12).reshape(-1, 4, 3)
    lines = np.array(d["lines_end_pts"]).reshape(-1, 6)
    assert ret == {"curves_ctl_pts": curves.tolist(), "lines_end_pts": lines.tolist()}
    np.testing.assert_array_equal(pts, IO.sample_edge_points(curves, lines))
    assert list(ret) == ["curves_ctl_pts", "lines_end_pts"]


def test_get_parametric_edge_needs_the_scan_dir():
    with pytest.raises(ValueError, match="meta_data_dir"):
        EE.get_parametric_edge(True, _edge_dict())


def test_thresholds_are_the_references():
    assert (EE.EDGE_VISIBILITY_THRESHOLD, EE.EDGE_MAX_THRESHOLD, EE.EDGE_VISIBILITY_FRAMES_RATIO) == (0.1, 0.5, 0.05)
    assert [EE.edge_visibility_frames(f) for f in (1, 20, 24, 64, 65, 70, 200)] == [1, 1, 2, 4, 4, 4, 10]


def test_compute_visibility_rejects_cpu_tensors():
    c = torch.zeros((1, 4, 3), dtype=torch.float64)
    ln = torch.zeros((1, 2, 3), dtype=torch.float64)
    maps = torch.zeros((1, 4, 4), dtype=torch.uint8)
    with pytest.raises(_lib.CurveGSError, match="GPU tensor"):
        EE.compute_visibility(c, ln, maps, np.eye(3)[None], np.eye(4)[None], "DexiNed")


def test_abi_rejects_invalid_arguments_before_launch():
    lib = _lib.load()
    one = torch.zeros(16, dtype=torch.float64)
    p = _lib.ptr(one)
    INVALID = -1                                               # CGS_ERR_INVALID_ARGUMENT
    assert lib.cgs_edge_visibility(0, None, 0, None, 5, None, None, 0, 0, None, 1, None, None) == 0   # E = 0: no-op
    for args in [(-1, p, 0, None, 1, p, p, 4, 4, p, 1, p),      # negative sizes
                 (1, p, -1, None, 1, p, p, 4, 4, p, 1, p),
                 (1, p, 0, None, -1, p, p, 4, 4, p, 1, p),
                 (1, p, 0, None, 1, p, p, 0, 4, p, 1, p),       # height / width <= 0 with frames
                 (1, p, 0, None, 1, p, p, 4, -3, p, 1, p),
                 (1, None, 0, None, 1, p, p, 4, 4, p, 1, p),    # NULL with a non-zero size
                 (0, None, 1, None, 1, p, p, 4, 4, p, 1, p),
                 (1, p, 0, None, 1, None, p, 4, 4, p, 1, p),
                 (1, p, 0, None, 1, p, None, 4, 4, p, 1, p),
                 (1, p, 0, None, 1, p, p, 4, 4, None, 1, p),
                 (1, p, 0, None, 1, p, p, 4, 4, p, 1, None)]:
        rc = lib.cgs_edge_visibility(*args, None)
        assert rc == INVALID, args
        assert "cgs_edge_visibility: invalid argument" in _lib.last_error()
