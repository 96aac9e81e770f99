"""GPU: the depth-gated control-point visibility kernel (cgs_edge_visibility_depth) against the numpy back end bit for bit
-- the planted scene, random scenes in which both verdicts are common, both detectors --, against cgs_edge_visibility with
an all-+inf depth, and get_parametric_edge / the visibility tool with an occluder on a written box scan."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import edge_visgate_cases as C
from curve_gaussian_amd import edge_extraction as EE
from curve_gaussian_amd.edge_extraction import para_edge as PE
from curve_gaussian_amd.scene import dataset_io as IO
from curve_gaussian_amd.scene import solid_scan as SS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")


def _both(s, detector, depth=None):
    args = (s["curves"], s["lines"], s["maps"], s["K"], s["c2w"], detector, s["depth"] if depth is None else depth, s["slack"])
    host = PE.edge_visibility_counts_depth(*args, backend="host")
    a = PE.edge_visibility_counts_depth(*args, backend="gpu", device=DEV)
    b = PE.edge_visibility_counts_depth(*args, backend="gpu", device=DEV)
    torch.cuda.synchronize()
    assert a.dtype == torch.int32 and a.is_cuda and tuple(a.shape) == tuple(host.shape)
    assert torch.equal(a, b), "two runs differ"
    return a.cpu().numpy(), host.numpy()


def test_planted_scene_equals_the_host_and_the_hand_written_counts():
    s = C.planted_scene()
    got, host = _both(s, "PidiNet")
    np.testing.assert_array_equal(got, host)
    np.testing.assert_array_equal(got, s["want"])
    got, host = _both(s, "DexiNed")   # every value is 0: nothing is visible, the gate touches the same cells
    np.testing.assert_array_equal(got, host)
    assert not got[:, 0].any()
    np.testing.assert_array_equal(got[:, 1], s["want"][:, 1])


@pytest.mark.parametrize("detector", ["PidiNet", "DexiNed"])
@pytest.mark.parametrize("size", C.RANDOM_SIZES)
@pytest.mark.parametrize("shape", C.RANDOM_SHAPES)
def test_random_scenes_equal_the_host_bit_for_bit(shape, size, detector):
    s = C.random_scene(*shape, *size, seed=1)
    got, host = _both(s, detector)
    np.testing.assert_array_equal(got, host)
    if shape[0] + shape[1] == 0:
        assert got.shape == (0, 2)
        return
    # not vacuous: the gate touches 10 % to 90 % of the cells that keep a point (a cell keeps one iff it is visible on an
    # all-255 map without the gate)
    inf = np.full_like(s["depth"], np.inf)
    kept = _both(dict(s, maps=np.full_like(s["maps"], 255)), "PidiNet", inf)[0][:, 0].sum()
    assert 0.1 * kept <= got[:, 1].sum() <= 0.9 * kept, (got[:, 1].sum(), kept)
    assert got[:, 0].sum() > 0
    # an all-+inf depth: the ungated kernel's counts, and the gate touches nothing
    plain, _ = _both(s, detector, inf)
    c, ln, m = (torch.from_numpy(np.ascontiguousarray(s[k])).to(DEV) for k in ("curves", "lines", "maps"))
    want = EE.edge_visibility_counts(c, ln, m, s["K"], s["c2w"], detector).cpu().numpy()
    np.testing.assert_array_equal(plain[:, 0], want)
    assert not plain[:, 1].any()


@pytest.fixture(scope="module")
def box(tmp_path_factory):
    scan = SS.solid_scan("box", C.BOX_VIEWS, C.BOX_H, C.BOX_W, backend="gpu", device=DEV)
    path = str(tmp_path_factory.mktemp("visgate") / "box")
    SS.write_solid_scan(path, scan)
    truth = np.asarray(scan.edges["lines_end_pts"], np.float64).reshape(-1, 2, 3)
    lines = np.concatenate([truth, C.interior_segments(scan.tris)])
    return dict(path=path, d={"curves_ctl_pts": [], "lines_end_pts": lines.reshape(-1, 6).tolist()}, truth=truth)


def test_get_parametric_edge_with_an_occluder_returns_exactly_the_box(box, capsys):
    mesh = os.path.join(box["path"], "mesh.ply")
    pts, ret = EE.get_parametric_edge(True, box["d"], box["path"], "PidiNet", occluder=mesh)
    assert ret == {"curves_ctl_pts": [], "lines_end_pts": box["truth"].reshape(-1, 6).tolist()}
    np.testing.assert_array_equal(pts, IO.sample_edge_points(np.zeros((0, 4, 3)), box["truth"].reshape(-1, 6)))
    assert "before visible checking:  212 after visible checking:  12" in capsys.readouterr().out
    _, host = EE.get_parametric_edge(True, box["d"], box["path"], "PidiNet", occluder=mesh, backend="host")
    assert host == ret
    _, ungated = EE.get_parametric_edge(True, box["d"], box["path"], "PidiNet")
    assert len(ungated["lines_end_pts"]) >= 12 + 40   # what the gate is for


def test_the_visibility_tool_with_an_occluder_writes_the_same_file(box, tmp_path):
    edges = str(tmp_path / "all.json")
    json.dump(box["d"], open(edges, "w"))
    pts, ret = EE.get_parametric_edge(True, box["d"], box["path"], "PidiNet", occluder=os.path.join(box["path"], "mesh.ply"))
    want = str(tmp_path / "want")
    IO.write_edge_files(want, ret, pts)
    out = str(tmp_path / "cli")
    r = subprocess.run([sys.executable, "-m", "curve_gaussian_amd.edge_extraction.visibility", "--edges", edges, "--scan_dir",
                        box["path"], "--detector", "PidiNet", "--out", out, "--occluder", "mesh.ply"], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "before visible checking:  212 after visible checking:  12" in r.stdout
    for name in ("parametric_edges.json", "edge_points.ply"):
        assert open(os.path.join(out, name), "rb").read() == open(os.path.join(want, name), "rb").read(), name
