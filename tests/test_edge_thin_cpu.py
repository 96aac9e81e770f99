"""Host: the Guo-Hall thinning of ops.edge_thin on the numpy back end -- against a brute force in Python integers, its
properties, how far it erodes the drawn scan's dilated masks, what it does to the support check and the reprojection score
on thick responses, the ``thin`` option's defaults and command lines, and the C ABI's argument checks."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import edge_dir_cases as DC
import edge_score_cases as EC
import edge_seed_cases as SC
import edge_support_cases as SPC
import edge_thin_cases as C
from curve_gaussian_amd.edge_extraction import reprojection as RP
from curve_gaussian_amd.ops import edge_score as ES
from curve_gaussian_amd.ops import edge_seed as SD
from curve_gaussian_amd.ops import edge_support as SP
from curve_gaussian_amd.ops import edge_thin as ET

SPECIAL = C.special_masks()


def _host(mask, **kw):
    out, n = ET.thin_masks(np.asarray(mask)[None], backend="host", return_iterations=True, **kw)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (1,) + np.asarray(mask).shape
    return out[0].numpy(), n


def _check_properties(mask, out):
    assert set(np.unique(out)) <= {0, 1}
    assert not (out & ~(mask != 0)).any(), "the output is a subset of the input"
    again, n = _host(out)
    assert np.array_equal(again, out) and n == 1, "a thinned mask is a fixed point: one iteration that changes nothing"


# ------------------------------------------------------------------------------------------------ against the brute force
@pytest.mark.parametrize("density", C.DENSITIES)
def test_host_equals_the_brute_force_on_random_masks(density):
    thinned = 0
    for shape in C.SMALL_SHAPES:
        mask = C.random_mask(shape, density)
        keep = mask.copy()
        want, want_n = C.thin_brute(mask)
        got, got_n = _host(mask)
        assert np.array_equal(got, want) and got_n == want_n, shape
        assert np.array_equal(mask, keep), "the input is not modified"
        _check_properties(mask, got)
        thinned += int(mask.sum() - got.sum())
        for n in (1, 2, 3):
            want, want_n = C.thin_brute(mask, n)
            got, got_n = _host(mask, max_iterations=n)
            assert np.array_equal(got, want) and got_n == want_n and got_n <= n, (shape, n)
    assert thinned > 0, "the cases must hold pixels to clear"


@pytest.mark.parametrize("name, mask", SPECIAL, ids=[n for n, _ in SPECIAL])
def test_host_equals_the_brute_force_on_the_hand_cases(name, mask):
    want, want_n = C.thin_brute(mask)
    got, got_n = _host(mask)
    assert np.array_equal(got, want) and got_n == want_n
    _check_properties(mask, got)
    if name.startswith(("zeros", "pixel", "border_top", "border_bottom", "border_left", "border_right")) \
            or name in ("horizontal1", "vertical1"):
        assert np.array_equal(got, mask) and got_n == 1, "a one-pixel line is already thin"
    if name.startswith("ones") and mask.size > 1:
        assert 0 < got.sum() < mask.sum()
    if name[:-1] in ("horizontal", "vertical", "diagonal", "antidiagonal"):
        assert got.sum() > 0, "a stroke is never thinned away"


def test_nonzero_bytes_count_as_set_and_bool_masks_are_taken():
    mask = C.random_mask((17, 33), 0.6)
    want = _host(mask)[0]
    loud = mask * np.random.default_rng(0).integers(1, 256, mask.shape).astype(np.uint8)
    assert loud.max() > 1 and np.array_equal(loud != 0, mask != 0)
    keep = loud.copy()
    assert np.array_equal(_host(loud)[0], want) and np.array_equal(loud, keep)
    assert np.array_equal(ET.thin_masks(torch.from_numpy(mask.astype(bool))[None], backend="host")[0].numpy(), want)
    t = torch.from_numpy(loud.copy())[None]
    assert np.array_equal(ET.thin_masks(t, backend="host")[0].numpy(), want) and np.array_equal(t[0].numpy(), keep)


def test_a_stack_counts_the_view_that_settles_last():
    pixel = np.zeros((33, 33), np.uint8)
    pixel[5, 7] = 1
    views = [np.zeros((33, 33), np.uint8), pixel, C.disc((33, 33), (16, 16), 12)]
    counts = [_host(v)[1] for v in views]
    assert counts[0] == counts[1] == 1 < counts[2]
    out, n = ET.thin_masks(np.stack(views), backend="host", return_iterations=True)
    assert n == max(counts)
    for v, view in enumerate(views):
        assert np.array_equal(out[v].numpy(), _host(view)[0])
    empty, n0 = ET.thin_masks(np.zeros((0, 4, 5), np.uint8), backend="host", return_iterations=True)
    assert tuple(empty.shape) == (0, 4, 5) and n0 == 0


def test_argument_errors():
    with pytest.raises(ValueError, match="backend"):
        ET.thin_masks(np.zeros((1, 2, 2), np.uint8), backend="cuda")
    with pytest.raises(ValueError, match="max_iterations"):
        ET.thin_masks(np.zeros((1, 2, 2), np.uint8), backend="host", max_iterations=-1)
    with pytest.raises(ValueError, match=r"\[V,H,W\]"):
        ET.thin_masks(np.zeros((2, 2), np.uint8), backend="host")
    with pytest.raises(ValueError, match=r"\[V,H,W\]"):
        ET.thin_masks(np.zeros((1, 2, 2), np.float32), backend="host")
    with pytest.raises(ValueError, match=r"\[1, 16384\]"):
        ET.thin_masks(np.zeros((1, 1, 16385), np.uint8), backend="host")
    if not torch.cuda.is_available():
        from curve_gaussian_amd import _lib
        with pytest.raises(_lib.CurveGSError, match="needs a GPU"):
            ET.thin_masks(np.zeros((1, 2, 2), np.uint8), backend="gpu")


# ------------------------------------------------------------------------------------------------ the drawn scan, dilated
@pytest.mark.parametrize("r", [0, 1, 2])
def test_the_erosion_cap_on_the_dilated_drawn_scan(r):
    """Every pixel of the response dilated by r lies within d^2 <= (2r + 3)^2 of a thinned pixel.  Measured (host): the
    furthest lies at d^2 = 2, 13, 41 for r = 0, 1, 2 (caps 9, 25, 49) after 3, 5, 7 iterations; Zhang-Suen, which eats
    two-pixel diagonal strokes from their ends, gives 265, 313, 365."""
    thick = C.scan_masks(r)
    thin, n = ET.thin_masks(thick, backend="host", return_iterations=True)
    d2 = ES.edt_squared(thin, backend="host").numpy()
    worst = int(d2[thick != 0].max())
    print(f"r = {r}: {n} iterations, {int(thick.sum())} -> {int(thin.sum())} pixels, furthest response pixel d^2 = {worst}")
    assert worst <= (2 * r + 3) ** 2
    assert not (thin.numpy() & ~thick).any() and thin.numpy().any(axis=(1, 2)).all()


def _support(r, thin=None, backend="host", budget_bytes=None):
    cams, maps = C.thick_scan(r)
    kw = {} if thin is None else {"thin": thin}
    return SP.edge_support(SPC.scan_edges()[0], cams, maps, "PidiNet", resolution=EC.SCAN_RESOLUTION, keep_tolerance_px=2,
                           min_visible=0.5, min_near=0.8, frames_ratio=SPC.SCAN_FRAMES_RATIO, backend=backend,
                           budget_bytes=budget_bytes, **kw)


@pytest.mark.parametrize("r", [1, 2])
def test_thinning_restores_the_support_check_on_a_thick_response(r):
    """The scan and edges of edge_support_cases, masks dilated by r, at the support check's test settings (2 px, min_near
    0.8, more than 6 of 12 views).  Measured (host): as they are the thick maps keep 3 (r = 1) and 11 (r = 2) of the 72
    bogus chords; thinned, none: a bogus edge is supported by at most 5 and 6 views -- 6 is the verdict's own threshold,
    not a margin -- and every drawn edge by 12 of 12."""
    drawn = SPC.scan_edges()[1]
    thick, thin = _support(r, thin=False), _support(r, thin=True)
    t = thin["settings"]["tolerances_px"].index(2.0)
    print(f"r = {r}: bogus kept {int(thick['kept'][~drawn].sum())} -> {int(thin['kept'][~drawn].sum())}; thinned: bogus "
          f"supported by at most {int(thin['supporting_views'][~drawn, t].max())} views, drawn by "
          f"{thin['supporting_views'][drawn, t].tolist()}")
    assert thick["kept"][~drawn].sum() >= 1, "a thick response keeps bogus chords"
    assert thick["kept"][drawn].all()
    assert np.array_equal(thin["kept"], drawn), "thinned: exactly the four drawn edges are kept"
    assert (thin["supporting_views"][~drawn, t] <= 6).all()
    assert (thin["supporting_views"][drawn, t] == DC.DIR_VIEWS).all()
    assert thin["settings"]["thin"] is True and "thin" not in thick["settings"]


def test_thinning_a_thin_scan_leaves_the_verdict():
    plain, thin = _support(0, thin=False), _support(0, thin=True)
    assert np.array_equal(plain["kept"], thin["kept"]) and np.array_equal(thin["kept"], SPC.scan_edges()[1])
    assert np.array_equal(plain["seeing_views"], thin["seeing_views"]), "what a view sees does not depend on its mask"


def test_thinning_restores_the_recall_of_the_reprojection_score():
    """score_edges of the drawn edges on the masks dilated by r = 2, at 2 px.  Measured (host): recall 0.755 thick, 0.998
    thinned; precision 1.000 thick, 0.984 thinned."""
    cams, maps = C.thick_scan(2)
    kw = dict(sample_resolution=EC.SCAN_RESOLUTION, backend="host")
    thick = RP.score_edges(EC.SCAN_EDGES, cams, maps, "PidiNet", **kw, thin=False)
    thin = RP.score_edges(EC.SCAN_EDGES, cams, maps, "PidiNet", **kw, thin=True)
    t = thin["aggregate"]["tolerances_px"].index(2.0)
    print(f"recall at 2 px {thick['aggregate']['recall'][t]:.4f} -> {thin['aggregate']['recall'][t]:.4f}, precision "
          f"{thick['aggregate']['precision'][t]:.4f} -> {thin['aggregate']['precision'][t]:.4f}")
    assert thin["aggregate"]["recall"][t] > thick["aggregate"]["recall"][t] + 0.2
    assert thin["aggregate"]["precision"][t] >= 0.95
    assert thin["settings"]["thin"] is True and "thin" not in thick["settings"]


# ------------------------------------------------------------------------------------------------ defaults
def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if torch.is_tensor(a):
        return torch.is_tensor(b) and torch.equal(a, b)
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, float) and a != a:
        return isinstance(b, float) and b != b
    return type(a) is type(b) and a == b


def test_the_option_is_off_by_default_and_adds_nothing_then():
    absent, off = _support(1), _support(1, thin=False)
    assert _same(absent, off) and "thin" not in absent["settings"]
    cams, maps = C.thick_scan(1)
    kw = dict(sample_resolution=EC.SCAN_RESOLUTION, backend="host")
    absent, off = RP.score_edges(EC.SCAN_EDGES, cams, maps, "PidiNet", **kw), RP.score_edges(EC.SCAN_EDGES, cams, maps,
                                                                                             "PidiNet", thin=False, **kw)
    assert _same(absent, off) and "thin" not in absent["settings"]
    kw = dict(backend="host", **DC.DIR_OPTIONS)
    (s0, i0), (s1, i1) = SD.seed_points(cams, maps, "PidiNet", DC.DIR_BOUNDS, **kw), SD.seed_points(
        cams, maps, "PidiNet", DC.DIR_BOUNDS, thin=False, **kw)
    assert np.array_equal(s0, s1) and _same(i0, i1) and "thin" not in i0
    s2, i2 = SD.seed_points(cams, maps, "PidiNet", DC.DIR_BOUNDS, thin=True, **kw)
    assert i2["thin"] is True and {k: v for k, v in i2.items() if k != "thin"}.keys() == i0.keys()
    assert 0 < i2["kept_voxels"] < i0["kept_voxels"], "a thinned response narrows the band of voxels that vote"


# ------------------------------------------------------------------------------------------------ command lines
def test_the_support_and_score_command_lines_write_the_setting(tmp_path):
    from curve_gaussian_amd.edge_extraction import support as S
    base, data = SPC.write_support_scan(tmp_path)
    argv = ["--base_dir", base, "--dataset_dir", data, "--detector", "PidiNet", "--backend", "host"]
    support = argv + ["--frames_ratio", "0.5", "--sample_resolution", str(EC.SCAN_RESOLUTION)]
    assert S.main(support) == 0
    plain = json.load(open(os.path.join(base, "room", S.SUPPORT_FILE)))
    assert S.main(support + ["--thin"]) == 0
    thin = json.load(open(os.path.join(base, "room", S.SUPPORT_FILE)))
    assert "thin" not in plain["settings"] and thin["settings"]["thin"] is True
    assert {k: v for k, v in thin["settings"].items() if k != "thin"} == plain["settings"]
    assert [e["kept"] for e in thin["edges"]] == [e["kept"] for e in plain["edges"]] == SPC.scan_edges()[1].tolist()
    assert RP.main(argv) == 0
    plain = json.load(open(os.path.join(base, "room", RP.SCORE_FILE)))
    assert RP.main(argv + ["--thin"]) == 0
    thin = json.load(open(os.path.join(base, "room", RP.SCORE_FILE)))
    assert "thin" not in plain["settings"] and thin["settings"]["thin"] is True
    assert {k: v for k, v in thin["settings"].items() if k != "thin"} == plain["settings"]


def test_the_seed_command_line_takes_the_flag(tmp_path, capsys):
    from curve_gaussian_amd import edge_seed_cli as CLI
    scan = SC.write_seed_scan(tmp_path, "emap", detector="PidiNet")
    _, plain = CLI.seed_scan(scan, "emap", "PidiNet", backend="host", **SC.SEED_OPTIONS)
    _, thin = CLI.seed_scan(scan, "emap", "PidiNet", backend="host", thin=True, **SC.SEED_OPTIONS)
    assert "thin" not in plain and thin["thin"] is True and thin["seeds"] > 0
    argv = ["--scan", scan, "--detector", "PidiNet", "--backend", "host", "--out", str(tmp_path / "seeds.ply"), "--grid",
            str(SC.SEED_GRID), "--tol_px", str(SC.SEED_TOL_PX), "--cell", str(SC.SEED_CELL)]
    assert CLI.main(argv + ["--thin"]) == 0
    assert f"seeds {thin['seeds']}" in capsys.readouterr().out
    assert CLI.main(argv) == 0
    assert f"seeds {plain['seeds']}" in capsys.readouterr().out
    assert "thin" not in CLI.seed_options(CLI.parser().parse_args(["--scan", "s", "--out", "o.ply"]))
    assert CLI.seed_options(CLI.parser().parse_args(["--scan", "s", "--out", "o.ply", "--thin"]))["thin"] is True


def test_the_driver_passes_the_flag_to_its_three_users(tmp_path):
    from curve_gaussian_amd import train as T
    from curve_gaussian_amd.edge_extraction import support as S
    from curve_gaussian_amd.scene import dataset_io as IO
    dataset, _, args = T.parse_args(["-s", "scan", "-m", "out", "--init", "edge_votes", "--thin_edge_maps"])
    assert args.thin_edge_maps and dataset.init_options == {"thin": True} and T.support_options(args) == {"thin": True}
    dataset, _, args = T.parse_args(["-s", "scan", "-m", "out", "--init", "edge_votes"])
    assert not args.thin_edge_maps and dataset.init_options == {} and T.support_options(args) == {}
    # what the driver then calls, on the cameras of a scene: the scene's score, its support check and its seed cloud
    base, data = SPC.write_support_scan(tmp_path)
    cams = IO.read_emap(os.path.join(data, "room"), detector="PidiNet")

    class FakeScene:
        def getTrainCameras(self):
            return cams

        def getTestCameras(self):
            return []
    model = os.path.join(base, "room")
    out = RP.score_scene(model, FakeScene(), "PidiNet", sample_resolution=EC.SCAN_RESOLUTION, backend="host", thin=True)
    assert out["train"]["settings"]["thin"] is True
    assert json.load(open(os.path.join(model, RP.SCORE_FILE)))["train"]["settings"]["thin"] is True
    S.support_scene(model, SPC.scan_edges()[0], cams, None, "PidiNet", resolution=EC.SCAN_RESOLUTION, frames_ratio=0.5,
                    backend="host", thin=True)
    assert json.load(open(os.path.join(model, S.SUPPORT_FILE)))["settings"]["thin"] is True
    cloud = IO.edge_vote_point_cloud(cams, "PidiNet", DC.DIR_BOUNDS, backend="host", thin=True, **DC.DIR_OPTIONS)
    assert len(cloud.points) > 0


# ------------------------------------------------------------------------------------------------ the C ABI
def test_abi_rejections_without_a_gpu():
    from curve_gaussian_amd import _lib
    lib = _lib.load()
    assert (_lib.THIN_TILE_HEIGHT, _lib.THIN_TILE_WIDTH, _lib.THIN_PASS_ITERATIONS) == (ET.TILE_HEIGHT, ET.TILE_WIDTH,
                                                                                        ET.PASS_ITERATIONS)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "curvegs.h")).read()
    for name, value in (("CGS_THIN_TILE_HEIGHT", ET.TILE_HEIGHT), ("CGS_THIN_TILE_WIDTH", ET.TILE_WIDTH),
                        ("CGS_THIN_PASS_ITERATIONS", ET.PASS_ITERATIONS)):
        assert f"#define {name} {value}\n" in header
    p = ctypes.c_void_p(64)   # never dereferenced: every call below is rejected before anything is launched
    n = ctypes.c_int(-7)

    def call(V=2, H=4, W=5, masks=p, scratch=p, flag=p, max_iterations=0, iterations=None):
        return lib.cgs_thin_masks(V, H, W, masks, scratch, flag, max_iterations, iterations, None)

    for kw in [dict(V=-1), dict(H=0), dict(H=-2), dict(H=16385), dict(W=0), dict(W=16385), dict(max_iterations=-1),
               dict(masks=None), dict(scratch=None), dict(flag=None), dict(V=0, W=0), dict(V=0, max_iterations=-1)]:
        assert call(**kw) == -1 and b"cgs_thin_masks: invalid argument" in lib.cgs_last_error(), kw
    assert call(H=16385) == -1 and b"height=16385" in lib.cgs_last_error()
    assert call(max_iterations=-3) == -1 and b"max_iterations=-3" in lib.cgs_last_error()
    assert call(flag=None) == -1 and b"NULL pointer" in lib.cgs_last_error()
    assert call(V=0) == 0 and call(V=0, masks=None, scratch=None, flag=None) == 0, "no view leaves nothing to thin"
    assert call(V=0, iterations=ctypes.byref(n)) == 0 and n.value == 0
