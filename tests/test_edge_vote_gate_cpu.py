"""Host: the depth gate on the edge vote (ops.edge_seed ``voxel_votes`` / ``ray_claims`` / ``ray_wins`` with ``depth=``,
``seed_points`` with ``occluder`` / ``depth_maps``, the seeding tool and train.py) -- the numpy back end against per-pair
restatements bit for bit, the gate's identities on every grid, view count and width, the solids the ungated vote finds
nothing on, the ungated output unchanged, and the C ABI's rejections through the library."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import edge_seed_cases as SC
import edge_vote_gate_cases as G
from curve_gaussian_amd.ops import edge_occlusion as EO
from curve_gaussian_amd.ops import edge_seed as SD

GRIDS = pytest.mark.parametrize("dims", SC.VOTE_GRIDS, ids=lambda d: "x".join(map(str, d)))


# ------------------------------------------------------------------------------------------------ brute force
@pytest.mark.parametrize("W", [67, 33, 1])
def test_the_host_vote_equals_the_per_pair_loop_bit_for_bit(W):
    dims, V = (65, 3, 2), 3
    K, M = SC.vote_cameras(V)
    hidden_total = 0
    for kind in G.PLANES:
        depth, slack = G.plane(kind, dims, V, W)
        got = G.run_votes(dims, V, W, depth, slack, "host")
        want = G.votes_brute(dims, K, M, G.vote_bits(V, W), W, depth, slack)
        for name, a, b in zip(("seen", "hit", "hidden"), got, want):
            assert a.dtype == np.uint16 and np.array_equal(a, b), (kind, name)
        hidden_total += int(got[2].sum())
    plain = G.run_votes(dims, V, W, None, 0.0, "host")
    want = G.votes_brute(dims, K, M, G.vote_bits(V, W), W, None, 0.0)
    assert np.array_equal(plain[0], want[0]) and np.array_equal(plain[1], want[1])
    assert plain[0].sum() > 0 and hidden_total > 0, "the case sees and hides"


@pytest.mark.parametrize("kind", ["inf", "own", "mixed"])
def test_the_host_claims_and_wins_equal_their_restatement(kind):
    dims, V, W = (65, 3, 2), 3, 67
    index, support = G.listed(dims)
    depth, slack = G.plane(kind, dims, V, W)
    for window, margin in ((0, 0), (1, 0), (2, 9000)):
        best, wins = G.run_claims(dims, V, W, index, support, depth, slack, "host", window=window, margin=margin)
        want_best, want_wins = G.claims_brute(dims, V, W, index, support, depth, slack, window, margin)
        assert np.array_equal(best, want_best) and np.array_equal(wins, want_wins), (window, margin)
    assert best.max() > 0 and wins.max() > 0


# ------------------------------------------------------------------------------------------------ identities
@GRIDS
@pytest.mark.parametrize("V", SC.VOTE_VIEWS)
def test_the_gates_identities_hold_on_every_grid_view_count_and_width(dims, V):
    for W in G.WIDTHS:
        plain = G.run_votes(dims, V, W, None, 0.0, "host")
        for kind in G.PLANES:
            depth, slack = G.plane(kind, dims, V, W)
            seen, hit, hidden = G.run_votes(dims, V, W, depth, slack, "host")
            assert np.array_equal(seen.astype(np.int64) + hidden, plain[0]), ("seen + hidden is the ungated seen", kind, W)
            assert (hit <= seen).all() and (hit <= plain[1]).all(), (kind, W)
            if kind in ("inf", "nan"):   # nothing is hidden: the ungated call, exactly
                assert np.array_equal(seen, plain[0]) and np.array_equal(hit, plain[1]) and not hidden.any(), (kind, W)
            if kind == "zero":           # c2 > 0 + 0 for every kept pair
                assert not seen.any() and not hit.any() and np.array_equal(hidden, plain[0]), W
            quiet = G.run_votes(dims, V, W, depth, slack, "host", hidden=False)
            assert len(quiet) == 2 and np.array_equal(quiet[0], seen) and np.array_equal(quiet[1], hit), (kind, W)


def test_the_comparison_is_strict_at_a_centres_own_depth():
    """The voxels that own their pixel in every view that keeps them, held against their own float64 depth rounded to float32
    and the float32 steps beside it: c2 > d + 0 hides exactly when d lies below c2."""
    dims, V, W = (65, 3, 2), 3, 67
    K, M = SC.vote_cameras(V)
    c2, u, v = G.project(K, M, G.centres64(dims))
    keep = G.kept(c2, u, v, W)
    _, owner = G.own_planes(dims, V, W)
    owns = np.zeros_like(keep)
    for i in range(V):
        at = np.nonzero(keep[i])[0]
        owns[i, at] = owner[i, np.floor(v[i][at]).astype(np.int64), np.floor(u[i][at]).astype(np.int64)] == at
    sole = np.nonzero(keep.any(0) & (owns | ~keep).all(0))[0]
    assert sole.size > 20
    hidden = {kind: G.run_votes(dims, V, W, *G.plane(kind, dims, V, W), "host")[2] for kind in ("own", "own_up", "own_down")}
    with np.errstate(all="ignore"):
        below = keep & (c2 > c2.astype(np.float32).astype(np.float64))   # float32(c2) was rounded down
    assert np.array_equal(hidden["own"][sole], below.sum(0)[sole].astype(np.uint16))
    assert below[:, sole].any() and (keep & ~below)[:, sole].any(), "both roundings occur"
    assert not hidden["own_up"][sole].any() and np.array_equal(hidden["own_down"][sole], keep.sum(0)[sole].astype(np.uint16))


@GRIDS
def test_accumulating_unevenly_split_views_gives_the_counts_of_one_call(dims):
    V, W = 40, 33
    depth, slack = G.plane("mixed", dims, V, W)
    one = G.run_votes(dims, V, W, depth, slack, "host")
    for split in (1, 39, 17):
        two = G.run_votes(dims, V, W, depth, slack, "host", split=split)
        assert all(np.array_equal(a, b) for a, b in zip(one, two)), split
    assert one[2].sum() > 0 or dims == (1, 1, 1)


@GRIDS
def test_gated_claims_and_wins(dims):
    V, W = 3, 67
    index, support = G.listed(dims)
    plain = G.run_claims(dims, V, W, index, support, None, 0.0, "host")
    same = G.run_claims(dims, V, W, index, support, *G.plane("inf", dims, V, W), "host")
    assert np.array_equal(same[0], plain[0]) and np.array_equal(same[1], plain[1]), "+inf planes: the ungated claims and wins"
    best, wins = G.run_claims(dims, V, W, index, support, *G.plane("zero", dims, V, W), "host")
    assert not best.any() and not wins.any(), "hidden in every view: nothing claimed, nothing won"
    # claimed into a prefilled best, a voxel hidden everywhere leaves every word as it was
    K, M = SC.vote_cameras(V)
    filled = torch.full((V, G.HEIGHT, W), 7, dtype=torch.int32)
    out = SD.ray_claims(SC.VOTE_BOUNDS, dims, index, support, K, M, G.vote_bits(V, W), G.HEIGHT, W, best=filled, backend="host",
                        depth=G.plane("zero", dims, V, W)[0], slack=0.0)
    assert out is filled and (filled == 7).all()
    best, wins = G.run_claims(dims, V, W, index, support, *G.plane("mixed", dims, V, W), "host")
    assert (best <= plain[0]).all() and np.array_equal(
        best, G.claims_brute(dims, V, W, index, support, *G.plane("mixed", dims, V, W))[0])


def test_the_operators_check_their_new_arguments():
    dims, V, W = (65, 3, 2), 3, 33
    K, M = SC.vote_cameras(V)
    bits, (depth, _) = G.vote_bits(V, W), G.plane("mixed", dims, V, W)
    index, support = G.listed(dims)
    votes = lambda **kw: SD.voxel_votes(SC.VOTE_BOUNDS, dims, K, M, bits, G.HEIGHT, W, backend="host", **kw)
    claims = lambda **kw: SD.ray_claims(SC.VOTE_BOUNDS, dims, index, support, K, M, bits, G.HEIGHT, W, backend="host", **kw)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="voxel_votes: the slack must be finite and >= 0"):
            votes(depth=depth, slack=bad)
        with pytest.raises(ValueError, match="ray_claims: the slack must be finite and >= 0"):
            claims(depth=depth, slack=bad)
    with pytest.raises(ValueError, match=r"voxel_votes: depth must be float32 \[3,45,33\]"):
        votes(depth=depth[:2])
    with pytest.raises(ValueError, match="ray_wins: depth must be float32"):
        SD.ray_wins(SC.VOTE_BOUNDS, dims, index, support, K, M, bits, claims(), G.HEIGHT, W, backend="host",
                    depth=depth.astype(np.float64))
    with pytest.raises(ValueError, match="return_hidden needs depth"):
        votes(return_hidden=True)
    with pytest.raises(ValueError, match="counts must hold 3 tensors"):
        votes(depth=depth, return_hidden=True, counts=votes())
    # the default slack is half the voxel diagonal of the grid
    lo, hi = (np.array(b) for b in SC.VOTE_BOUNDS)
    assert SD.default_slack(SC.VOTE_BOUNDS, dims) == 0.5 * float(np.sqrt((((hi - lo) / np.array(dims)) ** 2).sum()))
    a, b = votes(depth=depth), votes(depth=depth, slack=SD.default_slack(SC.VOTE_BOUNDS, dims))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------ the scan level
@pytest.mark.parametrize("shape", ["box", "cylinder"])
def test_the_gated_vote_finds_a_solids_edges_at_the_default_ratio(shape):
    """The test that fails without the gate.  ``seed_points`` on 24 views of 240 x 320 with hidden lines removed, grid 64, every
    other default, the scan's own z-buffer as depth maps.  Host prototype of the issue: box 903 kept voxels, worst
    sample-to-kept distance 0.012; cylinder 541 and 0.017; none farther than 0.02 from the ground truth."""
    info, keep, _ = G.check_solid(shape, "host")
    assert info["kept_voxels"] == int(keep.sum()) > 0
    if shape == "box":   # (d): the same call without a depth source leaves more than half of the samples uncovered
        _, plain, _, cen, counts = G.solid_votes("box", "host")
        gt = G.ground_truth("box")
        uncovered = int((G.nearest(gt, cen) > G.COVER_RADIUS).sum())
        print(f"box, ungated: kept {plain['kept_voxels']}, uncovered {uncovered} of {len(gt)}")
        assert 2 * uncovered > len(gt), "(d) the ungated vote covers the box: the test shows nothing"
        assert len(counts) == 2 and not {"hidden_pairs", "depth_maps", "occluder", "depth_slack", "depth_window"} & set(plain)


def test_the_bracket_is_covered_and_the_claims_and_directions_run_through_the_gate():
    info, keep, _ = G.check_solid("l_bracket", "host")   # (a) only: one far voxel was seen on it
    scan = G.solid("l_bracket")
    seeds, full, keep_full, _, _ = G.solid_votes("l_bracket", "host", depth_maps=list(scan.depth), exclusive=True, directions=True)
    assert np.array_equal(keep_full, keep), "the selection before the claims is the gated vote's"
    assert 0 < full["exclusive_voxels"] <= full["kept_voxels"] == int(keep.sum())
    assert full["seeds"] == len(seeds) > 0 and full["directions"].shape == (len(seeds), 3) and full["directed"] > 0
    # the survivors' seeds lie in cells that hold a gated kept voxel
    dims, cell = full["dims"], 4
    ijk = np.stack(np.unravel_index(np.nonzero(keep)[0], dims[::-1]), 1)[:, ::-1] // cell
    cells = {tuple(c) for c in ijk.tolist()}
    lo, hi = (np.array(b, np.float64) for b in G.SOLID_BOUNDS)
    of_seed = np.floor((seeds - lo) / ((hi - lo) / np.array(dims)) / cell).astype(np.int64)
    assert all(tuple(c) in cells for c in of_seed.tolist()), "a subset of the gated kept mask"


def test_the_result_does_not_depend_on_the_chunking():
    scan = G.solid("box")
    sub = slice(0, 6)
    cams, maps, depth = scan.cameras[sub], list(scan.maps[sub]), list(scan.depth[sub])
    kw = dict(grid=32, tol_px=2, min_views=2, backend="host", exclusive=True)
    for gate in (dict(depth_maps=depth), dict(occluder=scan.tris)):
        whole = SD.seed_points(cams, maps, "PidiNet", G.SOLID_BOUNDS, **kw, **gate)
        for budget in (1, 2 * 16 * G.SOLID_H * G.SOLID_W):   # one view, and two views of the first sweep, per chunk
            cut = SD.seed_points(cams, maps, "PidiNet", G.SOLID_BOUNDS, budget_bytes=budget, **kw, **gate)
            assert np.array_equal(cut[0], whole[0]) and cut[1] == whole[1], (sorted(gate), budget)
        assert whole[1]["hidden_pairs"] > 0 and whole[1]["seeds"] > 0


# ------------------------------------------------------------------------------------------------ opt-in
def test_without_a_depth_source_the_seeds_and_info_are_the_parents():
    """tests/golden/edge_vote_ungated.npz: ``seed_points`` of the commit before the gate on the drawn scan of edge_seed_cases,
    host back end, plain and with ``exclusive`` and ``directions``."""
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "edge_vote_ungated.npz"))
    cams, maps = SC.seed_novel_cameras()
    for tag, kw in (("plain", {}), ("full", dict(exclusive=True, directions=True))):
        for extra in ({}, dict(occluder=None, depth_maps=None, depth_slack=0.5, depth_window=3)):
            seeds, info = SD.seed_points(cams, maps, "PidiNet", SC.SEED_BOUNDS, backend="host", **SC.SEED_OPTIONS, **kw, **extra)
            assert seeds.dtype == np.float64 and np.array_equal(seeds, gold[tag + "_seeds"]), tag
            if "directions" in info:
                np.testing.assert_allclose(info.pop("directions"), gold[tag + "_directions"], rtol=0, atol=1e-12)
            want = json.loads(str(gold[tag + "_info"]))
            assert json.loads(json.dumps(info)) == want and set(info) == set(want), (tag, "no new key")


def test_two_depth_sources_and_bad_parameters_are_rejected():
    scan = G.solid("box")
    args = (scan.cameras[:3], list(scan.maps[:3]), "PidiNet", G.SOLID_BOUNDS)
    with pytest.raises(ValueError, match="seed_points: give an occluder or depth_maps, not both"):
        SD.seed_points(*args, backend="host", occluder=scan.tris, depth_maps=list(scan.depth[:3]))
    with pytest.raises(ValueError, match="seed_points: the slack must be finite and >= 0"):
        SD.seed_points(*args, backend="host", occluder=scan.tris, depth_slack=-1.0)
    with pytest.raises(ValueError, match="seed_points: the window radius must lie in"):
        SD.seed_points(*args, backend="host", occluder=scan.tris, depth_window=EO.MAX_WINDOW + 1)
    with pytest.raises(ValueError, match="3 cameras and 2 depth maps"):
        SD.seed_points(*args, backend="host", depth_maps=list(scan.depth[:2]))


# ------------------------------------------------------------------------------------------------ the C ABI
def test_abi_symbols_and_argument_checks_are_pinned():
    """Status and the exact text of cgs_last_error() for the gate's rejections; the pointers are dummies that are never
    dereferenced, and no row passes validation with work to do."""
    from curve_gaussian_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(1 << 20)
    host3 = (ctypes.c_double * 3)(0.0, 0.0, 0.0), (ctypes.c_double * 3)(0.5, 0.5, 0.5)
    lo, step = (ctypes.cast(a, ctypes.c_void_p) for a in host3)

    def votes(V=2, intr=p, bits=p, depth=p, slack=0.01, acc=0, seen=p, hit=p, hidden=p, H=4):
        return lib.cgs_voxel_votes_depth(2, 2, 2, lo, step, V, intr, p, H, 6, bits, depth, slack, acc, seen, hit, hidden, None)

    def claims(M=3, V=2, index=p, depth=p, slack=0.01, best=p, H=4):
        return lib.cgs_ray_claims_depth(2, 2, 2, lo, step, M, index, p, V, p, p, H, 6, p, depth, slack, 1, best, None)

    def wins(M=3, V=2, index=p, depth=p, slack=0.01, best=p, window=1, margin=0, out=p, H=4):
        return lib.cgs_ray_wins_depth(2, 2, 2, lo, step, M, index, p, V, p, p, H, 6, p, best, depth, slack, window, margin, 0, out,
                                      None)

    for fn, call in (("cgs_voxel_votes_depth", votes), ("cgs_ray_claims_depth", claims), ("cgs_ray_wins_depth", wins)):
        rows = [(dict(depth=None), "(NULL pointer)"), (dict(slack=-1.0), "(slack=-1; the slack is finite and >= 0)"),
                (dict(slack=float("nan")), "(slack=nan; the slack is finite and >= 0)"),
                (dict(slack=float("inf")), "(slack=inf; the slack is finite and >= 0)"),
                (dict(H=16385), "(V=2, height=16385, width=6; sizes lie in [1, 16384])"),
                (dict(V=65536), "(V=65536, height=4, width=6; sizes lie in [1, 16384])")]
        for kw, text in rows:
            assert call(**kw) == -1, (fn, kw)
            assert lib.cgs_last_error().decode() == f"{fn}: invalid argument {text}", (fn, kw, lib.cgs_last_error())
    assert votes(seen=None) == -1 and votes(bits=None) == -1 and claims(index=None) == -1 and wins(out=None) == -1
    assert claims(M=-1) == -1 and lib.cgs_last_error() == b"cgs_ray_claims_depth: invalid argument (M=-1)"
    assert wins(window=5) == -1 and b"cgs_ray_wins_depth: invalid argument (window=5, margin=0" in lib.cgs_last_error()
    # V = 0 as in the siblings: the accumulating vote, the claims without a best to clear and the wins are no-ops
    assert votes(V=0, acc=1, intr=None, bits=None, depth=None) == 0
    assert claims(V=0, depth=None, best=None) == 0 and wins(V=0, depth=None) == 0 and wins(M=0, depth=None, out=None) == 0
    assert votes(V=0, acc=1, slack=-1.0) == -1, "the slack is checked before the no-op"
    i, vp, d = ctypes.c_int, ctypes.c_void_p, ctypes.c_double
    assert _lib.SIGNATURES["cgs_voxel_votes_depth"] == (i, [i, i, i, vp, vp, i, vp, vp, i, i, vp, vp, d, i, vp, vp, vp, vp])
    assert _lib.SIGNATURES["cgs_ray_claims_depth"] == (i, [i, i, i, vp, vp, i, vp, vp, i, vp, vp, i, i, vp, vp, d, i, vp, vp])
    assert _lib.SIGNATURES["cgs_ray_wins_depth"] == (i, [i, i, i, vp, vp, i, vp, vp, i, vp, vp, i, i, vp, vp, vp, d, i, i, i, vp,
                                                         vp])
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "curvegs.h")).read()
    for fn in ("cgs_voxel_votes_depth", "cgs_ray_claims_depth", "cgs_ray_wins_depth"):
        assert hasattr(lib, fn) and f"int {fn}(" in header, fn
    assert "seen + hidden is the sibling's seen" in header and "no near-plane clipping" in header


# ------------------------------------------------------------------------------------------------ the tools
def test_the_seeding_tool_takes_the_flags(tmp_path, capsys):
    from curve_gaussian_amd import edge_seed_cli as CLI
    from curve_gaussian_amd.scene import solid_scan as SS
    scan = G.solid("box")
    scan_dir = tmp_path / "box"
    SS.write_solid_scan(str(scan_dir), scan, depth=True)
    args = CLI.parser().parse_args(["--scan", "x", "--out", "y", "--occluder", "mesh.ply"])
    assert (args.occluder, args.depth_dir, args.depth_slack, args.depth_window) == ("mesh.ply", None, None, EO.DEPTH_WINDOW)
    assert not {"occluder", "depth_dir", "depth_slack", "depth_window"} & set(
        CLI.seed_options(CLI.parser().parse_args(["--scan", "x", "--out", "y", "--depth_slack", "0.5"])))
    common = ["--scan", str(scan_dir), "--detector", "PidiNet", "--backend", "host", "--grid", "64", "--bounds", "0", "0", "0",
              "1", "1", "1"]
    counts = {}
    for tag, flags in (("mesh", ["--occluder", "mesh.ply"]), ("maps", ["--depth_dir", "depth"]), ("plain", [])):
        out = tmp_path / f"{tag}.ply"
        assert CLI.main(common + flags + ["--out", str(out)]) == 0
        text = capsys.readouterr().out
        assert ("depth gate hid" in text) == (tag != "plain"), text
        header = out.read_text().split("end_header")[0]
        counts[tag] = int(header.split("element vertex")[1].split()[0])
    assert counts["mesh"] == counts["maps"] > 100 and counts["plain"] < counts["mesh"] // 4
    with pytest.raises(ValueError, match="an occluder or a depth_dir, not both"):
        CLI.main(common + ["--occluder", "mesh.ply", "--depth_dir", "depth", "--out", str(tmp_path / "no.ply")])


def test_train_puts_the_init_depth_options_into_init_options(tmp_path, capsys):
    from curve_gaussian_amd import train
    base = ["-s", str(tmp_path), "-m", str(tmp_path / "m"), "--init", "edge_votes"]
    dataset, _, _ = train.parse_args(base)
    assert not {"occluder", "depth_dir", "depth_slack", "depth_window"} & set(dataset.init_options)
    dataset, _, _ = train.parse_args(base + ["--init_occluder", "mesh.ply", "--init_depth_slack", "0.01", "--init_depth_window", "2"])
    assert dataset.init_options == {"occluder": "mesh.ply", "depth_slack": 0.01, "depth_window": 2}
    dataset, _, _ = train.parse_args(base + ["--init_depth_dir", "depth"])
    assert dataset.init_options == {"depth_dir": "depth"}
    with pytest.raises(SystemExit):
        train.parse_args(base + ["--init_occluder", "mesh.ply", "--init_depth_dir", "depth"])
    assert "takes one depth source" in capsys.readouterr().err
