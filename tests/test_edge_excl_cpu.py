"""Host: the ray-exclusive claim pass of ops.edge_seed (voxel_support, ray_claims, ray_wins, select_exclusive and
seed_points(exclusive=True)) on the numpy back end: a hand-made column, the order of the list and of the views, the ghosts
of the two drawn scans, the option's plumbing and the argument errors."""
import ctypes

import numpy as np
import pytest
import torch

import edge_dir_cases as DC
import edge_excl_cases as XC
import edge_seed_cases as SC
from curve_gaussian_amd.ops import edge_seed as SD


def _hand(columns, index, support, window=0, margin=0, best=None):
    bounds, dims = XC.hand_grid(columns)
    K, M = XC.identity_camera()
    bits = XC.ones_bits(1, XC.HAND_H, XC.HAND_W)
    if best is None:
        best = SD.ray_claims(bounds, dims, index, support, K, M, bits, XC.HAND_H, XC.HAND_W, backend="host")
    wins = SD.ray_wins(bounds, dims, index, support, K, M, bits, best, XC.HAND_H, XC.HAND_W, window=window, margin=margin,
                       backend="host")
    assert best.dtype == torch.int32 and wins.dtype == torch.uint16
    return best.numpy(), wins.numpy().tolist()


# ------------------------------------------------------------------------------------------------ the hand case
def test_one_column_on_one_pixel():
    index = [0, 1, 2, 3]
    best, wins = _hand(1, index, XC.HAND_SUPPORT)
    assert best[0, 0, 0] == 30 and best.sum() == 30, "the largest support at pixel (0, 0), 0 elsewhere"
    assert wins == [0, 1, 1, 0], "equal maxima both win"
    assert _hand(1, index, XC.HAND_SUPPORT, margin=10)[1] == [0, 1, 1, 1]
    assert _hand(1, index, XC.HAND_SUPPORT, margin=9)[1] == [0, 1, 1, 0]
    assert _hand(1, index, XC.HAND_SUPPORT, margin=65535)[1] == [1, 1, 1, 1]
    top = [65535, 1, 65535, 65534]
    assert _hand(1, index, top, margin=65535)[1] == [1, 1, 1, 1], "65535 + 65535 does not wrap"
    assert _hand(1, index, top, margin=65533)[1] == [1, 0, 1, 1]


def test_a_second_column_interacts_through_the_window_only():
    index = list(range(8))                       # voxel (i, 0, k) = 2 k + i: even = column 0, odd = column 1
    support = [10, 5, 30, 29, 30, 7, 20, 29]     # column 0: 10 30 30 20, column 1: 5 29 7 29
    best, wins = _hand(2, index, support, window=0)
    assert best[0, 0, 0] == 30 and best[0, 0, 1] == 29 and best.sum() == 59
    assert wins == [0, 0, 1, 1, 1, 0, 0, 1], "window 0: each column has its own winners"
    assert _hand(2, index, support, window=1)[1] == [0, 0, 1, 0, 1, 0, 0, 0], "window 1: column 1 loses to column 0"
    assert _hand(2, index, support, window=1, margin=1)[1] == [0, 0, 1, 1, 1, 0, 0, 1]


def test_the_window_is_clipped_at_the_image_corner():
    """The column sits on pixel (0, 0); the opposite corner (3, 2) holds a larger claim.  A window that wrapped around the
    image would see it at once; the clipped one sees it only when it reaches it."""
    best = torch.zeros((1, XC.HAND_H, XC.HAND_W), dtype=torch.int32)
    best[0, 0, 0], best[0, XC.HAND_H - 1, XC.HAND_W - 1] = 30, 65535
    for window, want in [(0, 1), (1, 1), (2, 1), (3, 0), (4, 0)]:
        assert _hand(1, [1], [30], window=window, best=best)[1] == [want], window


# ------------------------------------------------------------------------------------------------ views
def test_a_voxel_that_hits_in_no_view_wins_nothing():
    bounds, dims = XC.hand_grid(2)
    K, M = XC.identity_camera()
    mask = np.ones((1, XC.HAND_H, XC.HAND_W), bool)
    mask[0, 0, 1] = False                         # column 1 lands on a pixel that is not near
    bits = XC.mask_bits(mask)
    index, support = list(range(8)), [9] * 8
    best = SD.ray_claims(bounds, dims, index, support, K, M, bits, XC.HAND_H, XC.HAND_W, backend="host")
    assert best[0, 0, 0] == 9 and best.sum() == 9
    wins = SD.ray_wins(bounds, dims, index, support, K, M, bits, best, XC.HAND_H, XC.HAND_W, window=1, margin=65535,
                       backend="host")
    assert wins.tolist() == [1, 0] * 4
    behind = ((-0.75, -0.5, -1.35), (0.75, 0.5, -0.95)), (1, 1, 4)   # behind the camera: dropped by the projection
    best = SD.ray_claims(*behind, [0, 1], [5, 6], K, M, bits, XC.HAND_H, XC.HAND_W, backend="host")
    assert not best.numpy().any()
    assert SD.ray_wins(*behind, [0, 1], [5, 6], K, M, bits, best, XC.HAND_H, XC.HAND_W, backend="host").tolist() == [0, 0]
    none = SD.ray_wins(*behind, [0, 1], [5, 6], K[:0], M[:0], bits[:0], best[:0], XC.HAND_H, XC.HAND_W, backend="host")
    assert none.tolist() == [0, 0], "no view: nothing is won"


def test_support_is_an_integer_ratio():
    seen = torch.tensor([6, 6, 3, 65535, 65535, 0, 7], dtype=torch.uint16)
    hit = torch.tensor([6, 5, 1, 65535, 1, 0, 0], dtype=torch.uint16)
    got = SD.voxel_support(seen, hit, np.arange(7))
    assert got.dtype == torch.uint16 and got.tolist() == [65535, 54612, 21845, 65535, 1, 0, 0]
    assert SD.voxel_support(seen, hit, [4, 1]).tolist() == [1, 54612]
    assert SD.voxel_support(seen.numpy(), hit.numpy(), np.zeros(0, np.int64)).shape == (0,)


def test_select_exclusive_is_an_integer_comparison():
    hit = np.array([0, 1, 2, 3, 4, 5, 6, 6])
    wins = np.array([0, 0, 1, 1, 2, 3, 2, 3])
    need = SD.need_table(0.5, 6)
    assert need.tolist() == [0, 1, 1, 2, 2, 3, 3]
    assert SD.select_exclusive(wins, hit, 0.5).tolist() == [True, False, True, False, True, True, False, True]
    assert SD.select_exclusive(wins, hit, 0.0).all(), "ratio 0 keeps every voxel"
    assert SD.select_exclusive(wins, hit, 1.0).tolist() == [True] + [False] * 7, "ratio 1: every hit view must be won"
    assert SD.select_exclusive(hit, hit, 1.0).all()
    assert SD.select_exclusive(torch.zeros(0, dtype=torch.uint16), np.zeros(0, np.int64), 0.5).shape == (0,)


# ------------------------------------------------------------------------------------------------ order
def test_the_order_of_the_list_and_of_the_views_does_not_matter():
    dims, V = (65, 3, 2), 40
    K, M = SC.vote_cameras(V)
    bits = XC.vote_bits(V)
    index, support = XC.random_list(dims, 0.5)
    args = (K, M, bits, SC.MASK_H, SC.MASK_W)
    best = SD.ray_claims(SC.VOTE_BOUNDS, dims, index, support, *args, backend="host")
    wins = SD.ray_wins(SC.VOTE_BOUNDS, dims, index, support, *args[:3], best, *args[3:], window=1, backend="host")
    assert best.numpy().max() > 0 and 0 < wins.numpy().max() and wins.numpy().min() == 0, "the case must hold wins and losses"
    perm = np.random.default_rng(1).permutation(index.size)
    best_p = SD.ray_claims(SC.VOTE_BOUNDS, dims, index[perm], support[perm], *args, backend="host")
    wins_p = SD.ray_wins(SC.VOTE_BOUNDS, dims, index[perm], support[perm], *args[:3], best_p, *args[3:], window=1,
                         backend="host")
    assert torch.equal(best_p, best) and np.array_equal(wins_p.numpy(), wins.numpy()[perm])
    # the list claimed in two pieces into one best
    half = index.size // 2
    part = SD.ray_claims(SC.VOTE_BOUNDS, dims, index[:half], support[:half], *args, backend="host")
    both = SD.ray_claims(SC.VOTE_BOUNDS, dims, index[half:], support[half:], *args, best=part, backend="host")
    assert both is part and torch.equal(both, best)
    # the views in two accumulating calls
    cut = 13
    first = SD.ray_wins(SC.VOTE_BOUNDS, dims, index, support, K[:cut], M[:cut], bits[:cut], best[:cut], SC.MASK_H, SC.MASK_W,
                        window=1, backend="host")
    total = SD.ray_wins(SC.VOTE_BOUNDS, dims, index, support, K[cut:], M[cut:], bits[cut:], best[cut:], SC.MASK_H, SC.MASK_W,
                        window=1, counts=first, backend="host")
    assert total is first and torch.equal(total, wins)


def test_wins_never_exceed_hits_and_grow_with_the_margin():
    dims, V = (257, 2, 1), 3
    K, M = SC.vote_cameras(V)
    bits = XC.vote_bits(V)
    index, support = XC.random_list(dims, 1.0)
    _, hit = SD.voxel_votes(SC.VOTE_BOUNDS, dims, K, M, bits, SC.MASK_H, SC.MASK_W, backend="host")
    best = SD.ray_claims(SC.VOTE_BOUNDS, dims, index, support, K, M, bits, SC.MASK_H, SC.MASK_W, backend="host")
    last = None
    for window, margin in [(4, 0), (1, 0), (0, 0), (0, 1), (0, 65535)]:   # each step can only add wins
        wins = SD.ray_wins(SC.VOTE_BOUNDS, dims, index, support, K, M, bits, best, SC.MASK_H, SC.MASK_W, window=window,
                           margin=margin, backend="host").numpy().astype(int)
        assert (wins <= hit.numpy()[index]).all()
        assert last is None or (wins >= last).all()
        last = wins
    assert np.array_equal(last, hit.numpy()[index]), "with the largest margin every hit is a win: the claims use the vote's pixels"


# ------------------------------------------------------------------------------------------------ the drawn scans
def test_the_claims_suppress_the_ghosts_of_the_six_view_scan():
    """A ghost is a seed more than 3 voxels from the nearest drawn sample; coverage is the share of the samples with a seed
    within SEED_CELL + 1 voxels.  The yardstick is the plain vote on the same inputs.  Measured (host back end, the
    defaults window 1, margin 0, win_ratio 0.5): the plain vote keeps 3177 voxels and gives 664 seeds, 219 of them ghosts,
    coverage 1.0; with the claims 2002 voxels remain and give 441 seeds, 33 of them ghosts (7.5 %), coverage 1.0 -- the
    counts of the prototype this pass was proposed with."""
    samples, voxel = SC.seed_points_sampled(), 1.0 / SC.SEED_GRID
    plain, plain_info = XC.six_view_seeds(False)
    seeds, info = XC.six_view_seeds(True)
    ghosts_plain, cover_plain = XC.ghosts_and_coverage(plain, samples, voxel, SC.SEED_CELL)
    ghosts, cover = XC.ghosts_and_coverage(seeds, samples, voxel, SC.SEED_CELL)
    print(f"plain: kept {plain_info['kept_voxels']}, seeds {len(plain)}, ghosts {ghosts_plain}, coverage {cover_plain:.4f}; "
          f"exclusive: voxels {info['exclusive_voxels']}, seeds {len(seeds)}, ghosts {ghosts}, coverage {cover:.4f}")
    assert ghosts_plain > 100, "the plain vote of six views has ghosts"
    assert 2 * ghosts <= ghosts_plain, "at most half of them are left"
    assert cover >= cover_plain, "no drawn sample loses its seed"
    assert info["kept_voxels"] == plain_info["kept_voxels"] and 0 < info["exclusive_voxels"] < info["kept_voxels"]
    assert info["seeds"] == len(seeds) == info["cells"] < len(plain)


def test_the_claims_keep_the_twelve_view_scan_covered_and_directed():
    """The twelve-view scan has no ghosts to begin with; the pass thins its tubes.  Measured: 901 kept voxels, 271 seeds, 267
    directed without the option; 541 voxels, 197 seeds, 196 directed with it; coverage 1.0 both times, no ghost either way."""
    samples, voxel, cell = DC.dir_samples()[0], 1.0 / DC.DIR_OPTIONS["grid"], DC.DIR_OPTIONS["cell"]
    plain, plain_info = XC.twelve_view_seeds(False)
    seeds, info = XC.twelve_view_seeds(True)
    ghosts_plain, cover_plain = XC.ghosts_and_coverage(plain, samples, voxel, cell)
    ghosts, cover = XC.ghosts_and_coverage(seeds, samples, voxel, cell)
    print(f"plain: kept {plain_info['kept_voxels']}, seeds {len(plain)}, directed {plain_info['directed']}, ghosts "
          f"{ghosts_plain}, coverage {cover_plain:.4f}; exclusive: voxels {info['exclusive_voxels']}, seeds {len(seeds)}, "
          f"directed {info['directed']}, ghosts {ghosts}, coverage {cover:.4f}")
    assert cover == cover_plain, "coverage is unchanged"
    assert ghosts <= ghosts_plain
    assert 2 * info["directed"] >= plain_info["directed"] > 0, "at least half as many directed seeds"
    assert info["directions"].shape == seeds.shape and info["exclusive_voxels"] < info["kept_voxels"]


def test_the_option_off_changes_nothing():
    cams, maps = SC.seed_novel_cameras()
    seeds, info = SD.seed_points(cams, maps, "PidiNet", SC.SEED_BOUNDS, backend="host", **SC.SEED_OPTIONS)
    off, off_info = XC.six_view_seeds(False)
    assert sorted(info) == ["backend", "capped", "cells", "dims", "kept_voxels", "seeds", "views", "voxels"]
    assert info == off_info and np.array_equal(seeds, off)
    on, on_info = XC.six_view_seeds(True)
    assert sorted(set(on_info) - set(info)) == ["exclusive_voxels"]
    # ratio 0 keeps every voxel: the pass runs and changes nothing but the new key
    same, same_info = SD.seed_points(cams, maps, "PidiNet", SC.SEED_BOUNDS, backend="host", exclusive=True, excl_win_ratio=0.0,
                                     **SC.SEED_OPTIONS)
    assert np.array_equal(same, seeds) and same_info == dict(info, exclusive_voxels=info["kept_voxels"])


def test_chunking_the_second_sweep_changes_nothing():
    cams, maps = SC.seed_novel_cameras()
    whole, info = XC.six_view_seeds(True)
    budget = 2 * SD.BYTES_PER_PIXEL * SC.SEED_H * SC.SEED_W   # two views at a time in the first sweep, four in the second
    parts, info_p = SD.seed_points(cams, maps, "PidiNet", SC.SEED_BOUNDS, backend="host", exclusive=True, budget_bytes=budget,
                                   **SC.SEED_OPTIONS)
    assert np.array_equal(parts, whole) and info_p == info
    one, info_1 = SD.seed_points(cams, maps, "PidiNet", SC.SEED_BOUNDS, backend="host", exclusive=True, budget_bytes=1,
                                 **SC.SEED_OPTIONS)
    assert np.array_equal(one, whole) and info_1 == info, "one view at a time"
    kw = dict(backend="host", exclusive=True, directions=True, **SC.SEED_OPTIONS)   # and with the directions on top
    whole_d, info_d = SD.seed_points(cams, maps, "PidiNet", SC.SEED_BOUNDS, **kw)
    one_d, info_1d = SD.seed_points(cams, maps, "PidiNet", SC.SEED_BOUNDS, budget_bytes=1, **kw)
    assert np.array_equal(whole_d, whole) and np.array_equal(one_d, whole) and XC.same_info(info_1d, info_d)
    assert info_d["directions"].shape == (len(whole), 3) and {k: info_d[k] for k in info} == info
    assert SD.EXCL_BYTES_PER_PIXEL == 4 and SD.BYTES_PER_PIXEL == 8


# ------------------------------------------------------------------------------------------------ plumbing
def test_scene_cloud_and_cli_carry_the_option(tmp_path, capsys):
    from curve_gaussian_amd import edge_seed_cli as CLI
    from curve_gaussian_amd.scene import dataset_io as IO
    scan = SC.write_seed_scan(tmp_path, "emap", detector="PidiNet")
    cams = IO.read_emap(scan, detector="PidiNet")
    cloud = IO.edge_vote_point_cloud(cams, "PidiNet", IO.default_seed_bounds("emap"), exclusive=True, backend="host",
                                     **SC.SEED_OPTIONS)
    seeds, info = CLI.seed_scan(scan, "emap", "PidiNet", backend="host", exclusive=True, **SC.SEED_OPTIONS)
    assert np.array_equal(cloud.points, seeds) and len(seeds) == info["seeds"]
    assert info["exclusive_voxels"] < info["kept_voxels"]
    out = tmp_path / "seeds.ply"
    argv = ["--scan", scan, "--detector", "PidiNet", "--backend", "host", "--out", str(out), "--grid", str(SC.SEED_GRID),
            "--tol_px", str(SC.SEED_TOL_PX), "--cell", str(SC.SEED_CELL)]
    assert CLI.main(argv + ["--exclusive"]) == 0
    assert f"after the claims {info['exclusive_voxels']} voxels" in capsys.readouterr().out
    assert CLI.main(argv) == 0
    assert "after the claims" not in capsys.readouterr().out


def test_the_command_lines_parse_the_options():
    from curve_gaussian_amd import edge_seed_cli as CLI
    from curve_gaussian_amd import train as T
    dataset, _, _ = T.parse_args(["-s", "scan", "-m", "out", "--init", "edge_votes", "--init_exclusive", "--init_excl_window", "2",
                                  "--init_excl_margin", "300", "--init_excl_win_ratio", "0.75"])
    assert dataset.init_options == {"exclusive": True, "excl_window": 2, "excl_margin": 300, "excl_win_ratio": 0.75}
    dataset, _, _ = T.parse_args(["-s", "scan", "-m", "out", "--init", "edge_votes", "--init_exclusive"])
    assert dataset.init_options == {"exclusive": True}
    assert T.parse_args(["-s", "scan", "-m", "out", "--init", "edge_votes"])[0].init_options == {}
    args = CLI.parser().parse_args(["--scan", "s", "--out", "o.ply", "--exclusive", "--excl_window", "3", "--excl_margin", "7",
                                    "--excl_win_ratio", "0.25"])
    opts = CLI.seed_options(args)
    assert (opts["exclusive"], opts["excl_window"], opts["excl_margin"], opts["excl_win_ratio"]) == (True, 3, 7, 0.25)
    opts = CLI.seed_options(CLI.parser().parse_args(["--scan", "s", "--out", "o.ply"]))
    assert (opts["exclusive"], opts["excl_window"], opts["excl_margin"], opts["excl_win_ratio"]) == \
        (False, SD.EXCL_WINDOW, SD.EXCL_MARGIN, SD.EXCL_WIN_RATIO) == (False, 1, 0, 0.5)
    import inspect
    assert set(opts) <= set(inspect.signature(SD.seed_points).parameters)


# ------------------------------------------------------------------------------------------------ argument errors
def test_argument_errors():
    bounds, dims = XC.hand_grid(1)
    K, M = XC.identity_camera()
    H, W = XC.HAND_H, XC.HAND_W
    bits = XC.ones_bits(1, H, W)
    best = torch.zeros((1, H, W), dtype=torch.int32)
    claims = lambda index=(0, 1), support=(5, 6), bits=bits, **kw: SD.ray_claims(
        bounds, dims, list(index), list(support), K, M, bits, H, W, **{"backend": "host", **kw})
    wins = lambda index=(0, 1), support=(5, 6), bits=bits, best=best, **kw: SD.ray_wins(
        bounds, dims, list(index), list(support), K, M, bits, best, H, W, **{"backend": "host", **kw})
    for call in (claims, wins):
        with pytest.raises(ValueError, match="outside"):
            call(index=(0, 4))
        with pytest.raises(ValueError, match="outside"):
            call(index=(-1, 0))
        with pytest.raises(ValueError, match="support"):
            call(support=(5,))
        with pytest.raises(ValueError, match="support"):
            call(support=(5, 65536))
        with pytest.raises(ValueError, match="bits"):
            call(bits=bits[:, :, :0])
        with pytest.raises(ValueError, match="backend"):
            call(backend="cuda")
    with pytest.raises(ValueError, match="integer"):
        SD.ray_claims(bounds, dims, np.array([0.0, 1.0]), [5, 6], K, M, bits, H, W, backend="host")
    with pytest.raises(ValueError, match="best"):
        claims(best=torch.zeros((1, H, W), dtype=torch.int64))
    with pytest.raises(ValueError, match="best"):
        wins(best=torch.zeros((1, H, W + 1), dtype=torch.int32))
    for bad in (-1, 5, 1.5):
        with pytest.raises(ValueError, match="window"):
            wins(window=bad)
    for bad in (-1, 65536, 0.5):
        with pytest.raises(ValueError, match="margin"):
            wins(margin=bad)
    with pytest.raises(ValueError, match="counts"):
        wins(counts=torch.zeros(3, dtype=torch.uint16))
    with pytest.raises(ValueError, match="counts"):
        wins(counts=torch.zeros(2, dtype=torch.int32))
    assert claims(index=(), support=()).shape == (1, H, W) and wins(index=(), support=()).shape == (0,)
    seen, hit = np.array([3, 3, 0]), np.array([2, 3, 0])
    with pytest.raises(ValueError, match="outside"):
        SD.voxel_support(seen, hit, [3])
    with pytest.raises(ValueError, match="shape"):
        SD.voxel_support(seen, hit[:2], [0])
    with pytest.raises(ValueError, match="hit"):
        SD.voxel_support(seen, np.array([4, 3, 0]), [0])
    with pytest.raises(ValueError, match="shape"):
        SD.select_exclusive(np.zeros(2, np.int64), np.zeros(3, np.int64), 0.5)
    for bad in (-0.1, 1.1):
        with pytest.raises(ValueError, match="win_ratio"):
            SD.select_exclusive(np.zeros(2, np.int64), np.zeros(2, np.int64), bad)
    cams, maps = SC.seed_novel_cameras()
    for kw, word in [(dict(excl_window=5), "excl_window"), (dict(excl_margin=-1), "excl_margin"),
                     (dict(excl_margin=65536), "excl_margin"), (dict(excl_win_ratio=1.5), "excl_win_ratio")]:
        with pytest.raises(ValueError, match=word):
            SD.seed_points(cams, maps, "PidiNet", SC.SEED_BOUNDS, backend="host", exclusive=True, **kw, **SC.SEED_OPTIONS)
    # without the option its values are not looked at, as dir_radius is not without directions
    SD.seed_points(cams[:1], maps[:1], "PidiNet", SC.SEED_BOUNDS, backend="host", excl_window=9, grid=4)


def test_abi_rejections_without_a_gpu():
    from curve_gaussian_amd import _lib
    lib = _lib.load()
    assert _lib.SEED_MAX_WINDOW == SD.SEED_MAX_WINDOW == 4
    p = ctypes.c_void_p(64)   # never dereferenced: every call below is rejected before anything is launched
    lo, step = (ctypes.c_double * 3)(0.0, 0.0, 0.0), (ctypes.c_double * 3)(1.0, 1.0, 1.0)
    ptr = lambda a: ctypes.cast(a, ctypes.c_void_p)

    def claims(nx=2, ny=2, nz=2, lo=ptr(lo), step=ptr(step), M=1, index=p, support=p, V=1, intr=p, w2c=p, H=4, W=4, bits=p,
               clear=0, best=p):
        return lib.cgs_ray_claims(nx, ny, nz, lo, step, M, index, support, V, intr, w2c, H, W, bits, clear, best, None)

    def wins(nx=2, ny=2, nz=2, lo=ptr(lo), step=ptr(step), M=1, index=p, support=p, V=1, intr=p, w2c=p, H=4, W=4, bits=p,
             best=p, window=1, margin=0, accumulate=0, out=p):
        return lib.cgs_ray_wins(nx, ny, nz, lo, step, M, index, support, V, intr, w2c, H, W, bits, best, window, margin,
                                accumulate, out, None)

    nan, neg = (ctypes.c_double * 3)(0.0, float("nan"), 0.0), (ctypes.c_double * 3)(1.0, 1.0, -1.0)
    shared = [dict(M=-1), dict(V=-1), dict(V=65536), dict(nx=0), dict(ny=-1), dict(nz=0), dict(nx=2048, ny=2048, nz=512),
              dict(nx=65536, ny=65536, nz=1), dict(H=0), dict(W=16385), dict(lo=None), dict(step=None), dict(lo=ptr(nan)),
              dict(step=ptr(neg)), dict(index=None), dict(support=None), dict(intr=None), dict(w2c=None), dict(bits=None),
              dict(best=None)]
    for kw in shared:
        assert claims(**kw) == -1 and b"cgs_ray_claims: invalid argument" in lib.cgs_last_error(), kw
        assert wins(**kw) == -1 and b"cgs_ray_wins: invalid argument" in lib.cgs_last_error(), kw
    for kw in [dict(window=-1), dict(window=5), dict(margin=-1), dict(margin=65536), dict(out=None)]:
        assert wins(**kw) == -1 and b"cgs_ray_wins: invalid argument" in lib.cgs_last_error(), kw
    for kw in [dict(M=0), dict(V=0), dict(M=0, V=0, index=None, support=None, intr=None, w2c=None, bits=None, best=None)]:
        assert claims(**kw) == 0, "no voxel or no view is a no-op without a clear"
        assert wins(**kw) == 0
    assert wins(M=0, out=None) == 0 and claims(V=0, clear=1, best=None) == 0, "no view leaves nothing to clear"
