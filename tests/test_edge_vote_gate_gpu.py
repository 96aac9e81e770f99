"""GPU: cgs_voxel_votes_depth / cgs_ray_claims_depth / cgs_ray_wins_depth against the host back end, bit for bit -- every grid,
view count and width of edge_seed_cases under depth planes that reach every branch of the gate, accumulation over unevenly
split views, listed voxels outside the grid, the ungated kernels under +inf planes -- and the solids the ungated vote finds
nothing on, with the two back ends' votes and selections equal."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import edge_seed_cases as SC
import edge_vote_gate_cases as G
from curve_gaussian_amd.ops import edge_seed as SD

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GRIDS = pytest.mark.parametrize("dims", SC.VOTE_GRIDS, ids=lambda d: "x".join(map(str, d)))


def _words(n, dtype=np.uint16):
    return torch.from_numpy(np.full(n, G.SENTINEL, dtype)).to(DEV)


class _Raw:
    """The raw C calls on device copies of one case."""

    def __init__(self, dims, V, W, depth, slack):
        from curve_gaussian_amd import _lib as L
        self.L, self.lib = L, L.load()
        lo, hi = (np.asarray(b, np.float64) for b in SC.VOTE_BOUNDS)
        self.host = (ctypes.c_double * 3)(*lo), (ctypes.c_double * 3)(*((hi - lo) / np.array(dims, np.float64)))
        K, M = SC.vote_cameras(V)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        self.K, self.M, self.bits = dev(np.asarray(K, np.float64)), dev(np.asarray(M, np.float64).reshape(-1, 12)), G.vote_bits(V, W).to(DEV)
        self.depth, self.slack, self.dims, self.V, self.W = dev(depth), float(slack), dims, V, W
        self.stream = L.raw_stream(DEV)

    def _grid(self):
        return (*self.dims, ctypes.cast(self.host[0], ctypes.c_void_p), ctypes.cast(self.host[1], ctypes.c_void_p))

    def _views(self):
        p = self.L.ptr
        return (self.V, p(self.K), p(self.M), G.HEIGHT, self.W, p(self.bits))

    def votes(self, seen, hit, hidden, accumulate=0):
        p = self.L.ptr
        return self.lib.cgs_voxel_votes_depth(*self._grid(), *self._views(), p(self.depth), self.slack, accumulate, p(seen), p(hit),
                                              None if hidden is None else p(hidden), self.stream)

    def claims(self, index, support, best, clear):
        p = self.L.ptr
        return self.lib.cgs_ray_claims_depth(*self._grid(), index.numel(), p(index), p(support), *self._views(), p(self.depth),
                                             self.slack, clear, p(best), self.stream)

    def wins(self, index, support, best, out, window=1, margin=0, accumulate=0):
        p = self.L.ptr
        return self.lib.cgs_ray_wins_depth(*self._grid(), index.numel(), p(index), p(support), *self._views(), p(best),
                                           p(self.depth), self.slack, window, margin, accumulate, p(out), self.stream)


# ------------------------------------------------------------------------------------------------ the vote
@GRIDS
@pytest.mark.parametrize("V", SC.VOTE_VIEWS)
def test_the_gated_vote_is_bit_identical_to_the_host(dims, V):
    n = dims[0] * dims[1] * dims[2]
    hidden_total = 0
    for W in G.WIDTHS:
        plain_host = G.run_votes(dims, V, W, None, 0.0, "host")
        plain = G.run_votes(dims, V, W, None, 0.0, "gpu", DEV)
        assert all(np.array_equal(a, b) for a, b in zip(plain, plain_host)), W
        for kind in G.PLANES:
            depth, slack = G.plane(kind, dims, V, W)
            want = G.run_votes(dims, V, W, depth, slack, "host")
            got = G.run_votes(dims, V, W, depth, slack, "gpu", DEV)
            for name, a, b in zip(("seen", "hit", "hidden"), got, want):
                assert a.dtype == np.uint16 and np.array_equal(a, b), (kind, W, name)
            assert np.array_equal(got[0].astype(np.int64) + got[2], plain[0]), ("seen + hidden is the ungated seen", kind, W)
            if kind == "inf":
                assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1]) and not got[2].any(), W
            if kind == "nan":
                assert not got[2].any(), W
            if kind == "zero":
                assert not got[0].any() and not got[1].any() and np.array_equal(got[2], plain[0]), W
            hidden_total += int(got[2].sum())
            # the raw call writes every word of all three outputs, and of two when hidden is NULL
            raw = _Raw(dims, V, W, depth, slack)
            seen, hit, hidden = _words(n), _words(n), _words(n)
            assert raw.votes(seen, hit, hidden) == 0
            assert all(np.array_equal(t.cpu().numpy(), b) for t, b in zip((seen, hit, hidden), want)), (kind, W)
            seen, hit = _words(n), _words(n)
            assert raw.votes(seen, hit, None) == 0
            assert np.array_equal(seen.cpu().numpy(), want[0]) and np.array_equal(hit.cpu().numpy(), want[1]), (kind, W)
    assert hidden_total > 0 or (n == 1 and V == 1)


@GRIDS
def test_accumulating_unevenly_split_views_gives_the_counts_of_one_call(dims):
    V, W = 40, 33
    depth, slack = G.plane("mixed", dims, V, W)
    want = G.run_votes(dims, V, W, depth, slack, "host")
    one = G.run_votes(dims, V, W, depth, slack, "gpu", DEV)
    assert all(np.array_equal(a, b) for a, b in zip(one, want))
    for split in (1, 39):
        two = G.run_votes(dims, V, W, depth, slack, "gpu", DEV, split=split)
        assert all(np.array_equal(a, b) for a, b in zip(two, want)), split
    # V = 0: the storing call zeroes all three counts, the accumulating call leaves them
    K, M = SC.vote_cameras(V)
    none = dict(depth=depth[:0], slack=slack, return_hidden=True, backend="gpu", device=DEV)
    zero = SD.voxel_votes(SC.VOTE_BOUNDS, dims, K[:0], M[:0], G.vote_bits(V, W)[:0], G.HEIGHT, W, **none)
    assert all(not t.cpu().numpy().any() for t in zero)
    kept = tuple(_words(want[0].size) for _ in range(3))
    SD.voxel_votes(SC.VOTE_BOUNDS, dims, K[:0], M[:0], G.vote_bits(V, W)[:0], G.HEIGHT, W, counts=kept, **none)
    assert all((t.cpu().numpy() == G.SENTINEL).all() for t in kept)


# ------------------------------------------------------------------------------------------------ claims and wins
@GRIDS
@pytest.mark.parametrize("V", SC.VOTE_VIEWS)
def test_gated_claims_and_wins_are_bit_identical_to_the_host(dims, V):
    n = dims[0] * dims[1] * dims[2]
    index, support = G.listed(dims)
    outside = np.array([-1, n, n + 5, np.iinfo(np.int32).max, np.iinfo(np.int32).min], np.int32)
    at = np.sort(np.random.default_rng(n + V).integers(0, index.size + 1, outside.size))
    wide_index = np.insert(index, at, outside)                       # indices outside the grid among the listed ones
    wide_support = np.insert(support, at, np.uint16(65535))          # with the largest support: they would win every pixel
    inside = np.isin(np.arange(wide_index.size), at + np.arange(outside.size), invert=True)
    assert np.array_equal(wide_index[inside], index)
    idx_d, sup_d = torch.from_numpy(wide_index).to(DEV), torch.from_numpy(wide_support).to(DEV)
    for W in (67, 33, 1):
        plain = G.run_claims(dims, V, W, index, support, None, 0.0, "gpu", DEV)
        if W == 67 and n > 60 and V >= 3:
            assert plain[0].max() > 0 and plain[1].max() > 0, "the case holds hits and wins"
        for kind in G.PLANES:
            depth, slack = G.plane(kind, dims, V, W)
            want_best, want_wins = G.run_claims(dims, V, W, index, support, depth, slack, "host")
            best, wins = G.run_claims(dims, V, W, index, support, depth, slack, "gpu", DEV)
            assert best.dtype == np.int32 and np.array_equal(best, want_best), (kind, W)
            assert wins.dtype == np.uint16 and np.array_equal(wins, want_wins), (kind, W)
            if kind == "inf":
                assert np.array_equal(best, plain[0]) and np.array_equal(wins, plain[1]), ("the ungated kernels", W)
            raw = _Raw(dims, V, W, depth, slack)
            raw_best = torch.full((V, G.HEIGHT, W), G.SENTINEL, dtype=torch.int32, device=DEV)
            assert raw.claims(idx_d, sup_d, raw_best, clear=1) == 0
            assert np.array_equal(raw_best.cpu().numpy(), want_best), ("an index outside the grid claims nothing", kind, W)
            out = _words(wide_index.size)
            assert raw.wins(idx_d, sup_d, raw_best, out) == 0
            got = out.cpu().numpy()
            assert np.array_equal(got[inside], want_wins) and not got[~inside].any(), ("and wins nothing", kind, W)
            if kind == "zero":   # hidden in every view: best is left as it was, nothing is won
                kept = torch.full((V, G.HEIGHT, W), 7, dtype=torch.int32, device=DEV)
                assert raw.claims(idx_d, sup_d, kept, clear=0) == 0 and bool((kept == 7).all())
                assert not want_best.any() and not want_wins.any()


def test_wins_accumulate_over_split_views_at_every_window():
    dims, V, W = (65, 3, 2), 40, 67
    K, M = SC.vote_cameras(V)
    index, support = G.listed(dims)
    depth, slack = G.plane("mixed", dims, V, W)
    bits = G.vote_bits(V, W)
    for window, margin in ((0, 0), (2, 9000), (4, 65535)):
        want = G.run_claims(dims, V, W, index, support, depth, slack, "host", window=window, margin=margin)[1]
        wins = None
        for sel in (slice(0, 1), slice(1, V)):
            args = (SC.VOTE_BOUNDS, dims, index, support, K[sel], M[sel], bits[sel])
            gate = dict(depth=depth[sel], slack=slack, backend="gpu", device=DEV)
            best = SD.ray_claims(*args, G.HEIGHT, W, **gate)
            wins = SD.ray_wins(*args, best, G.HEIGHT, W, window=window, margin=margin, counts=wins, **gate)
        assert np.array_equal(wins.cpu().numpy(), want), (window, margin)


# ------------------------------------------------------------------------------------------------ the scan level
@functools.lru_cache(maxsize=None)
def _host_votes(shape):
    scan = G.solid(shape)
    _, _, keep, _, counts = G.solid_votes(shape, "host", depth_maps=list(scan.depth))
    return keep, counts


@pytest.mark.parametrize("shape", ["box", "cylinder"])
def test_the_gated_vote_finds_a_solids_edges_at_the_default_ratio(shape):
    """The assertions of the host test on the GPU back end (host prototype: box 903 kept voxels, worst sample-to-kept distance
    0.012; cylinder 541 and 0.017; none farther than 0.02 from the ground truth), and both back ends' votes and selections
    equal."""
    info, keep, counts = G.check_solid(shape, "gpu", DEV)
    want_keep, want_counts = _host_votes(shape)
    assert np.array_equal(keep, want_keep), "the kept masks of the two back ends"
    for name, a, b in zip(("seen", "hit", "hidden"), counts, want_counts):
        assert np.array_equal(a, b), name
    if shape == "box":   # (d)
        _, plain, _, cen, _ = G.solid_votes("box", "gpu", DEV)
        gt = G.ground_truth("box")
        uncovered = int((G.nearest(gt, cen) > G.COVER_RADIUS).sum())
        print(f"box, ungated: kept {plain['kept_voxels']}, uncovered {uncovered} of {len(gt)}")
        assert 2 * uncovered > len(gt), "(d) the ungated vote covers the box: the test shows nothing"


def test_the_bracket_is_covered_and_the_claims_and_directions_run_through_the_gate():
    info, keep, counts = G.check_solid("l_bracket", "gpu", DEV)   # (a) only: one far voxel was seen on it
    scan = G.solid("l_bracket")
    opts = dict(depth_maps=list(scan.depth), exclusive=True, directions=True)
    seeds, full, keep_full, _, _ = G.solid_votes("l_bracket", "gpu", DEV, **opts)
    want_seeds, want, want_keep, _, _ = G.solid_votes("l_bracket", "host", **opts)
    assert np.array_equal(keep_full, keep) and np.array_equal(keep, want_keep)
    assert np.array_equal(seeds, want_seeds) and full["exclusive_voxels"] == want["exclusive_voxels"] <= full["kept_voxels"]
    assert full["seeds"] > 0 and full["directed"] == want["directed"] > 0 and full["hidden_pairs"] == want["hidden_pairs"]
    # a budget of one view per chunk, in both sweeps, changes nothing
    cut, cut_info, _, _, _ = G.solid_votes("l_bracket", "gpu", DEV, budget_bytes=1, **opts)
    assert np.array_equal(cut, seeds) and cut_info["exclusive_voxels"] == full["exclusive_voxels"]
    assert cut_info["hidden_pairs"] == full["hidden_pairs"]
