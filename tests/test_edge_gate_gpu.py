"""GPU: the four depth-gated kernels (cgs_edge_support_depth, cgs_sample_support_depth, cgs_sample_support_oriented_depth,
cgs_sample_snap_terms_depth) against their numpy back ends BIT FOR BIT at the shapes where a kernel can go wrong -- sample
counts around a wave and a workgroup, edge counts around the four waves of a workgroup with an empty edge and ranges off
the 64-lane stride, widths 1 / 33 / 67, 1 / 2 / 5 views, both slacks, the hidden output null and given, outputs handed in
pre-filled -- and the scan-level functions on a solid against ``backend="host"`` at three budgets and both kinds of gate."""
import numpy as np
import pytest
import torch

import edge_gate_cases as G
import edge_occlusion_cases as OC
from curve_gaussian_amd import _lib as L
from curve_gaussian_amd.ops import edge_occlusion as EO
from curve_gaussian_amd.ops import edge_orient as OR
from curve_gaussian_amd.ops import edge_score as ES
from curve_gaussian_amd.ops import edge_snap as SN
from curve_gaussian_amd.ops import edge_support as SP
from curve_gaussian_amd.ops import edge_trim as ET

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.mark.parametrize("W", G.WIDTHS)
@pytest.mark.parametrize("V", G.VIEWS)
def test_gated_kernels_equal_the_host_back_ends_bit_for_bit(W, V):
    seen = hidden = 0
    combos = [(s, h) for s in G.SLACKS for h in (True, False)]
    for n, (P, E) in enumerate((P, E) for P in G.POINT_COUNTS for E in G.EDGE_COUNTS if (E > 0) == (P > 0) or E == 1):
        for slack, with_hidden in (combos[n % 4], combos[(n + 1) % 4]):
            want = G.run_operators(P, E, W, V, slack, "host", hidden=with_hidden)
            got = G.run_operators(P, E, W, V, slack, "gpu", DEV, hidden=with_hidden)
            G.assert_same(got, want, f"P={P} E={E} W={W} V={V} slack={slack} hidden={with_hidden}")
            if with_hidden:
                seen, hidden = seen + int(got["tally"][:, 0].sum()), hidden + int(got["tally_hidden"].sum())
    if W > 1:
        assert seen > 0 and hidden > 0, "the cases hold hidden and visible samples"


@pytest.mark.parametrize("P,E,W,V", [(65, 3, 33, 2), (4096, 5, 67, 5)])
def test_outputs_handed_in_come_back_added_to_or_overwritten(P, E, W, V):
    slack = 0.01
    want = G.run_operators(P, E, W, V, slack, "host", prefill=7)
    got = G.run_operators(P, E, W, V, slack, "gpu", DEV, prefill=7)
    G.assert_same(got, want, f"P={P} E={E} W={W} V={V} pre-filled")
    zero = G.run_operators(P, E, W, V, slack, "host")
    for k in ("tally", "tally_hidden", "oriented", "oriented_hidden", "views", "snap_hidden"):
        assert G.same_bits(got[k], zero[k] + 7), k
    # counts and hidden [E,V] are WRITTEN: the entry itself, on buffers full of sevens
    c = G.views_case(W, V)
    up = lambda a: torch.from_numpy(np.array(a)).to(DEV)
    pts, off, tol2 = up(OC.samples(P)), up(G.offsets_for(E, P)), up(np.asarray(ES.tolerances_squared(G.TOLERANCES), np.int32))
    K, M, d2, depth = up(c["K"]), up(c["M"].reshape(V, 12)), up(c["d2"]), up(c["depth"])
    T = len(G.TOLERANCES)
    counts = torch.full((E, V, 1 + T), 7, dtype=torch.int32, device=DEV)
    hid = torch.full((E, V), 7, dtype=torch.int32, device=DEV)
    for hidden in (hid, None):
        counts.fill_(7)
        rc = L.load().cgs_edge_support_depth(E, P, L.ptr(pts), L.ptr(off), V, L.ptr(K), L.ptr(M), G.HEIGHT, W, L.ptr(d2), T,
                                             L.ptr(tol2), L.ptr(depth), slack, L.ptr(counts), L.ptr(hidden), L.raw_stream(DEV))
        L.check(rc, "cgs_edge_support_depth")
        torch.cuda.synchronize()
        assert G.same_bits(counts.cpu().numpy(), zero["counts"])
    assert G.same_bits(hid.cpu().numpy(), zero["counts_hidden"])


def test_an_all_inf_depth_runs_the_gated_kernels_to_the_ungated_result():
    P, E, W, V = 4096, 5, 67, 5
    plain = G.run_operators(P, E, W, V, 0.0, "gpu", DEV, depth=None)
    got = G.run_operators(P, E, W, V, 0.0, "gpu", DEV, depth=np.full((V, G.HEIGHT, W), np.inf, np.float32))
    for k in ("counts", "tally", "oriented", "terms", "views"):
        assert G.same_bits(got[k], plain[k]), k
    for k in ("counts_hidden", "tally_hidden", "oriented_hidden", "snap_hidden"):
        assert not got[k].any(), k
    G.assert_same(plain, G.run_operators(P, E, W, V, 0.0, "host", depth=None), "the ungated kernels")


def test_scan_level_functions_on_a_solid_equal_the_host_at_every_budget():
    scan = G.solid("l_bracket", 5, 48, 64)
    for gate in (dict(occluder=scan.tris), dict(depth_maps=list(scan.depth))):
        want = G.comparable(G.scan_level(scan, "host", None, **gate))
        for budget, chunks in G.BUDGETS:
            got = G.scan_level(scan, "gpu", budget, device=DEV, **gate)
            assert got["snap"]["settings"]["chunks"] == chunks and got["support"]["settings"]["backend"] == "gpu"
            assert G.comparable(got) == want, (sorted(gate), budget)
    assert int(got["trim"]["hidden"].sum()) == int(scan.hidden.sum()) > 0


def test_the_solid_facts_hold_on_the_device():
    G.check_solid_facts("box", 6, 48, 64, "gpu")


def test_the_profiles_pixel_strides():
    """3 views of 1200 x 1600 with 4096 samples: the planes' strides of profiles/edge_gate.md, against the host."""
    from curve_gaussian_amd import synthetic
    from curve_gaussian_amd.ops.view_chunks import camera_arrays
    from curve_gaussian_amd.scene import solid_scan as SS
    H, W, V, P = 1200, 1600, 3, 4096
    tris, edges = SS.solid_geometry("box")
    intr, w2c = camera_arrays(SS.emap_cameras_of(synthetic.fibonacci_cameras(V, H, W)))
    pts, _ = SP.sample_edges(edges["curves_ctl_pts"], edges["lines_end_pts"], 0.0014)
    pts = np.ascontiguousarray(pts[:P])
    assert pts.shape == (P, 3)
    off = np.asarray([0, 1000, 1000, 2500, P], np.int32)
    masks = torch.from_numpy((np.random.default_rng(5).random((V, H, W)) < 0.05).astype(np.uint8)).to(DEV)
    d2 = ES.edt_squared(masks, backend="gpu", device=DEV)
    near = OR.oriented_near(OR.mask_orientation(masks, backend="gpu", device=DEV), 1, backend="gpu", device=DEV)
    depth = EO.mesh_depth(tris, intr, w2c, H, W, EO.DEPTH_WINDOW, backend="gpu", device=DEV)
    partner = OR.sample_partners(off)
    slack = EO.DEPTH_SLACK

    def run(backend):
        a, b, c = (d2, near, depth) if backend == "gpu" else (d2.cpu(), near.cpu(), depth.cpu())
        kw = dict(backend=backend, depth=c, slack=slack)
        dev = DEV if backend == "gpu" else None
        hid = [torch.zeros(P, dtype=torch.int32, device=dev) for _ in range(3)]
        counts, ch = SP.support_counts(pts, off, intr, w2c, a, (1, 2), return_hidden=True, **kw)
        tally = ET.sample_tally(pts, intr, w2c, a, (1, 2), hidden_out=hid[0], **kw)
        ot = OR.oriented_tally(pts, partner, intr, w2c, b, 1, hidden_out=hid[1], **kw)
        terms, views = SN.snap_terms(pts, intr, w2c, a, 3, hidden_out=hid[2], **kw)
        return {k: v.cpu().numpy() for k, v in dict(counts=counts, counts_hidden=ch, tally=tally, oriented=ot, terms=terms,
                                                    views=views, h0=hid[0], h1=hid[1], h2=hid[2]).items()}

    got, want = run("gpu"), run("host")
    G.assert_same(got, want, "1200 x 1600")
    assert got["h0"].sum() > 0 and got["tally"][:, 0].sum() > 0 and got["views"].sum() > 0
