"""GPU: cgs_densification_stats (csrc/densify.hip) against the reference's two lines (train.py:184-187) written in torch,
and GaussianCurveModel.accumulate_densification_stats."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _reference(mr, acc, den, radii, grad):
    """train.py:184-187 with visibility_filter = radii > 0 (gaussian_renderer/__init__.py:150 of the reference)."""
    vis = radii > 0
    mr[vis] = torch.max(mr[vis], radii[vis])
    acc[vis] += torch.norm(grad[vis, :2], dim=-1, keepdim=True)
    den[vis] += 1


def _kernel(mr, acc, den, radii, grad, skip=None):
    from curve_gaussian_amd import _lib as L
    lib = L.load()
    rc = lib.cgs_densification_stats(radii.shape[0], L.ptr(radii), L.ptr(grad), grad.shape[1], L.ptr(mr), L.ptr(acc),
                                     L.ptr(den), L.ptr(skip) if skip is not None else None, L.raw_stream(DEV))
    L.check(rc, "cgs_densification_stats")


@pytest.mark.parametrize("P", [0, 1, 4097, 200004])
def test_kernel_matches_the_reference_lines(P):
    """max_radii2D and denom bit-equal; xyz_gradient_accum within rtol 1e-6.  Worst relative difference measured on the
    MI355X: 0 (P = 1), 2.1e-7 (P = 4 097), 2.3e-7 (P = 200 004) -- one rounding of sqrtf(x*x + y*y) against torch.norm."""
    gen = torch.Generator(device=DEV).manual_seed(P + 1)
    mine = [torch.zeros(P, device=DEV), torch.zeros(P, 1, device=DEV), torch.zeros(P, 1, device=DEV)]
    ref = [t.clone() for t in mine]
    for _ in range(5):
        radii = torch.randint(1, 40, (P,), device=DEV, dtype=torch.int32, generator=gen)
        radii[torch.rand(P, device=DEV, generator=gen) < 0.4] = 0
        grad = torch.randn(P, 3, device=DEV, generator=gen) * 1e-3
        _kernel(*mine, radii, grad)
        _reference(*ref, radii, grad)
    torch.cuda.synchronize()
    assert torch.equal(mine[0], ref[0])
    assert torch.equal(mine[2], ref[2])
    torch.testing.assert_close(mine[1], ref[1], rtol=1e-6, atol=0)
    if P:
        worst = float(((mine[1] - ref[1]).abs() / ref[1].abs().clamp_min(1e-30)).max())
        print(f"P={P}: worst relative difference of xyz_gradient_accum {worst:.3e}")


def test_raised_skip_flag_writes_nothing():
    P = 4097
    gen = torch.Generator(device=DEV).manual_seed(7)
    bufs = [torch.rand(P, device=DEV, generator=gen), torch.rand(P, 1, device=DEV, generator=gen),
            torch.rand(P, 1, device=DEV, generator=gen)]
    before = [t.clone() for t in bufs]
    radii = torch.randint(1, 9, (P,), device=DEV, dtype=torch.int32, generator=gen)
    grad = torch.randn(P, 3, device=DEV, generator=gen)
    flag = torch.ones(1, dtype=torch.int32, device=DEV)
    _kernel(*bufs, radii, grad, skip=flag)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(bufs, before))
    flag.zero_()
    _kernel(*bufs, radii, grad, skip=flag)
    torch.cuda.synchronize()
    assert torch.equal(bufs[2], before[2] + 1)


def test_argument_errors_return_minus_one():
    from curve_gaussian_amd import _lib as L
    lib = L.load()
    t = torch.zeros(4, 3, device=DEV)
    r = torch.ones(4, dtype=torch.int32, device=DEV)
    p = L.ptr
    assert lib.cgs_densification_stats(0, None, None, 3, None, None, None, None, None) == 0
    assert lib.cgs_densification_stats(4, None, p(t), 3, p(t), p(t), p(t), None, None) == -1
    assert b"NULL" in lib.cgs_last_error()
    assert lib.cgs_densification_stats(4, p(r), p(t), 1, p(t), p(t), p(t), None, None) == -1
    assert b"grad_stride" in lib.cgs_last_error()
    assert lib.cgs_densification_stats(-1, p(r), p(t), 3, p(t), p(t), p(t), None, None) == -1


def test_model_method_allocates_and_matches():
    from curve_gaussian_amd.scene import GaussianCurveModel
    from util import S
    c = S.make_curves(50, 5)
    gm = GaussianCurveModel(0, 12, device=DEV).create_from_curves(c["curve_points"], c["width"], c["opacity"], None,
                                                                  c["is_bezier"])
    P = gm.n_splats
    gen = torch.Generator(device=DEV).manual_seed(3)
    ref = [torch.zeros(P, device=DEV), torch.zeros(P, 1, device=DEV), torch.zeros(P, 1, device=DEV)]
    for _ in range(3):
        radii = torch.randint(0, 5, (P,), device=DEV, dtype=torch.int32, generator=gen)
        grad = torch.randn(P, 3, device=DEV, generator=gen)
        gm.accumulate_densification_stats(radii, grad)
        _reference(*ref, radii, grad)
    torch.cuda.synchronize()
    assert torch.equal(gm.max_radii2D, ref[0]) and torch.equal(gm.denom, ref[2])
    torch.testing.assert_close(gm.xyz_gradient_accum, ref[1], rtol=1e-6, atol=0)
    with pytest.raises(ValueError):
        gm.accumulate_densification_stats(radii[:-1].contiguous(), grad)
