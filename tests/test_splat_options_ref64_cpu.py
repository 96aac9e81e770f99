"""CPU: the float64 truth of the per-splat options (tests/raster_ref64.py, "Options": spherical-harmonic colours at degrees
0 .. 3, antialiasing, cov3D_precomp, scale_modifier) and its scenes.

For every option set of OPTION_SETS: no per-splat decision inside its margin (the `clamped` flag, the antialiasing floor and
the antialiased 1/255 cut included), the undecided pixels within check_mask's limits, the scene holds the edges it is there
for (option_edges), the truth's stage sums reproduce its own autograd, and the C oracle (oracle/raster_ref.c: the reference's
float32 arithmetic) stays within every bound, element by element -- the run that measures the K of the new tensors and stages
(printed: pytest -s).  The two departures of the reference's backward from the derivative are pinned:
plain autograd differs from the C oracle by more than 1e-2 where they act, the departure Functions bring it inside the
bound, and the spherical-harmonic path needs none.

Mutation check (a copy of oracle/raster_ref.c standing in for a kernel, test_oracle_within_the_option_bounds as the judge;
the worst ratio |mutant - truth| / bound it reports, the bound being 1):
    one degree-3 direction term (SH_C3[4] sh[13] (...) of dRGBdx) with its factor halved: dL_dmeans3D 10.6 [sh3], 8.4 [nogeo_sh3],
        6.9 [sh3_aa_mod17]; the other nine sets pass
    the antialiasing formula fed the undilated c_xx, c_yy: dL_dscales 41.4, dL_drotations 10.3 [aa]; dL_dscales 1.1e3
        [sh3_aa_mod17]; dL_dcov3D 5.9e3 [cov_aa_sh2]
    dL_dscale multiplied by mod: dL_dscales 9.0e3 [mod05], 6.3e3 [mod17], 2.7e3 [sh3_aa_mod17]
    dcov[2] and dcov[4] swapped: dL_dcov3D 4.9e4 [cov], 6.1e3 [cov_aa_sh2]; dL_drotations 174 .. 2.0e4 on the ten other sets
    SH_C2[2] off in the 7th digit (0.31539156 -> 0.31539186, 9.5e-7 relative = 16 eps of ONE term): NOT caught -- colour 0.010
        (0.66 / 64, against 0.63 / 64 unmutated), dL_dsh 0.048 [sh2].  A bound of K eps = 64 eps (dL_dsh: 128 eps) times the sum
        of the magnitudes of an element's terms cannot see 16 eps of one of them, and the K rule (4 x the oracle's worst
        ratio, at least 16) allows no constant under 16: this one stays open.
"""
import functools

import numpy as np
import pytest
import torch

import raster_ref64 as R64
from util import ORA, oracle_forward

ALL = (True, True, True)
IMAGES = (("color", "color"), ("invdepth", "invdepth"), ("all_map", "out_all_map"))


def ratios(got, ref, bound_k1):
    """worst |got - ref| / bound (bound taken at K = 1); an element with bound 0 must be exact: inf where it is not."""
    got, ref, b = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bound_k1, np.float64)
    assert got.shape == ref.shape == b.shape, (got.shape, ref.shape, b.shape)
    err = np.abs(got - ref)
    zero = b == 0
    if (err[zero] != 0).any():
        return np.inf
    return float((err[~zero] / b[~zero]).max()) if (~zero).any() else 0.0


@functools.lru_cache(maxsize=None)
def built(name):
    """(scene, undecided pixels, upstream gradients, Truth with the reference's departures) of an option set."""
    sc = R64.option_scene(name)
    mask = R64.undecided_pixels(sc, R64.Truth(sc, sc.sp, None, sc.render_geo, sc.opt))
    grads = R64.scene_grads(sc, ALL, mask)
    return sc, mask, grads, R64.Truth(sc, sc.sp, grads, sc.render_geo, sc.opt)


def run_oracle(sc, grads):
    """The C oracle's images and gradients on an option scene, dL_dsh in the operator's layout (quirk 16)."""
    o = sc.opt
    fw = oracle_forward(sc.sp, sc.cam, sc.bg, sc.render_geo, o.antialiasing, o.scale_modifier, o.cov3D, o.sh, o.degree)
    gr = ORA.backward(fw, *(d.numpy() for d in grads))
    out = dict(radii=fw.radii.copy(), **{k: getattr(fw, a).copy() for k, a in IMAGES})
    out["g"] = {k: v for k, v in gr.items() if v is not None}
    if o.sh is not None:
        out["g"]["dL_dsh"] = R64.quirk16(out["g"]["dL_dsh"].astype(np.float64))
        out["rgb"] = fw._view("ora_rgb", fw.P, np.float32)     # the per-splat colours the forward computed (visible splats)
    fw.free()
    return out


def new_tensors(o):
    """The tensors whose bound an option's own tensors and stages enter: the ones the K rule (4 x the oracle's worst ratio
    stays within the bound) is applied to.  The others are bounded as on every scene (ratio <= 1): their error is that of
    the stages raster_ref64.K was measured on, on scenes that are not part of that measurement (like test_raster_ref64_cpu's
    random scenes)."""
    new = []
    if o.sh is not None:
        new += ["color", "dL_dsh", "dL_dmeans3D"]
    if o.antialiasing:   # (hrel enters every pair's alpha error: the images too)
        new += ["color", "invdepth", "all_map", "dL_dopacity", "dL_dscales", "dL_drotations", "dL_dmeans3D"]
    if o.scale_modifier != 1.0:
        new += ["dL_dscales", "dL_drotations"]
    if o.cov3D is not None:
        new += ["dL_dcov3D"]
        new = [k for k in new if k not in ("dL_dscales", "dL_drotations")]
    return sorted(set(new))


def compared(sc, t):
    """The gradient tensors an option set is compared on (colours that come from SH have no dL_dcolors)."""
    return [k for k in t.g if not (k == "dL_dcolors" and sc.opt.sh is not None)]


@pytest.mark.parametrize("name", list(R64.OPTION_SETS))
def test_oracle_within_the_option_bounds(name):
    sc, mask, grads, t = built(name)
    R64.check_mask(sc, mask)
    mg = R64.margins(sc, t, mask=mask)
    R64.check_margins(mg)
    edges = R64.option_edges(sc, t)
    img_b, _ = R64.bounds(t)
    Bd, Gd = t.grad_bounds()
    # the truth's stage sums are its autograd gradients (float64: 1e-5 of the bound's own scale)
    for k in compared(sc, t):
        assert np.abs(Gd[k] - t.g[k]).max() <= 1e-5 * Bd[k].max() + 1e-300, (k, np.abs(Gd[k] - t.g[k]).max(), Bd[k].max())
    # culled splats: every row an exact zero, in the truth and (bound 0) in whatever is compared with it
    culled = t.radii == 0
    for k in compared(sc, t):
        rows = R64.rows_of(culled, t.g[k], k)
        assert (t.g[k][rows] == 0).all() and (Bd[k][rows] == 0).all(), k
    if sc.opt.antialiasing:   # visible, antialiased below the 1/255 cut: never blended, every gradient an exact zero
        gone = (t.radii > 0) & (t.opac < 1.0 / 255.0)
        for k in compared(sc, t):
            rows = R64.rows_of(gone, t.g[k], k)
            assert (t.g[k][rows] == 0).all() and (Bd[k][rows] == 0).all(), k
    if sc.opt.sh is not None:   # coefficients beyond (degree + 1)^2 are not read
        nb = (sc.opt.degree + 1) ** 2
        raw = np.zeros((sc.P, sc.opt.sh.shape[1]))
        raw[:, nb:] = 1.0
        assert (t.g["dL_dsh"][R64.quirk16(raw) == 3.0] == 0).all() and (Bd["dL_dsh"][R64.quirk16(raw) == 3.0] == 0).all()
    got = run_oracle(sc, grads)
    assert (got["radii"] == t.radii).all()
    keep = ~mask
    worst = {k: ratios(got[k][:, keep], t.out[k][:, keep], img_b[k][:, keep]) for k, _ in IMAGES}
    for k in compared(sc, t):
        worst[k] = ratios(got["g"][k].reshape(t.g[k].shape), t.g[k], Bd[k])
    new = new_tensors(sc.opt)
    if sc.opt.sh is not None:
        # the spherical-harmonic stage alone: every visible splat's colour within K_SH eps colmag of the float64 sh_colour
        # (a clamped one: an exact 0), measured in units of eps colmag
        vis = t.radii > 0
        worst["sh_colour"] = ratios(got["rgb"][vis], t.colors[vis], R64.K_SH * R64.EPS * t.colmag[vis])
        new = new + ["sh_colour"]
    print(f"\n{sc.name}: " + " ".join(f"{k} {v}" for k, v in edges.items()))
    print(f"   undecided pixels {int(mask.sum())} of {mask.size} ({100.0 * mask.mean():.2f} %), margins "
          + " ".join(f"{k} {v:.3g}" for k, v in mg.items()))
    print("   oracle ratios |oracle - truth| / bound: " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    print("   worst ratio |oracle - truth| / bound: %.3f" % max(worst.values()))
    print("   of these the option's own tensors and stages (K measurement): " + " ".join(f"{k} {worst[k]:.3f}" for k in new))
    for k, v in worst.items():
        assert v <= 1.0, f"{k}: the oracle is outside the bound (ratio {v:.2f})"
        if k in new:
            assert 4.0 * v <= 1.0, f"{k}: the oracle takes {v:.3f} of the bound: its constant is below 4 x what the oracle needs"
            assert v <= R64.K_MEASURED_OPTIONS[k][0] * 1.005, f"{k}: {v:.3f} is above the recorded worst {R64.K_MEASURED_OPTIONS[k]}"


def test_option_k_measurements_stay_under_a_quarter_of_the_bounds():
    """The K rule on the recorded worst ratios (K_MEASURED_OPTIONS: fractions of the bound, the option set in brackets): 4 x
    the worst stays within the bound for every tensor an option's own stage enters, so K stays 64; the spherical-harmonic
    stage's and dL_dsh's inherited part's own constants are what the rule gives them (a power of two, at least 16)."""
    assert set(R64.K_MEASURED_OPTIONS) == {"color", "invdepth", "all_map", "dL_dsh", "dL_dmeans3D", "dL_dopacity", "dL_dscales",
                                           "dL_drotations", "dL_dcov3D", "sh_colour"}
    for k, (worst, where) in R64.K_MEASURED_OPTIONS.items():
        assert where in R64.OPTION_SETS and 4.0 * worst <= 1.0, (k, worst)
    pow2 = lambda x: max(16.0, 2.0 ** np.ceil(np.log2(4.0 * x)))
    assert R64.K_SH == pow2(R64.K_MEASURED_OPTIONS["sh_colour"][0] * R64.K_SH)
    assert R64.K_DL_DSH == pow2(R64.K_DL_DSH_MEASURED)


def _rel_of_max(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / np.abs(b).max())


def _plain_autograd(sc, grads):
    """Float64 autograd of dense_render WITHOUT the departures: the derivative of the forward."""
    from oracle import torch_ref as TR
    o = sc.opt
    ins = {k: v.to(R64.DT).requires_grad_(True) for k, v in sc.sp.items()}
    kw = dict(scale_modifier=o.scale_modifier, antialiasing=o.antialiasing)
    if o.sh is not None:
        ins["sh"] = o.sh.to(R64.DT).requires_grad_(True)
        kw.update(sh=ins["sh"], sh_degree=o.degree, campos=sc.cam.camera_center.to(R64.DT))
    col, _, invd, amap = TR.dense_render(ins["means3D"], ins["opacities"], ins["scales"], ins["rotations"], ins["colors"],
                                         ins["all_map"], sc.cam.world_view_transform.to(R64.DT), sc.cam.full_proj_transform.to(R64.DT),
                                         sc.tfx, sc.tfy, sc.H, sc.W, sc.bg.to(R64.DT), **kw)
    sum((o_ * d.to(R64.DT)).sum() for o_, d in zip((col, invd, amap), grads)).backward()
    return {"dL_d" + k: v.grad.numpy() for k, v in ins.items() if v.grad is not None}


def test_antialiasing_backward_departs_from_the_derivative():
    """Quirk 23: plain autograd differs from the C oracle by more than 1e-2 of the maximum on dL_dscales and dL_drotations;
    with the departure Function the oracle is inside the bound (test_oracle_within_the_option_bounds["aa"])."""
    sc, mask, grads, t = built("aa")
    got, plain = run_oracle(sc, grads)["g"], _plain_autograd(sc, grads)
    d = {k: (_rel_of_max(got[k], plain[k]), _rel_of_max(got[k], t.g[k])) for k in ("dL_dscales", "dL_drotations", "dL_dmeans3D")}
    print("\nantialiasing, (oracle vs plain autograd, oracle vs the reference formula): " + " ".join(f"{k} {v[0]:.2e} {v[1]:.2e}" for k, v in d.items()))
    assert d["dL_dscales"][0] > 1e-2 and d["dL_drotations"][0] > 1e-2
    Bd, _ = t.grad_bounds()
    for k in ("dL_dscales", "dL_drotations", "dL_dmeans3D", "dL_dopacity"):
        assert ratios(got[k], t.g[k], Bd[k]) <= 1.0, k


def test_scale_modifier_backward_lacks_the_factor_mod():
    """Quirk 24: plain autograd differs from the C oracle by more than 1e-2 of the maximum on dL_dscales (by the factor mod
    exactly: oracle x mod agrees at float32 level), not on dL_drotations and dL_dmeans3D."""
    sc, mask, grads, t = built("mod17")
    got, plain = run_oracle(sc, grads)["g"], _plain_autograd(sc, grads)
    d = {k: _rel_of_max(got[k], plain[k]) for k in ("dL_dscales", "dL_drotations", "dL_dmeans3D")}
    timesmod = _rel_of_max(got["dL_dscales"] * np.float64(1.7), plain["dL_dscales"])
    print("\nscale_modifier 1.7, oracle vs plain autograd: " + " ".join(f"{k} {v:.2e}" for k, v in d.items()) + f"; oracle x mod {timesmod:.2e}")
    assert d["dL_dscales"] > 1e-2 and timesmod < 1e-3 and d["dL_drotations"] < 1e-3 and d["dL_dmeans3D"] < 1e-3
    Bd, _ = t.grad_bounds()
    assert ratios(got["dL_dscales"], t.g["dL_dscales"], Bd["dL_dscales"]) <= 1.0


@pytest.mark.parametrize("name", ["sh1", "sh3"])
def test_sh_path_needs_no_departure(name):
    """The spherical-harmonic backward is the derivative: with no departure in play the truth IS plain autograd, bit for bit,
    and the oracle is inside its bounds (clamped splats present)."""
    sc, mask, grads, t = built(name)
    plain = _plain_autograd(sc, grads)
    assert (plain["dL_dmeans3D"] == t.g["dL_dmeans3D"]).all() and (R64.quirk16(plain["dL_dsh"]) == t.g["dL_dsh"]).all()
    got = run_oracle(sc, grads)["g"]
    Bd, _ = t.grad_bounds()
    assert int(((t.radii > 0) & t.clampd).sum()) >= 5
    for k in ("dL_dmeans3D", "dL_dsh"):
        assert ratios(got[k], t.g[k], Bd[k]) <= 1.0, k


@pytest.mark.parametrize("name", ["stack16_17", "turned_1"])
def test_default_options_return_the_same_float64_numbers(name):
    """All options at their defaults, through the option path (Options(), reference_backward, the eight-entry 2D state):
    the same images and gradients as the call without options, bit for bit; the same image and compositor bounds, and 3D
    bounds that are never below (the option path's |d conic / d cov2D| is the formula's magnitudes)."""
    sc = R64.Scene(name)
    grads = R64.scene_grads(sc, ALL)
    a, b = R64.Truth(sc, sc.sp, grads), R64.Truth(sc, sc.sp, grads, opt=R64.Options())
    for k in a.out:
        assert (a.out[k] == b.out[k]).all(), k
    for k in a.g:
        assert (a.g[k] == b.g[k]).all(), k
    (ia, ga), (ib, gb) = R64.bounds(a), R64.bounds(b)
    for k in ia:
        assert (ia[k] == ib[k]).all(), k
    for k in ga:   # (the option path takes |d conic / d cov2D| from the magnitudes of the kernels' formula: never below)
        if k in ("dL_dmeans3D", "dL_dmeans2D", "dL_dscales", "dL_drotations"):
            assert (gb[k] >= ga[k] * (1 - 1e-12)).all(), k
        else:
            assert (ga[k] == gb[k]).all(), k
