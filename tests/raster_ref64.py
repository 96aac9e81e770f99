"""Float64 truth, per-element error bounds and constructed scenes for the tile compositors (k_render_fwd3, k_render_bwd3,
k_render_bwd_unit): test infrastructure shared by test_raster_ref64_cpu.py and test_raster_ref64_gpu.py.

The truth is oracle/torch_ref.dense_render in float64 with float64 autograd; its `trace` hands out every (splat, pixel) pair's
unclamped alpha, dL/dalpha, dx, dy, blend weight and decision masks, from which the bounds below are summed.

Derivation of the bounds (first order in eps = 2^-24)
------------------------------------------------------
Notation, per pair (splat s, pixel p) that the float64 forward blended: alpha = opacity exp(power), power = -q / 2 with
q = A dx^2 + 2 B dx dy + C dy^2; T = the transmittance in front of the pair, w = alpha T; n_front = the number of pairs blended
in front of it at the pixel; m = A dx^2 + 2 |B| |dx dy| + C dy^2 (the sum of the magnitudes of q's terms: composite.h's `mag`).

1. The pair's own alpha.  A float32 evaluation of q -- in any order, as the plain quadratic form or as the polynomial the
   matrix cores expand about a half-quadrant centre from three-way bf16 splits (24 significant bits per coefficient, float32
   accumulation) -- rounds each of its terms once or twice: |delta power| <= c eps m, and exp turns an absolute error of the
   exponent into a relative error of alpha.  With the roundings of exp2 / log2(opacity) / the product:
       |delta alpha| / alpha <= eps (k0 + k1 m).
2. The recurrences.  T in front of the pair is a product of n_front factors (1 - alpha_t): each costs one rounding and passes
   on the relative error of its alpha_t scaled by alpha_t / (1 - alpha_t); the sums "behind" the pair (the reference's
   accum_rec recurrence, backward.cu:619-640) do the same for the pairs behind.  Calling
       X_p = sum over the pixel's blended pairs t of alpha_t / (1 - alpha_t) * m_t
   every quantity of pixel p that is a product / sum over its pairs carries eps (n + X_p) on top of 1.
3. g = alpha dL/dalpha, with dL/dalpha = sum over channels ch of d_ch (T v_s - behind_ch / (1 - alpha)), v_s the splat's value
   in the channel and behind_ch = sum_{t behind} v_t w_t (+ bg T_final for the colour).  The two halves CANCEL (completely,
   when every colour is 1), so the rounding error of g is proportional not to |g| but to the sum of the magnitudes of its terms,
       gmag = alpha sum_ch |d_ch| (T |v_s| + (sum_{t behind} |v_t| w_t + |bg| T_final) / (1 - alpha))  >=  |g|,
   (gmag == |g| when nothing cancels) and with 1. and 2.:
       |delta g| <= eps gmag (k0 + k1 (m + X_p) + k2 n_front).
   k0, k1, k2 are small integers (roundings per pair: exp2, log2, product, rcp of 1 - alpha, two fmas per recurrence step);
   their RELATIVE size is all that matters, since one measured constant K multiplies every bound: k0 = k1 = k2 = 1, and
       omega = 1 + m + X_p + n_front
   is the weight of a pair.  It multiplies each term INSIDE the sums below: it differs from pair to pair.
4. Per-splat outputs of the compositor (sums over the splat's own pairs; a float32 tree or atomic sum of n terms adds
   eps log2 n .. eps n times the sum of magnitudes, omega >= 1 covers the few hundred pairs of these scenes inside K):
       dL/dopacity        = Sg / op,                  bound  K eps sum_p gmag omega / op
       dL/dcolour         = sum w d_col,              bound  K eps sum_p w |d_col| omega      (dL/dall_map, dL/d(1/depth) alike)
       dL/dpx             = -sum g (A dx + B dy),     bound  K eps sum_p gmag (|A dx| + |B dy|) omega     (py alike)
       dL/dmeans2D (NDC)  = dL/dpx W/2, dL/dpy H/2
       dL/dconic          = -1/2 (Sxx, 2 Sxy, Syy),   bound  K eps sum_p gmag (dx^2/2, |dx dy|, dy^2/2) omega
5. 3D gradients (means3D, scales, rotations): G_3D = J_pre^T G_2D with J_pre the float64 Jacobian of the preprocess
   (px, py, conic, tz) of that splat.  The kernel's float32 chain rule adds a relative rounding per product:
       bound = |J_pre|^T B_2D + K eps |J_pre|^T |G_2D|.
   For the covariance path |J_pre| is the product of the magnitudes of its stages, |d conic / d Sigma| |d Sigma / d (S, R)|
   |d R / d q| (Truth.jacobian): the stages cancel in J_pre itself -- exactly, for a splat with equal in-plane scales, where
   d conic / d q == 0 while a float32 backward leaves the rounding of the cancelled terms (found by the term_group scenes on
   the GPU: an element with bound 0 that the kernel, legitimately, does not write as an exact zero).
6. Images, per pixel and channel: out = sum_s v_s w_s (+ bg T_final);
       bound = K eps (sum_s alpha_s (T_s |v_s| + behindmag_s / (1 - alpha_s)) (1 + m_s)  +  (n_blended + 2) (sum_s |v_s| w_s + |bg| T_final)),
   the first term being sum_s |d out / d ln alpha_s| times the pair's alpha error, the second the accumulation.

Every scale is a float64 sum of magnitudes over the element's own pairs; nothing is scaled by a tensor's maximum, and an element
whose pairs vanish has bound 0: the kernel must write an exact zero.

K
-
K is fixed by test_raster_ref64_cpu.py from the C oracle (oracle/raster_ref.c: the reference's float32 arithmetic, per-splat sums
in double): 4 x the largest ratio |oracle - truth| / (eps * scale) over all scenes and tensors, rounded up to a power of two, at
least 16.  It is never taken from a HIP run.  Measured (worst over the scenes of SCENES, all upstream gradients flowing; the
scene it was measured on in brackets; the CPU test prints them again per scene):
    color 1.28, invdepth 4.19, all_map 6.33 [centres: a pixel under one turned, elongated splat -- the float32 pixel-space centre
    and conic move the exponent by about eps m, the first term of the image bound, which counts it once];
    dL_dmeans3D 0.42, dL_dmeans2D 0.43, dL_dopacity 0.18, dL_dcolors 1.18, dL_dscales 0.46, dL_drotations 0.23,
    dL_dall_map 1.27 [uneven_17_0_1_104].
4 x 6.33 = 25.3  ->  K = 32.

Scenes
------
SCENES names, per scene, the per-quadrant list lengths it must produce (quadrant_lists checks them on the CPU) and its seed; a
seed whose scene fails a margin is replaced in the table.  One departure from a naive reading of "far centres": the reference
clamps x/z at 1.3 tan(fov) in the projection's Jacobian and its backward is not the derivative beyond, so a centre can lie at
most 0.3 * W/2 px outside the image (7 px at 48 x 48) -- m still runs into the thousands under the turned, elongated splats.
"""
import math

import numpy as np
import torch

from curve_gaussian_amd import synthetic as S
from oracle import torch_ref as TR

EPS = 2.0 ** -24
# worst |oracle - truth| / (eps * scale) per tensor over SCENES, as printed by test_raster_ref64_cpu.py
K_MEASURED = {"color": 1.28, "invdepth": 4.19, "all_map": 6.33, "dL_dmeans3D": 0.42, "dL_dmeans2D": 0.43, "dL_dopacity": 0.18,
              "dL_dcolors": 1.18, "dL_dscales": 0.46, "dL_drotations": 0.23, "dL_dall_map": 1.27}
K = 32.0   # 4 x max(K_MEASURED) = 25.3, rounded up to a power of two

DT = torch.float64


# ------------------------------------------------------------------------------------------------------------------ scenes
def _camera(H, W):
    """Camera at the origin whose axes are the world's (+z forward, +y down): view space == world space."""
    return S.make_camera((0.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.0, -1.0, 0.0), H, W)


class Builder:
    """Collects 3D splats whose projections land where wanted: centre on the camera ray through pixel (u, v) at depth z, pixel
    standard deviations (su, sv) along axes turned by `angle` in the image plane."""

    def __init__(self, H, W, seed):
        self.H, self.W = H, W
        self.cam = _camera(H, W)
        self.tfx, self.tfy = math.tan(self.cam.FoVx * 0.5), math.tan(self.cam.FoVy * 0.5)
        self.fx, self.fy = W / (2 * self.tfx), H / (2 * self.tfy)
        self.rng = np.random.default_rng(seed)
        self.rows = []

    def add(self, u, v, z, su, sv, op, angle=0.0):
        x = z * self.tfx * ((2 * u + 1) / self.W - 1)
        y = z * self.tfy * ((2 * v + 1) / self.H - 1)
        # pixel variance = (f s / z)^2 + 0.3 (the dilation): solve for s on the optical axis (off axis the projection shears
        # it a little: the lists are computed from the real projection, not from these numbers)
        s1 = math.sqrt(max(su * su - 0.3, 1e-4)) * z / self.fx
        s2 = math.sqrt(max(sv * sv - 0.3, 1e-4)) * z / self.fy
        r = self.rng
        self.rows.append(dict(mean=(x, y, z), scale=(s1, s2, 0.05 * min(s1, s2)),
                              rot=(math.cos(angle / 2), 0.0, 0.0, math.sin(angle / 2)), op=op,
                              color=r.uniform(0.2, 1.0), amap=tuple(r.normal(size=3)) + (1.0,)))

    def splats(self):
        f = lambda k: torch.tensor([r[k] for r in self.rows], dtype=torch.float32)
        return dict(means3D=f("mean"), scales=f("scale"), rotations=f("rot"), opacities=f("op").reshape(-1, 1),
                    all_map=f("amap"), colors=f("color").reshape(-1, 1))


def _stack(H, W, n, seed, centre, sigma, jitter=0.7):
    """n faint splats (opacity min(0.5, 4/n)) at distinct depths whose alpha >= 2/255 region covers all four quadrants."""
    b = Builder(H, W, seed)
    r = b.rng
    op = min(0.5, 4.0 / n)
    for i in range(n):
        b.add(centre[0] + r.uniform(-jitter, jitter), centre[1] + r.uniform(-jitter, jitter), 2.0 + 0.01 * i,
              sigma * r.uniform(1.0, 1.25), sigma * r.uniform(1.0, 1.25), op * r.uniform(0.9, 1.0), r.uniform(0, math.pi))
    return b


def _scene_stack16(n, seed):
    # (from 100 splats on the opacity is so low that a 4 px splat's alpha >= 1/255 edge would cross the tile: with tens of
    # thousands of pairs one of them always lands inside its margin -- the broad ones keep the edge outside the tile; the
    # edge inside a quadrant is what the uneven and termination scenes have)
    return _stack(16, 16, n, seed, (7.5, 7.5), 4.0 if n < 100 else 9.0)


def _scene_stack_ragged(n, seed):
    return _stack(19, 23, n, seed, (15.4, 15.6), 12.0 if n < 100 else 20.0)


QUAD_CENTRE = ((3.5, 3.5), (11.5, 3.5), (3.5, 11.5), (11.5, 11.5))


def _scene_uneven(lengths, seed):
    """Small splats confined to single quadrants of one tile: list lengths as given, depths interleaved across quadrants."""
    b = Builder(16, 16, seed)
    r = b.rng
    todo = [(q, i) for q, n in enumerate(lengths) for i in range(n)]
    order = r.permutation(len(todo))
    for k, j in enumerate(order):
        q, _ = todo[j]
        op = min(0.5, 4.0 / lengths[q])
        cx, cy = QUAD_CENTRE[q]
        b.add(cx + r.uniform(-0.4, 0.4), cy + r.uniform(-0.4, 0.4), 2.0 + 0.01 * k, r.uniform(0.85, 1.0), r.uniform(0.85, 1.0),
              op * r.uniform(0.9, 1.0), r.uniform(0, math.pi))
    return b


def _opaque(b, n, centre, sigma, z0, lo=0.85, hi=0.93, jitter=0.7):
    r = b.rng
    for i in range(n):
        b.add(centre[0] + r.uniform(-jitter, jitter), centre[1] + r.uniform(-jitter, jitter), z0 + 0.01 * i,
              sigma * r.uniform(1.0, 1.25), sigma * r.uniform(1.0, 1.25), r.uniform(lo, hi), r.uniform(0, math.pi))


def _scene_term_front(seed):
    """Opaque stack: the central pixels stop after 4 to 6 splats with 40 more behind them; the rim runs to the end."""
    b = Builder(16, 16, seed)
    _opaque(b, 46, (7.5, 7.5), 3.2, 2.0)
    return b


def _scene_term_quadrant(seed):
    """Every pixel of quadrant 0 terminates (large opaque splats centred in it) while most of quadrant 3 runs to the end."""
    b = Builder(16, 16, seed)
    _opaque(b, 30, (2.5, 2.5), 5.2, 2.0, jitter=0.5)
    return b


def _scene_term_second_batch(seed):
    """258 faint splats, then 8 opaque ones that terminate the centre inside the second batch, then 20 more."""
    b = Builder(16, 16, seed)
    r = b.rng
    for i in range(258):   # (broad: T in front of the opaque ones is nearly the same at every pixel, so that a seed can
        # keep all 256 termination tests clear of their edge with 258 pairs' worth of rounding in the bound)
        b.add(7.5 + r.uniform(-0.7, 0.7), 7.5 + r.uniform(-0.7, 0.7), 2.0 + 0.005 * i, 30.0 * r.uniform(1.0, 1.25),
              30.0 * r.uniform(1.0, 1.25), (2.5 / 258) * r.uniform(0.9, 1.0), r.uniform(0, math.pi))
    _opaque(b, 8, (7.5, 7.5), 30.0, 3.5)
    _opaque(b, 20, (7.5, 7.5), 4.0, 3.7, lo=0.3, hi=0.5)
    return b


def _scene_term_group(n_faint, seed):
    """n_faint barely visible splats, then 5 opaque ones: with n_faint = 11 / 12 the entry that terminates the centre is the
    list's 16th / 17th (the last of the first group / the first of the second)."""
    b = Builder(16, 16, seed)
    r = b.rng
    for i in range(n_faint):
        b.add(7.5 + r.uniform(-0.7, 0.7), 7.5 + r.uniform(-0.7, 0.7), 2.0 + 0.01 * i, 4.0 * r.uniform(1.0, 1.25),
              4.0 * r.uniform(1.0, 1.25), 0.03 * r.uniform(0.9, 1.0), r.uniform(0, math.pi))
    for i in range(5):   # all but uniform over the tile: T >= 0.7 * 0.12^4 > 1e-4 > 0.14^5, so the 5th of them terminates every pixel
        b.add(7.5, 7.5, 3.0 + 0.01 * i, 40.3, 40.3, r.uniform(0.86, 0.88), 0.0)
    _opaque(b, 6, (7.5, 7.5), 4.0, 3.5, lo=0.3, hi=0.5)
    return b


def _scene_ties(seed):
    """Eight bit-identical depths in mid-list (same z, different pixels): the order is by index."""
    b = Builder(16, 16, seed)
    r = b.rng
    for i in range(20):
        z = 2.5 if 6 <= i < 14 else (2.0 if i < 6 else 2.3) + 0.03 * i
        b.add(7.5 + r.uniform(-3, 3), 7.5 + r.uniform(-3, 3), z, 4.0 * r.uniform(1.0, 1.25), 4.0 * r.uniform(1.0, 1.25),
              r.uniform(0.15, 0.3), r.uniform(0, math.pi))
    return b


def _scene_centres(seed):
    """48 x 48: broad splats whose centres sit as far outside the tiles they reach as the reference's 1.3 tan(fov) clamp
    allows (its backward is not the derivative beyond: 0.3 * 24 px outside the image), elongated ones (axis ratio 30), one
    centre on a half-quadrant centre (x.5, y.5) and one exactly on a pixel."""
    b = Builder(48, 48, seed)
    r = b.rng
    far = [(-6.0, 10.0), (53.0, 30.0), (20.0, -6.5), (30.0, 54.0), (-5.0, -5.0), (53.0, 53.5)]
    for i, (u, v) in enumerate(far):
        b.add(u, v, 2.0 + 0.02 * i, 14.0 * r.uniform(1, 1.2), 14.0 * r.uniform(1, 1.2), r.uniform(0.3, 0.5), r.uniform(0, math.pi))
    for i in range(4):   # two turned (the cross term makes m hundreds of times the exponent), two along the pixel axes
        su, sv = (18.3, 0.61) if i < 2 else (24.3, 0.81)
        ang = r.uniform(0.3, 1.2) if i < 2 else (0.0, math.pi / 2)[i - 2]
        b.add(r.uniform(8, 40), r.uniform(8, 40), 2.2 + 0.02 * i, su, sv, r.uniform(0.3, 0.5), ang)
    b.add(19.5, 21.5, 2.4, 3.1, 2.1, 0.4, 0.3)     # half-quadrant centres are (x0 + 3.5, y0 + 1.5 | 5.5)
    b.add(28.0, 12.0, 2.42, 2.6, 3.4, 0.4, 1.1)    # on a pixel
    return b


def _reach(b, quadrants, z, op):
    """One splat whose alpha >= 1/255 region reaches exactly the given quadrants of the single tile (1: q0; 2: q0 q1;
    3: q0 q1 q2 -- a thin ellipse along the anti-diagonal through (5.5, 5.5); 4: all)."""
    r = b.rng
    j = lambda: r.uniform(-0.15, 0.15)
    if quadrants == 1:
        b.add(3.5 + j(), 3.5 + j(), z, 0.95, 0.9, op, r.uniform(0, math.pi))
    elif quadrants == 2:
        b.add(7.5 + j(), 3.5 + j(), z, 1.3, 0.9, op, 0.0)
    elif quadrants == 3:
        b.add(5.5 + j(), 5.5 + j(), z, 3.1, 0.62, op, -math.pi / 4)
    else:
        b.add(7.5 + j(), 7.5 + j(), z, 2.6, 2.4, op, r.uniform(0, math.pi))


def _scene_pooled(k, seed):
    """The unit backward pools the tile's (splat, quadrant) pairs in (splat, quadrant) order and cuts the pool into chunks of
    32: here 31 pairs (7 splats x 4 quadrants + 3 single-quadrant ones) come first, then a splat reaching k quadrants, whose
    run of pairs so starts on the last slot of the first chunk, then two more splats.  k = 0: 8 x 4 + 1 pairs, the last
    chunk holds exactly one."""
    b = Builder(16, 16, seed)
    r = b.rng
    z = iter(2.0 + 0.01 * i for i in range(100))
    op = lambda: r.uniform(0.25, 0.4)
    if k == 0:
        for _ in range(8):
            _reach(b, 4, next(z), op())
        _reach(b, 1, next(z), op())
        return b
    for _ in range(7):
        _reach(b, 4, next(z), op())
    for q in (0, 1, 2):
        cx, cy = QUAD_CENTRE[q]
        b.add(cx + r.uniform(-0.15, 0.15), cy + r.uniform(-0.15, 0.15), next(z), 0.95, 0.9, op(), r.uniform(0, math.pi))
    _reach(b, k, next(z), op())
    for _ in range(2):
        _reach(b, 4, next(z), op())
    return b


def _all4(n):
    return {0: (n, n, n, n)}


def _all4_ragged(n):
    return {t: (n, n, n, n) for t in range(4)}


# name -> (builder, args, seed, expected {tile: quadrant list lengths}; None = reported only)
SCENES = {}
# list-length edges: start 1; SLOTS 7 8 9; GROUP 15 16 17 31 32 33; the backward's park-or-atomics switch at list position
# CGS_BWD3_CAP = 104 (103 104 105) and, for the instances with more channels, CGS_BWD3_CAP_EXTRA = 96 (colour / inverse-depth
# gradients: 95 96 97) and CGS_BWD3_CAP_GEO = 64 (all_map gradients: 63 64 65); BWD_BATCH 127 128 129; BATCH / UB 255 256 257;
# a third backward batch 260
for _n in (1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 95, 96, 97, 103, 104, 105, 127, 128, 129, 255, 256, 257, 260):
    # (seeds replaced in the table because a decision sat inside its margin: 1095 -> 11095, 1097 -> 11097)
    SCENES[f"stack16_{_n}"] = (_scene_stack16, (_n,), {95: 11095, 97: 11097}.get(_n, 1000 + _n), _all4(_n))
    SCENES[f"ragged_{_n}"] = (_scene_stack_ragged, (_n,), 2000 + _n, _all4_ragged(_n))
SCENES["uneven_17_0_1_104"] = (_scene_uneven, ((17, 0, 1, 104),), 3001, {0: (17, 0, 1, 104)})
SCENES["uneven_0_0_0_33"] = (_scene_uneven, ((0, 0, 0, 33),), 3002, {0: (0, 0, 0, 33)})
SCENES["pooled_31_1"] = (_scene_pooled, (1,), 7001, {0: (11, 10, 10, 9)})
SCENES["pooled_31_2"] = (_scene_pooled, (2,), 7002, {0: (11, 11, 10, 9)})
SCENES["pooled_31_3"] = (_scene_pooled, (3,), 7003, {0: (11, 11, 11, 9)})
SCENES["pooled_31_4"] = (_scene_pooled, (4,), 7004, {0: (11, 11, 11, 10)})
SCENES["pooled_last_1"] = (_scene_pooled, (0,), 7005, {0: (9, 8, 8, 8)})
SCENES["term_front"] = (_scene_term_front, (), 4001, _all4(46))
SCENES["term_quadrant"] = (_scene_term_quadrant, (), 4002, _all4(30))
SCENES["term_second_batch"] = (_scene_term_second_batch, (), 4003, _all4(286))
SCENES["term_group_16"] = (_scene_term_group, (11,), 4004, _all4(22))
SCENES["term_group_17"] = (_scene_term_group, (12,), 14005, _all4(23))
SCENES["ties"] = (_scene_ties, (), 5001, _all4(20))
SCENES["centres"] = (_scene_centres, (), 6001, None)


class Scene:
    def __init__(self, name):
        fn, args, seed, expect = SCENES[name]
        b = fn(*args, seed)
        self.name, self.seed, self.expect = name, seed, expect
        self.sp, self.cam, self.H, self.W = b.splats(), b.cam, b.H, b.W
        self.tfx, self.tfy = b.tfx, b.tfy
        self.P = self.sp["means3D"].shape[0]
        self.bg = torch.tensor([0.3, 0.0, 0.0])


def scene_grads(scene, which=(True, True, True)):
    """Seeded upstream gradients (dL/dcolour, dL/dinvdepth, dL/dall_map); None where `which` is False."""
    g = torch.Generator().manual_seed(scene.seed + 7)
    H, W = scene.H, scene.W
    d = (torch.randn(1, H, W, generator=g), torch.randn(1, H, W, generator=g), torch.randn(4, H, W, generator=g))
    return tuple(t if w else None for t, w in zip(d, which))


def variant(scene, kind):
    """The splat dictionaries the instances run on: "base", "unit" (the reference call: all colours 1) and "nonunit" (unit
    but for one colour)."""
    sp = dict(scene.sp)
    if kind in ("unit", "nonunit"):
        sp["colors"] = torch.ones_like(sp["colors"])
    if kind == "nonunit":
        sp["colors"] = sp["colors"].clone()
        sp["colors"][scene.P // 2] = 0.35
    return sp


# ------------------------------------------------------------------------------------------------------------------- truth
def _pre_args(scene, ins, off):
    cam = scene.cam
    return (ins["means3D"], ins["opacities"], ins["scales"], ins["rotations"], cam.world_view_transform.to(DT),
            cam.full_proj_transform.to(DT), scene.tfx, scene.tfy, scene.H, scene.W, 1.0, off)


class Truth:
    """One float64 forward + backward of dense_render on a scene variant with one set of upstream gradients."""

    def __init__(self, scene, sp, grads=None, render_geo=True):
        self.scene, self.render_geo = scene, render_geo
        H, W, P = scene.H, scene.W, scene.P
        ins = {k: v.to(DT).requires_grad_(grads is not None) for k, v in sp.items()}
        off = torch.zeros(P, 2, dtype=DT, requires_grad=grads is not None)
        cam = scene.cam
        tr = {}
        col, radii, invd, amap = TR.dense_render(
            ins["means3D"], ins["opacities"], ins["scales"], ins["rotations"], ins["colors"], ins["all_map"],
            cam.world_view_transform.to(DT), cam.full_proj_transform.to(DT), scene.tfx, scene.tfy, H, W, scene.bg.to(DT),
            means2D_ndc_offset=off, trace=tr)
        if not render_geo:
            amap = torch.zeros_like(amap)
        self.out = dict(color=col.detach().numpy(), invdepth=invd.detach().numpy(), all_map=amap.detach().numpy())
        self.radii = radii.numpy()
        self.order = tr["order"].numpy()
        N = len(self.order)
        st = lambda k, dt=np.float64: (np.stack([t.detach().numpy() for t in tr[k]]).astype(dt) if N else np.zeros((0, H * W), dt))
        self.dx, self.dy, self.Tb = st("dx"), st("dy"), st("T")
        self.alpha_u = st("alpha")
        self.member, self.seen, self.stopped, self.blended = (st(k, bool) for k in ("member", "visible_alpha", "stopped", "blended"))
        self.px, self.py, self.conic, self.opac, self.tz = (tr[k].numpy() for k in ("px", "py", "conic", "opac", "tz"))
        self.lam, self.rect = tr["lam"].numpy(), tr["rect"].numpy()
        self.colors, self.all_map = sp["colors"].double().numpy()[:, 0], sp["all_map"].double().numpy()
        self.grads = grads
        self.g = None
        if grads is not None:
            loss = 0
            for o, d in zip((col, invd, amap), grads):
                if d is not None and (render_geo or o is not amap):
                    loss = loss + (o * d.to(DT)).sum()
            loss.backward()
            z = lambda t: (t.grad if t.grad is not None else torch.zeros_like(t)).numpy()
            m2 = np.concatenate([z(off), np.zeros((P, 1))], 1)
            self.g = dict(dL_dmeans3D=z(ins["means3D"]), dL_dmeans2D=m2, dL_dopacity=z(ins["opacities"]),
                          dL_dcolors=z(ins["colors"]), dL_dscales=z(ins["scales"]), dL_drotations=z(ins["rotations"]),
                          dL_dall_map=z(ins["all_map"]) if render_geo else np.zeros((P, 4)))
            self.dalpha = (np.stack([(t.grad if t.grad is not None else torch.zeros_like(t)).numpy() for t in tr["alpha"]])
                           if N else np.zeros((0, H * W)))
        self._pairs()

    # ---- per-pair quantities
    def _pairs(self):
        o = self.order
        A, B, C = (self.conic[o, i][:, None] for i in range(3))
        dx, dy = self.dx, self.dy
        self.m = A * dx * dx + 2 * np.abs(B) * np.abs(dx * dy) + C * dy * dy
        bl = self.blended
        self.al = np.where(bl, self.alpha_u, 0.0)
        self.w = self.al * self.Tb
        self.n_front = np.cumsum(bl, 0) - bl
        self.X = (bl * self.al / (1 - self.al) * self.m).sum(0)
        self.omega = 1 + self.m + self.X[None, :] + self.n_front
        self.T_final = (self.Tb[-1] * (1 - self.al[-1])) if len(o) else np.ones(self.scene.H * self.scene.W)
        self.n_blended = bl.sum(0)

    def _channels(self):
        """[(name, v [N], |bg|)] of the channels the forward accumulates."""
        o = self.order
        ch = [("color", self.colors[o], float(self.scene.bg[0])), ("invdepth", 1.0 / self.tz[o], 0.0)]
        if self.render_geo:
            ch += [(f"all_map{k}", self.all_map[o, k], 0.0) for k in range(4)]
        return ch

    def _chanmag(self, v, bg):
        """T |v_s| + (sum_{t behind} |v_t| w_t + |bg| T_final) / (1 - alpha_s): the magnitudes of d out / d alpha_s's terms."""
        t = np.abs(v)[:, None] * self.w
        behind = np.cumsum(t[::-1], 0)[::-1] - t + abs(bg) * self.T_final[None, :]
        return self.Tb * np.abs(v)[:, None] + behind / (1 - self.al)

    def image_bounds(self, K=None):
        K = globals()["K"] if K is None else K
        H, W = self.scene.H, self.scene.W
        out = {}
        for name, v, bg in self._channels():
            sens = (self.al * self._chanmag(v, bg) * (1 + self.m)).sum(0)
            mag = (np.abs(v)[:, None] * self.w).sum(0) + abs(bg) * self.T_final
            out[name] = (K * EPS * (sens + (self.n_blended + 2) * mag)).reshape(H, W)
        am = np.stack([out.get(f"all_map{k}", np.zeros((H, W))) for k in range(4)])
        return dict(color=out["color"][None], invdepth=out["invdepth"][None], all_map=am)

    def jacobian(self):
        """(J, Jmag), both [P, 6, 10]: d (px, py, A, B, C, tz) / d (means3D 3, scales 3, rotations 4) per splat by float64
        autograd, and the same chain with the MAGNITUDES of its stages multiplied for the covariance path,
            Jmag[conic, scales | rotations] = |d conic / d Sigma| |d Sigma / d (S, R)| |d R / d q|,   Sigma = R S^2 R^T,
        which is what the rounding of a float32 chain rule is proportional to: the stages' products cancel in J itself (a
        splat whose two in-plane scales are equal has d conic / d q == 0 exactly, and a float32 backward leaves the rounding
        of the cancelled terms there).  Jmag >= |J| element by element; for means3D the two are the same."""
        sc = self.scene
        ins = {k: sc.sp[k].to(DT).requires_grad_(True) for k in ("means3D", "opacities", "scales", "rotations")}
        px, py, conic, _, tz, _ = TR.preprocess_2d(*_pre_args(sc, ins, None))
        outs = [px, py, conic[:, 0], conic[:, 1], conic[:, 2], tz]
        P = sc.P
        z = lambda t, ref: np.zeros(ref.shape) if t is None else t.numpy()

        def jac(outs, xs):
            """[P, len(outs), sum of the xs' row sizes]: per-splat Jacobian of per-splat outputs (rows are independent)."""
            rows = []
            for o in outs:
                gs = torch.autograd.grad(o.sum(), xs, retain_graph=True, allow_unused=True)
                rows.append(np.concatenate([z(g, x).reshape(P, -1) for g, x in zip(gs, xs)], 1))
            return np.stack(rows, 1)

        J = jac(outs, (ins["means3D"], ins["scales"], ins["rotations"]))
        # the covariance path, stage by stage
        q = ins["rotations"].detach().clone().requires_grad_(True)
        R = TR._quat_to_R(q)
        J_Rq = jac([R[:, i, j] for i in range(3) for j in range(3)], (q,))                      # [P, 9, 4]
        Rl = R.detach().clone().requires_grad_(True)
        sl = ins["scales"].detach().clone().requires_grad_(True)
        Sig = Rl @ torch.diag_embed(sl ** 2) @ Rl.transpose(1, 2)
        J_SRs = jac([Sig[:, i, j] for i in range(3) for j in range(3)], (Rl, sl))               # [P, 9, 9 + 3]
        Sl = Sig.detach().clone().requires_grad_(True)
        con = TR.preprocess_2d(*_pre_args(sc, {k: v.detach() for k, v in ins.items()}, None), cov3D=Sl)[2]
        J_cS = jac([con[:, 0], con[:, 1], con[:, 2]], (Sl,))                                    # [P, 3, 9]
        a = np.abs
        Jmag = a(J)
        Jmag[:, 2:5, 3:6] = np.einsum("pij,pjk->pik", a(J_cS), a(J_SRs[:, :, 9:]))
        Jmag[:, 2:5, 6:10] = np.einsum("pij,pjk,pkl->pil", a(J_cS), a(J_SRs[:, :, :9]), a(J_Rq))
        assert (Jmag >= a(J) * (1 - 1e-9)).all()
        return J, Jmag

    def grad_bounds(self, K=None, J=None):
        """{name: ([P, ...] bound, same-shape truth recomputed from the pairs)}: the bound of every operator gradient."""
        K = globals()["K"] if K is None else K
        sc = self.scene
        P, H, W = sc.P, sc.H, sc.W
        o = self.order
        dcol, dinv, damap = (None if d is None else d.double().numpy().reshape(d.shape[0], -1) for d in self.grads)
        ups = {"color": None if dcol is None else dcol[0], "invdepth": None if dinv is None else dinv[0]}
        for k in range(4):
            ups[f"all_map{k}"] = None if damap is None or not self.render_geo else damap[k]
        gmag = np.zeros_like(self.al)
        for name, v, bg in self._channels():
            if ups[name] is not None:
                gmag += np.abs(ups[name])[None, :] * self._chanmag(v, bg)
        gmag *= self.al
        g = self.al * self.dalpha
        self.gmag, self.gpair = gmag, g
        om = self.omega
        A, B, C = (self.conic[o, i][:, None] for i in range(3))
        dx, dy = self.dx, self.dy
        full = lambda rows, shape=(P,): _scatter(rows, o, shape)
        Bd, Gd = {}, {}
        Bd["dL_dopacity"] = full(K * EPS * (gmag * om).sum(1) / self.opac[o])[:, None]
        Gd["dL_dopacity"] = full(g.sum(1) / self.opac[o])[:, None]
        wsum = lambda d: (np.zeros(len(o)), np.zeros(len(o))) if d is None else \
            ((self.w * d[None, :]).sum(1), K * EPS * (self.w * np.abs(d)[None, :] * om).sum(1))
        Gc, Bc = wsum(ups["color"])
        Gd["dL_dcolors"], Bd["dL_dcolors"] = full(Gc)[:, None], full(Bc)[:, None]
        ga = [wsum(ups[f"all_map{k}"]) for k in range(4)]
        Gd["dL_dall_map"] = np.stack([full(x[0]) for x in ga], 1)
        Bd["dL_dall_map"] = np.stack([full(x[1]) for x in ga], 1)
        Ginv, Binv = wsum(ups["invdepth"])
        # 2D state (px, py, A, B, C, tz): power = -(A dx^2 + C dy^2) / 2 - B dx dy, dx = px - pixel
        G2 = np.stack([-(g * (A * dx + B * dy)).sum(1), -(g * (C * dy + B * dx)).sum(1), -0.5 * (g * dx * dx).sum(1),
                       -(g * dx * dy).sum(1), -0.5 * (g * dy * dy).sum(1), -Ginv / self.tz[o] ** 2], 1)
        B2 = K * EPS * np.stack([(gmag * (np.abs(A * dx) + np.abs(B * dy)) * om).sum(1),
                                 (gmag * (np.abs(C * dy) + np.abs(B * dx)) * om).sum(1), 0.5 * (gmag * dx * dx * om).sum(1),
                                 (gmag * np.abs(dx * dy) * om).sum(1), 0.5 * (gmag * dy * dy * om).sum(1),
                                 Binv / (K * EPS) / self.tz[o] ** 2], 1)
        G2f, B2f = full(G2, (P, 6)), full(B2, (P, 6))
        half = np.array([0.5 * W, 0.5 * H])
        Gd["dL_dmeans2D"] = np.concatenate([G2f[:, :2] * half, np.zeros((P, 1))], 1)
        Bd["dL_dmeans2D"] = np.concatenate([B2f[:, :2] * half, np.zeros((P, 1))], 1)
        J, Jmag = self.jacobian() if J is None else J
        G3 = np.einsum("pij,pi->pj", J, G2f)
        B3 = np.einsum("pij,pi->pj", Jmag, B2f) + K * EPS * np.einsum("pij,pi->pj", Jmag, np.abs(G2f))
        for name, sl in (("dL_dmeans3D", slice(0, 3)), ("dL_dscales", slice(3, 6)), ("dL_drotations", slice(6, 10))):
            Gd[name], Bd[name] = G3[:, sl], B3[:, sl]
        self.G2, self.B2 = G2f, B2f
        return Bd, Gd

    # ---- decisions
    def terminated(self):
        return self.stopped.any(0).reshape(self.scene.H, self.scene.W)


def _scatter(rows, order, shape):
    out = np.zeros(shape)
    out[order] = rows
    return out


def truth(scene, grads, kind="base", render_geo=True):
    """Float64 outputs and float64 autograd gradients of every operator input (Truth.out, Truth.g)."""
    return Truth(scene, variant(scene, kind), grads, render_geo)


def bounds(t, K=None, J=None):
    """(image bounds, gradient bounds) of a Truth, per element (see the module docstring)."""
    gb = t.grad_bounds(K, J)[0] if t.grads is not None else None
    return t.image_bounds(K), gb


# ----------------------------------------------------------------------------------------------------------------- margins
def margins(scene, t=None, K=None):
    """Distance of every decision of the float64 forward from its edge; the first two as multiples of the pair's own bound.
    Returns a dict of the smallest margins (each must be >= its entry of MARGIN_MIN)."""
    K = globals()["K"] if K is None else K
    t = Truth(scene, variant(scene, "base")) if t is None else t
    out = {}
    reached = t.member & ~_done_before(t)
    a_err = K * EPS * (1 + t.m)
    r = np.abs(255.0 * t.alpha_u - 1.0) / a_err
    out["alpha"] = float(r[reached].min()) if reached.any() else np.inf
    tested = t.blended | t.stopped
    Tn = t.Tb * (1 - np.minimum(t.alpha_u, 0.99))
    t_err = K * EPS * (t.n_front + 1 + (1 + t.m) * t.alpha_u / (1 - np.minimum(t.alpha_u, 0.99)) + t.X[None, :])
    r = np.abs(1e4 * Tn - 1.0) / t_err
    out["T"] = float(r[tested].min()) if tested.any() else np.inf
    vis = t.radii > 0
    rad = 3.0 * np.sqrt(t.lam[vis])
    out["radius"] = float((np.minimum(np.ceil(rad) - rad, rad - np.floor(rad)) / rad).min()) if vis.any() else 1.0
    # tile rects: (p -+ radius [+ 15]) / 16 truncated -- the distance of the unclamped quotients from an integer
    R = np.ceil(rad)
    gx, gy = (scene.W + 15) // 16, (scene.H + 15) // 16
    d = 1.0
    for c, gmax in ((t.px[vis], gx), (t.py[vis], gy)):
        for q in ((c - R) / 16, (c + R + 15) / 16):
            inside = (q > 0) & (q < gmax)
            if inside.any():
                d = min(d, float(np.abs(q[inside] - np.round(q[inside])).min()))
    out["rect"] = d
    z32 = t.tz[vis].astype(np.float32)
    zs = np.sort(z32)
    gaps = np.diff(zs.view(np.int32).astype(np.int64))
    out["depth_ulps"] = int(gaps[gaps > 0].min()) if (gaps > 0).any() else 1 << 30
    if (gaps == 0).any():   # ties must be bit-identical in every arithmetic: identical 3D centres' z and a camera on the axes
        zin = scene.sp["means3D"][:, 2].numpy()[vis]
        for zv in np.unique(zs[1:][gaps == 0]):
            assert len(np.unique(zin[z32 == zv])) == 1, "depth tie between different inputs"
    out["alpha_max"] = float(t.alpha_u[t.member].max()) if t.member.any() else 0.0
    m = scene.sp["means3D"].double().numpy()
    out["clamp"] = float(min((1.3 * scene.tfx - np.abs(m[:, 0] / m[:, 2])).min() / scene.tfx,
                             (1.3 * scene.tfy - np.abs(m[:, 1] / m[:, 2])).min() / scene.tfy))
    out["near"] = float((t.tz / 0.2 - 1.0).min())
    return out


def _done_before(t):
    s = np.cumsum(t.stopped, 0)
    return (s - t.stopped) > 0


def check_margins(mg):
    assert mg["alpha"] >= 4.0, f"an alpha >= 1/255 decision sits {mg['alpha']:.2f} bounds from its edge"
    assert mg["T"] >= 4.0, f"a T < 1e-4 decision sits {mg['T']:.2f} bounds from its edge"
    assert mg["radius"] >= 1e-5, f"a radius sits {mg['radius']:.1e} (relative) from its ceil"
    assert mg["rect"] >= 1e-4, f"a tile rect edge sits {mg['rect']:.1e} tiles from an integer"
    assert mg["depth_ulps"] >= 4, f"depth keys {mg['depth_ulps']} ulp apart"
    assert mg["alpha_max"] <= 0.97, f"opacity * G reaches {mg['alpha_max']:.3f}"
    assert mg["clamp"] >= 0.01, f"|x/z| within {mg['clamp']:.3f} tan(fov) of the 1.3 tan(fov) clamp"
    assert mg["near"] >= 0.01, f"tz within {mg['near']:.3f} of the near cull"


# ---------------------------------------------------------------------------------------------------------- quadrant lists
def _quad_min_box(A, B, C, l, r, b, t):
    """min over dx in [l, r], dy in [b, t] of A dx^2 + 2 B dx dy + C dy^2 (composite.h::quad_min_box, float64)."""
    if l <= 0 <= r and b <= 0 <= t:
        return 0.0
    best = np.inf
    for x in (l, r):
        d = min(max(-B * x / C, b), t)
        best = min(best, A * x * x + (2 * B * x + C * d) * d)
    for y in (b, t):
        d = min(max(-B * y / A, l), r)
        best = min(best, C * y * y + (2 * B * y + A * d) * d)
    return best


def quadrant_lists(scene, t=None, strict=None):
    """{tile: dict(list=[splat ids in depth order], quadrants=[[ids] x 4])}: the tile list after tile culling and the four
    per-quadrant lists the compositors will walk.  Determinate or an AssertionError: every (splat, quadrant) either reaches
    alpha >= 2/255 at one of the quadrant's 64 pixel positions or has its quadratic form at or above 2 tau2 over the quadrant's
    box (quadrant_mask accepts up to 1.001 tau2 + 1e-3 + 8e-6 mag); a splat in no quadrant list must clear the whole tile's box
    the same way (common.h::tile_reach_det drops it)."""
    t = Truth(scene, variant(scene, "base")) if t is None else t
    # a scene whose table entry names no lengths (broad splats over many tiles: something always sits between the two cuts)
    # only COUNTS its undetermined entries ("slack"); positions in such a tile's list are then not compared
    strict = scene.expect is not None if strict is None else strict
    gx, gy = (scene.W + 15) // 16, (scene.H + 15) // 16
    out = {}
    yy, xx = np.mgrid[0:8, 0:8]
    for tile in range(gx * gy):
        ty, tx = divmod(tile, gx)
        ids, quads, slack = [], [[], [], [], []], 0
        for s in t.order:
            x0, y0, x1, y1 = t.rect[s]
            if not (x0 <= tx < x1 and y0 <= ty < y1):
                continue
            A, B, C = t.conic[s]
            op = t.opac[s]
            if op < 1.0 / 255.0:
                assert op < 0.5 / 255.0, "opacity in the slack of the 1/255 cut"
                continue
            tau2 = 2.0 * math.log(255.0 * op)
            assert tau2 > 0.05, "opacity in the slack of the 1/255 cut"
            hit = False
            for q in range(4):
                X0, Y0 = tx * 16 + 8 * (q & 1), ty * 16 + 8 * (q >> 1)
                dx, dy = t.px[s] - (X0 + xx), t.py[s] - (Y0 + yy)
                amax = (op * np.exp(-0.5 * (A * dx * dx + C * dy * dy) - B * dx * dy)).max()
                if amax >= 2.0 / 255.0:
                    quads[q].append(int(s))
                    hit = True
                else:
                    l, b = X0 - t.px[s], Y0 - t.py[s]
                    v = _quad_min_box(A, B, C, l, l + 7, b, b + 7)
                    assert v >= 2.0 * tau2 or not strict, \
                        f"{scene.name}: splat {s} sits in the slack of quadrant {q} of tile {tile} (q {v:.3f}, tau2 {tau2:.3f})"
                    slack += v < 2.0 * tau2
            if hit:
                ids.append(int(s))
            else:
                l, b = tx * 16 - t.px[s], ty * 16 - t.py[s]
                v = _quad_min_box(A, B, C, l, l + 15, b, b + 15)
                assert v >= 2.0 * tau2 or not strict, f"{scene.name}: splat {s} sits in the slack of tile {tile}"
        out[tile] = dict(list=ids, quadrants=quads, slack=int(slack))
    return out


def expected_n_contrib(scene, t, lists):
    """[H, W] 1-based position, in the pixel's tile list, of the last splat the float64 forward blended (0: none)."""
    H, W = scene.H, scene.W
    gx = (W + 15) // 16
    out = np.zeros(H * W, np.int64)
    rank = {s: i for i, s in enumerate(t.order.tolist())}
    tile_of = (np.arange(H)[:, None] // 16 * gx + np.arange(W)[None, :] // 16).reshape(-1)
    for tile, d in lists.items():
        pix = np.nonzero(tile_of == tile)[0]
        if d["slack"]:
            out[pix] = -1   # undetermined list: no position to compare
            continue
        for pos, s in enumerate(d["list"], 1):
            bl = t.blended[rank[s]][pix]
            out[pix[bl]] = pos
    return out.reshape(H, W)
