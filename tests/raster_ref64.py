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
    color 2.88 [turned_0], invdepth 6.07, all_map 10.66, dL_dcolors 5.00 [turned_2: a 61 x 77 image under a turned camera,
    pixels under thin (0.7 .. 0.9 px) splats at axis ratio 20 -- the float32 per-splat state moves the exponent by more than
    eps m there: the pixel-space centre is rounded at eps |px| (px up to 77, not 16) and the conic of a thin turned splat
    loses the digits that a c - b^2 cancels; K absorbs both, as it did at 6.33 for the `centres` scene at 48 x 48];
    dL_dmeans3D 0.79, dL_dmeans2D 0.82, dL_dopacity 1.89, dL_dscales 0.99, dL_dall_map 5.14 [turned_1],
    dL_drotations 0.65 [long_9000].
4 x 10.66 = 42.6  ->  K = 64.  (Before the long and turned scenes: all_map 6.33 [centres], K = 32; the longest list, 9000
entries, stays at dL_dall_map 2.64: the accumulation terms of the bounds hold their form.)

Scenes
------
SCENES names, per scene, the per-quadrant list lengths it must produce (quadrant_lists checks them on the CPU) and its seed; a
seed whose scene fails a margin is replaced in the table.  One departure from a naive reading of "far centres": the reference
clamps x/z at 1.3 tan(fov) in the projection's Jacobian and its backward is not the derivative beyond, so a centre can lie at
most 0.3 * W/2 px outside the image (7 px at 48 x 48) -- m still runs into the thousands under the turned, elongated splats.

Decisions: cleared per splat, masked per pixel
----------------------------------------------
A float32 forward may legitimately decide the other way wherever the float64 forward decides within a few bounds of an edge,
and nothing of such an element can be compared.  Two kinds:
- per splat (radius ceil, tile rect edge, near cull, the 1.3 tan(fov) clamp, depth keys under 4 ulp apart or tied between
  different 3D centres, opacity in the slack of the 1/255 cut): splat_failures.  Builder.clear re-draws such a splat from the
  scene's own rng when the scene is built (random_scene drops it), so no scene has one.
- per pair (alpha >= 1/255, T < 1e-4, the 0.99 clamp): with tens of thousands of pairs one always lands inside its margin.
  undecided_pixels masks the PIXEL of such a pair: its three upstream gradients are zero (scene_grads), so each of its pairs
  contributes g = alpha * sum_ch d_ch (...) = 0 to every gradient exactly, in any arithmetic and whichever way a kernel
  decides; the truth and the bounds need no new term, and the pixel is left out of the image, `terminated` and n_contrib
  comparisons.  A kernel that turns a zero upstream gradient into a contribution fails the bound == 0 => exact zero rule.
  check_mask: at most 5 % of a scene's pixels and 16 of the 64 of any quadrant of any tile; the scenes of OLD_SCENES (lists of
  at most 286 entries, built until every pair clears its margin) must have none.
The long_* scenes (one tile, 1024 .. 9000 entries: every sort and every batch carry of the compositors), the turned_* scenes
(20 tiles under the three turned cameras, depth ties) and the random scenes (RANDOM_SCENES) rest on the mask.

Options
-------
The per-splat kernels' options (Options: spherical-harmonic colours, antialiasing, scale_modifier, cov3D_precomp; the scenes
of OPTION_SETS; test_splat_options_ref64_cpu.py / _gpu.py).  The truth is dense_render with reference_backward=True: float64
autograd but for the reference's two departures from the derivative, each a torch.autograd.Function evaluating the reference's
own formula in float64 (torch_ref._AntialiasingScaleRef, backward.cu:234-241; _ScaleModifierRef, backward.cu:346,374-376;
SURVEY quirks 23, 24).  The 2D state reaching the per-splat backward is (px, py, A, B, C, tz, effective opacity, colour); the
bounds keep the construction above (first order in eps, sums of the magnitudes of an element's own terms, bound 0 = exact zero):
- SH colour: the stage has its own constant, K_SH eps colmag, colmag = |C0 sh_0| + sum over the active k of |c_k basis_k|_mag
  |sh_k| + 0.5 (|.|_mag: the sum of the magnitudes of the basis function's monomials), 0 for a clamped colour; measured on the
  per-splat colour alone.  It is ADDED to the compositor's part (which stays at K with |v_s|): K_SH eps sum_s colmag_s w_s in
  the colour image, (K_SH / K) colmag in place of |v_s| as a further term of gmag.
  dL_dsh[k]: |c_k basis_k|_mag ((K_DL_DSH / K) bound of dL_dcolour + K_SH eps |dL_dcolour|), then quirk 16's layout (quirk16)
  applied to truth and bound alike; the view-direction path into dL_dmeans3D: sum_k |sh_k| |d (c_k basis_k) / d dir| times
  |d dir / d mean|.
- two terms the option scenes' sub-0.04 px splats drawn on a pixel centre made necessary (the C oracle was outside without
  them; option path only, so no compositor scene's bound changes): |d conic / d cov2D| from the magnitudes of the terms of
  the kernels' formula, whose (denom - c_xx c_yy) cancels, and 16 eps |px| for the rounding of the pixel-space centre in the
  moments of g (see grad_bounds, jacobian_opt).
- antialiasing: h = sqrt(max(0.000025, det0 / det)) has the relative error eps hrel, hrel = 1/2 ((|a0 c0| + b0^2) / |det0| +
  (a c + b^2) / det) -- det0 = a0 c0 - b0^2 cancels for thin splats --, which joins m in every pair's alpha error (m_rel) and the
  effective opacity's gradient; the reference-formula gradient of h goes through |d h / d cov2D| |d cov2D / d Sigma| and the
  stage magnitudes of section 5.
- cov3D_precomp: Jmag ends at |d conic / d Sigma|; the off-diagonal entries of dL_dcov3D sum both symmetric entries (factor 2).
- scale_modifier: |d Sigma / d S| carries mod^2, divided by mod for the departure; |d Sigma / d R| carries mod^2 s^2.
Truth.jacobian_opt builds these; with every option at its default the numbers are those of the path above
(test_default_options_return_the_same_float64_numbers).  K stays 64; K_MEASURED_OPTIONS holds the oracle's worst ratios on the
option sets, and dL_dsh alone has its own constant K_DL_DSH.
"""
import math

import numpy as np
import torch

from curve_gaussian_amd import synthetic as S
from oracle import torch_ref as TR

EPS = 2.0 ** -24
# worst |oracle - truth| / (eps * scale) per tensor over SCENES, as printed by test_raster_ref64_cpu.py
K_MEASURED = {"color": 2.88, "invdepth": 6.07, "all_map": 10.66, "dL_dmeans3D": 0.79, "dL_dmeans2D": 0.82, "dL_dopacity": 1.89,
              "dL_dcolors": 5.00, "dL_dscales": 0.99, "dL_drotations": 0.65, "dL_dall_map": 5.14}
K = 64.0   # 4 x max(K_MEASURED) = 42.6, rounded up to a power of two
# The option sets (OPTION_SETS; test_splat_options_ref64_cpu.py measures and prints all of this from the C oracle).
# K_SH: the spherical-harmonic stage's own constant -- the per-splat colour against eps colmag, measured on the colour alone
# (the oracle's rgb buffer): worst 4.67 [sh3_aa_mod17, an isolated degree-3 coefficient]; 4 x 4.67 = 18.7 -> 32.  It bounds
# the colour's rounding wherever the colour enters (images, gmag, the basis factor of dL_dsh); the compositor's part of every
# bound stays at K.
K_SH = 32.0
# K_DL_DSH: the constant of the part of dL_dsh's bound inherited from the compositor's dL_dcolour (dL_dsh[k] = c_k basis_k
# dL_dcolour): on these random clouds dL_dcolour's own error reaches a third of K (as on test_raster_ref64_cpu's random scenes),
# 20.84 in dL_dsh[0] = C0 dL_dcolour on sh0: 4 x 20.84 = 83.4 -> 128.
K_DL_DSH_MEASURED = 20.84
K_DL_DSH = 128.0
# worst |oracle - truth| / bound per tensor whose bound an option's own stage enters (tensor: (worst, option set)); the K rule
# asks 4 x worst <= 1 of each
K_MEASURED_OPTIONS = {"color": (0.170, "sh0"), "invdepth": (0.111, "sh3_aa_mod17"), "all_map": (0.145, "sh3_aa_mod17"),
                      "dL_dmeans3D": (0.204, "aa"), "dL_dsh": (0.131, "sh2"), "dL_dopacity": (0.024, "cov_aa_sh2"),
                      "dL_dscales": (0.089, "aa"), "dL_drotations": (0.082, "sh3_aa_mod17"), "dL_dcov3D": (0.043, "cov_aa_sh2"),
                      "sh_colour": (0.146, "sh3_aa_mod17")}

DT = torch.float64


# ------------------------------------------------------------------------------------------------------------------ scenes
def _camera(H, W):
    """Camera at the origin whose axes are the world's (+z forward, +y down): view space == world space."""
    return S.make_camera((0.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.0, -1.0, 0.0), H, W)


def _mat_to_quat(R):
    """(w, x, y, z) of a rotation matrix (Shepperd's branch on the largest of w, x, y, z)."""
    t = (R[0, 0] + R[1, 1] + R[2, 2], R[0, 0], R[1, 1], R[2, 2])
    k = int(np.argmax(t))
    if k == 0:
        q = np.array([1 + t[0], R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    elif k == 1:
        q = np.array([R[2, 1] - R[1, 2], 1 + 2 * R[0, 0] - t[0], R[0, 1] + R[1, 0], R[0, 2] + R[2, 0]])
    elif k == 2:
        q = np.array([R[0, 2] - R[2, 0], R[0, 1] + R[1, 0], 1 + 2 * R[1, 1] - t[0], R[1, 2] + R[2, 1]])
    else:
        q = np.array([R[1, 0] - R[0, 1], R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], 1 + 2 * R[2, 2] - t[0]])
    return q / np.linalg.norm(q)


class Builder:
    """Collects 3D splats whose projections land where wanted: centre on the camera ray through pixel (u, v) at depth z, pixel
    standard deviations (su, sv) along axes turned by `angle` in the image plane.  `cam`: a general camera (None: the one at
    the origin with the world's axes); rows that name the same `tie` share one bit-identical 3D centre."""

    def __init__(self, H, W, seed, cam=None):
        self.H, self.W = H, W
        self.cam = _camera(H, W) if cam is None else cam
        self.turned = cam is not None
        V = self.cam.world_view_transform.double().numpy().T          # p_view = V p_world
        self.Rwc, self.twc = V[:3, :3], V[:3, 3]
        self.tfx, self.tfy = math.tan(self.cam.FoVx * 0.5), math.tan(self.cam.FoVy * 0.5)
        self.fx, self.fy = W / (2 * self.tfx), H / (2 * self.tfy)
        self.rng = np.random.default_rng(seed)
        self.rows = []

    def _place(self, u, v, z, su, sv, angle):
        x = z * self.tfx * ((2 * u + 1) / self.W - 1)
        y = z * self.tfy * ((2 * v + 1) / self.H - 1)
        # pixel variance = (f s / z)^2 + 0.3 (the dilation): solve for s on the optical axis (off axis the projection shears
        # it a little: the lists are computed from the real projection, not from these numbers)
        s1 = math.sqrt(max(su * su - 0.3, 1e-4)) * z / self.fx
        s2 = math.sqrt(max(sv * sv - 0.3, 1e-4)) * z / self.fy
        mean, rot = (x, y, z), (math.cos(angle / 2), 0.0, 0.0, math.sin(angle / 2))
        if self.turned:   # the same splat in the camera's frame, carried to the world
            c, s = math.cos(angle), math.sin(angle)
            mean = tuple(self.Rwc.T @ (np.array(mean) - self.twc))
            rot = tuple(_mat_to_quat(self.Rwc.T @ np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])))
        return dict(mean=mean, scale=(s1, s2, 0.05 * min(s1, s2)), rot=rot)

    def add(self, u, v, z, su, sv, op, angle=0.0, tie=None):
        r = self.rng
        self.rows.append(dict(self._place(u, v, z, su, sv, angle), op=op,
                              color=r.uniform(0.2, 1.0), amap=tuple(r.normal(size=3)) + (1.0,),
                              spec=[u, v, z, su, sv, angle], tie=tie))

    def splats(self):
        f = lambda k: torch.tensor([r[k] for r in self.rows], dtype=torch.float32)
        return dict(means3D=f("mean"), scales=f("scale"), rotations=f("rot"), opacities=f("op").reshape(-1, 1),
                    all_map=f("amap"), colors=f("color").reshape(-1, 1))

    def clear(self, max_rounds=64):
        """Re-draws, from the scene's own rng, every splat one of whose per-splat decisions (splat_failures) sits inside
        its margin -- a nudge of its centre (of all rows of its tie, together), depth, size and opacity -- until none
        does.  Returns the number of re-draws; a scene whose splats all pass is left as it was built, rng included."""
        n = 0
        for _ in range(max_rounds):
            fail = np.nonzero(splat_failures(self.splats(), self.cam, self.H, self.W).any(1))[0]
            if not len(fail):
                return n
            r = self.rng
            for i in fail:
                row = self.rows[i]
                du, dv, fz = r.uniform(-0.3, 0.3), r.uniform(-0.3, 0.3), 1.0 + r.uniform(-2e-5, 2e-5)
                fs, fo = r.uniform(0.97, 1.03, 2), r.uniform(0.97, 1.03)
                for j, other in enumerate(self.rows):
                    if j == i or (row["tie"] is not None and other["tie"] == row["tie"]):
                        sp = other["spec"]
                        sp[0], sp[1], sp[2] = sp[0] + du, sp[1] + dv, sp[2] * fz
                        if j == i:
                            sp[3], sp[4], other["op"] = sp[3] * fs[0], sp[4] * fs[1], other["op"] * fo
                        other.update(self._place(*sp))
                n += 1
        raise AssertionError(f"Builder.clear: per-splat margins still fail after {max_rounds} rounds")


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


def _faint(b, n, z0, dz, op_scale=1.0, tie_groups=0, sigma=1.5):
    """n small faint splats (sigma .. 1.25 sigma px, opacity 0.02 .. 0.04 times op_scale but at least 0.011: above 2/255 at
    the pixel next to the centre) whose centres lie inside the single tile, at depths z0 + dz * (a permutation of 0 .. n-1);
    with tie_groups, row i takes the centre of group i % tie_groups."""
    r = b.rng
    k = tie_groups or n
    depth = r.permutation(k)
    cu, cv = r.uniform(0.5, 14.5, k), r.uniform(0.5, 14.5, k)
    for i in range(n):
        j = i % k
        b.add(cu[j], cv[j], z0 + dz * depth[j], sigma * r.uniform(1.0, 1.25), sigma * r.uniform(1.0, 1.25),
              max(0.011, op_scale * r.uniform(0.02, 0.04)), r.uniform(0, math.pi), tie=j if tie_groups else None)


def _scene_long(n, seed):
    """One 16 x 16 tile whose list is exactly n entries long: every centre inside the tile, so faint that no pixel
    terminates: beyond 2500 entries the opacities shrink with 1 / n, beyond 5000 the splats as well (sigma 1 px), which keeps
    sum alpha of a pixel near 5 and the pairs on the alpha >= 1/255 edge few."""
    b = Builder(16, 16, seed)
    _faint(b, n, 2.0, 0.0005, min(1.0, 2500.0 / n), sigma=1.5 if n <= 5000 else 1.0)
    return b


def _scene_long_term(seed):
    """1100 faint entries that leave T well above 1e-4, then 8 opaque splats that terminate the centre pixels inside the
    forward's fifth batch of 256 (the backward's ninth of 128) while the rim runs on, then 200 more faint entries."""
    b = Builder(16, 16, seed)
    _faint(b, 1100, 2.0, 0.0005)
    _opaque(b, 8, (7.5, 7.5), 3.2, 3.0)
    _faint(b, 200, 3.5, 0.0005)
    return b


def _scene_long_ties(seed):
    """1700 entries in one tile on 300 distinct centres: depth ties of 5 or 6 rows each, ordered by index."""
    b = Builder(16, 16, seed)
    _faint(b, 1700, 2.0, 0.001, tie_groups=300)
    return b


# the turned cameras of test_raster_gpu.CAMS (eye, target, up); the last one sits inside that module's random cloud
TURNED_CAMS = [((0.5, -1.6, 0.7), (0.5, 0.5, 0.5), (0, 0, 1)), ((2.0, 1.4, 1.1), (0.4, 0.5, 0.6), (0, 0, 1)),
               ((0.5, 0.5, 0.5), (0.9, 0.2, 0.5), (0, 0, 1))]
TURNED_HW = (61, 77)   # the 4 x 5 tiles of a 64 x 80 image, cut so that the last row and the last column of tiles are ragged


def _scene_turned(cam_i, seed):
    """About 300 splats in front of a turned camera: two screen-filling ones, 40 thin elongated ones (axis ratio 20), 8
    centres that three rows each share (depth ties, ordered by index) and small ones."""
    H, W = TURNED_HW
    b = Builder(H, W, seed, cam=S.make_camera(*TURNED_CAMS[cam_i], H, W))
    r = b.rng
    uv = lambda: (r.uniform(1.0, W - 2.0), r.uniform(1.0, H - 2.0))
    for z in (1.5, 2.5):
        b.add(W / 2 + r.uniform(-6, 6), H / 2 + r.uniform(-6, 6), z, 60.0 * r.uniform(1.0, 1.2), 60.0 * r.uniform(1.0, 1.2),
              r.uniform(0.15, 0.25), r.uniform(0, math.pi))
    for _ in range(40):
        sv = r.uniform(0.7, 0.9)
        b.add(*uv(), r.uniform(1.0, 4.0), 20.0 * sv, sv, r.uniform(0.3, 0.6), r.uniform(0, math.pi))
    for g in range(8):
        (u, v), z = uv(), r.uniform(1.0, 4.0)
        for _ in range(3):
            b.add(u, v, z, r.uniform(1.5, 4.0), r.uniform(1.5, 4.0), r.uniform(0.1, 0.5), r.uniform(0, math.pi), tie=g)
    for _ in range(234):
        b.add(*uv(), r.uniform(1.0, 4.0), r.uniform(0.8, 3.0), r.uniform(0.8, 3.0), r.uniform(0.1, 0.7), r.uniform(0, math.pi))
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
    # (seeds replaced in the table because a decision sat inside its margin: 1095 -> 11095, 1097 -> 11097; at K = 64, whose
    # margins are twice as wide, 1096 -> 21096)
    SCENES[f"stack16_{_n}"] = (_scene_stack16, (_n,), {95: 11095, 96: 21096, 97: 11097}.get(_n, 1000 + _n), _all4(_n))
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
OLD_SCENES = tuple(SCENES)   # every pair decision of these clears its margin: their masks (undecided_pixels) are empty

# Scenes whose undecided pixels are masked, with a fifth table entry: `list` = the exact length of tile 0's list (None: the
# lists are reported), `layout` = the binning layout the operator's SECOND call must report (1: single-pass buckets, whose
# capacity is 5/4 of the longest list + 64, rounded up to 64 -- 0: exact, once that passes bucket_cap_limit() = 4096 entries,
# which lists from 3226 entries on do), `instances` = "long": four instances only (three truths; the float64 walk dominates).
# long_N: the rank sort's first and last length (1025, 2048), the LDS network's (2049, 4096), the global-memory network (4097,
# 9000); the forward carries T through 4 .. 36 batches of 256, the backward through twice as many of 128.
for _n in (1024, 1025, 2048, 2049, 4096, 4097, 9000):
    SCENES[f"long_{_n}"] = (_scene_long, (_n,), 8000 + _n, None, dict(list=_n, layout=int(_n <= 3225), instances="long"))
SCENES["long_term_1100"] = (_scene_long_term, (), 8101, None, dict(list=1308, layout=1, instances="long"))
SCENES["long_ties"] = (_scene_long_ties, (), 8102, None, dict(list=1700, layout=1, instances="long"))
for _k in range(3):
    SCENES[f"turned_{_k}"] = (_scene_turned, (_k,), 8200 + _k, None, dict(list=None, layout=1, instances="all"))


class Scene:
    def __init__(self, name, built=None):
        if built is None:
            fn, args, seed, expect = SCENES[name][:4]
            opts = SCENES[name][4] if len(SCENES[name]) > 4 else None
            b = fn(*args, seed)
            self.redrawn = b.clear()
            sp, cam, H, W = b.splats(), b.cam, b.H, b.W
        else:   # (splats, camera, H, W, seed): a scene from elsewhere (the random ones), cleared by its maker
            sp, cam, H, W, seed = built
            expect, opts, self.redrawn = None, dict(list=None, layout=None, instances="all"), 0
        self.name, self.seed, self.expect = name, seed, expect
        self.masked = opts is not None          # undecided pixels are masked instead of forbidden
        self.list_len, self.layout, self.instances = ((opts["list"], opts["layout"], opts["instances"]) if opts else (None, 1, "all"))
        self.sp, self.cam, self.H, self.W = sp, cam, H, W
        self.tfx, self.tfy = math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5)
        self.P = self.sp["means3D"].shape[0]
        self.bg = torch.tensor([0.3, 0.0, 0.0])


# Random scenes from the generator of test_raster_gpu's bucket-against-exact fuzz test (synthetic.random_splats under its three
# cameras, every third with the depth-tie trick), sized to the pair budget P * H * W <= 4e6:
# (seed, H, W, P, smallest scale, largest / smallest, camera, depth ties).  A row whose scene misses a mask condition
# (check_mask) is replaced, as in SCENES.
RANDOM_SCENES = [(2001, 33, 47, 500, 0.01, 10, 0, True), (2002, 64, 64, 500, 0.002, 40, 1, False), (2003, 16, 47, 3000, 0.01, 2, 2, False),
                 (2004, 100, 128, 300, 0.05, 2, 0, True), (2005, 33, 64, 1500, 0.002, 10, 1, False), (2006, 64, 47, 64, 0.05, 10, 2, False),
                 (2007, 16, 16, 3000, 0.01, 10, 0, True), (2008, 100, 47, 500, 0.01, 40, 1, False)]


def random_scene(row):
    """The Scene of a RANDOM_SCENES row: splats one of whose per-splat decisions sits inside its margin (splat_failures, off-
    screen ones included) are dropped before anything runs."""
    seed, H, W, P, lo, mult, cam_i, ties = row
    sp = S.random_splats(P, seed, scale_range=(lo, lo * mult))
    if ties:
        sp["means3D"] = sp["means3D"][torch.arange(P) % max(1, P // 20)]
    cam = S.make_camera(*TURNED_CAMS[cam_i], H, W)
    keep = torch.from_numpy(~splat_failures(sp, cam, H, W, outside=True).any(1))
    sp = {k: v[keep].contiguous() for k, v in sp.items()}
    assert not splat_failures(sp, cam, H, W, outside=True).any()
    return Scene(f"random_{seed}", built=(sp, cam, H, W, seed))


# Option sets (module docstring: "Options"): name -> (seed, camera, sh degree or None, M, antialiasing, scale_modifier,
# cov3D_precomp, render_geo).  A seed whose scene misses a mask condition or an edge count (option_edges) is replaced.
OPTION_SETS = {
    "sh0": (3100, 0, 0, 1, False, 1.0, False, True), "sh1": (3101, 1, 1, 4, False, 1.0, False, True),
    "sh2": (3102, 2, 2, 9, False, 1.0, False, True), "sh3": (3103, 0, 3, 16, False, 1.0, False, True),
    "sh1_m16": (3104, 1, 1, 16, False, 1.0, False, True), "aa": (3105, 2, None, 0, True, 1.0, False, True),
    "cov": (3106, 0, None, 0, False, 1.0, True, True), "mod05": (3107, 1, None, 0, False, 0.5, False, True),
    "mod17": (3108, 2, None, 0, False, 1.7, False, True), "sh3_aa_mod17": (3109, 0, 3, 16, True, 1.7, False, True),
    "cov_aa_sh2": (3110, 1, 2, 9, True, 1.0, True, True), "nogeo_sh3": (3111, 2, 3, 16, False, 1.0, False, False)}
OPTION_HW = (45, 64)     # 3 x 4 tiles, the last row ragged
TAGS = ("random", "thin", "below_floor", "faint", "near", "offscreen", "below_floor_drawn")


def option_scene(name):
    """The Scene of an OPTION_SETS row, with .opt (Options), .render_geo and .tag ([P] index into TAGS): 330 random splats
    (900 under the third camera; synthetic.random_splats, scales 0.01 .. 0.08) under a turned camera plus placed ones -- under antialiasing 12 thin ones at
    axis ratio 20 turned in the image plane; 8 far ones of 0.02 .. 0.03 px (antialiasing ratio below its floor 0.000025), 8 of 0.1 px at
    opacity 0.05 (above the floor; antialiased opacity under 0.5 / 255: visible, never blended), 6 inside the near plane and 6
    whose tile rectangle is empty beyond the right edge.  Splats with a per-splat decision inside its margin (splat_failures
    with the options, off-screen ones included) are dropped, then random ones from the tail until P is no multiple of 64."""
    seed, cam_i, degree, M, aa, mod, use_cov, render_geo = OPTION_SETS[name]
    H, W = OPTION_HW
    cam = S.make_camera(*TURNED_CAMS[cam_i], H, W)
    n_random = 330 if cam_i < 2 else 900     # (the third camera sits inside the cloud: it sees one splat in seven)
    sp = S.random_splats(n_random, seed, scale_range=(0.01, 0.08))
    b = Builder(H, W, seed + 50, cam=cam)
    r = b.rng
    uv = lambda: (r.uniform(2.0, W - 3.0), r.uniform(2.0, H - 3.0))
    tags = [0] * n_random
    # (thin ones under antialiasing only, where the issue is their cancelling det0: without it the float32 conic of a thin
    # turned splat is the compositor scenes' subject, turned_*, and costs the images of these small scenes up to 65 of K = 64)
    for _ in range(12 if aa else 0):
        sv = r.uniform(0.7, 0.9)
        b.add(*uv(), r.uniform(1.0, 3.0), 20.0 * sv, sv, r.uniform(0.3, 0.6), r.uniform(0, math.pi))
    for _ in range(8):
        s = math.sqrt(0.3 + r.uniform(0.02, 0.03) ** 2)
        b.add(*uv(), r.uniform(3.0, 4.0), s, s, r.uniform(0.2, 0.35), 0.0)   # (times h = 0.005: under 0.5 / 255)
    for _ in range(8):
        s = math.sqrt(0.3 + 0.1 ** 2)
        b.add(*uv(), r.uniform(1.5, 3.0), s, s, 0.05, 0.0)
    for _ in range(6):
        b.add(*uv(), 0.1, 2.0, 2.0, 0.5, 0.0)
    for _ in range(6):
        b.add(W + 6.0, r.uniform(2.0, H - 3.0), r.uniform(1.5, 3.0), 0.8, 0.8, 0.5, 0.0)
    for _ in range(6):   # below the floor and DRAWN: opacity 0.93 .. 0.95 times h = 0.005 is 1.2 / 255, and the centre lies within
        # 0.08 px of a pixel centre, where G >= 0.98: the floored h reaches the image and its zeroed gradient meets a dL_dopacity
        s = math.sqrt(0.3 + r.uniform(0.02, 0.03) ** 2)
        b.add(int(r.uniform(2.0, W - 3.0)) + r.uniform(-0.08, 0.08), int(r.uniform(2.0, H - 3.0)) + r.uniform(-0.08, 0.08),
              r.uniform(3.0, 4.0), s, s, r.uniform(0.93, 0.95), 0.0)
    tags += [1] * (12 if aa else 0) + [2] * 8 + [3] * 8 + [4] * 6 + [5] * 6 + [6] * 6
    placed = b.splats()
    # the sizes above are the ones the rasterizer sees: the inputs are those divided by scale_modifier (the option under test is
    # the factor, not a cloud of sub-pixel splats at 0.5)
    placed["scales"], sp["scales"] = placed["scales"] / mod, sp["scales"] / mod
    sp = {k: torch.cat([sp[k], placed[k]]).contiguous() for k in sp}
    P = len(tags)
    g = torch.Generator().manual_seed(seed + 99)
    # (coefficient spread per degree: wide enough at the low degrees for a few per cent of the results to fall below 0)
    sh = torch.randn(P, M, generator=g) * (1.2, 0.8, 0.5, 0.5)[degree] if degree is not None else None
    isolated = np.full(P, -1)
    if degree:
        # isolated coefficients: random splats whose only coefficient is one active k >= 1, at 40 with the sign that makes its
        # term positive -- the colour (and dL_dsh[k]) IS that term: an error of one constant or one basis function is not
        # averaged away by fifteen other terms.
        nb = (degree + 1) ** 2
        d = TR.sh_direction(sp["means3D"].to(DT), cam.camera_center.to(DT))
        basis = torch.stack(TR.sh_basis(d[:, 0], d[:, 1], d[:, 2], degree), 1)
        f64 = lambda v: v.to(DT)
        cpx, cpy, _, _, ctz, _ = TR.preprocess_2d(f64(sp["means3D"]), f64(sp["opacities"]), f64(sp["scales"]), f64(sp["rotations"]),
                                                  f64(cam.world_view_transform), f64(cam.full_proj_transform),
                                                  math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), H, W)
        on_screen = torch.nonzero((ctz[:n_random] > 0.2) & (cpx[:n_random] > 1) & (cpx[:n_random] < W - 2) & (cpy[:n_random] > 1)
                                  & (cpy[:n_random] < H - 2))[:, 0].tolist()
        for j, i in enumerate(on_screen[:3 * (nb - 1)]):   # three on-screen random splats per k
            k = 1 + j % (nb - 1)
            sh[i], isolated[i] = 0.0, k
            sh[i, k] = 40.0 * (1.0 if basis[i, k] >= 0 else -1.0)
    cov = None
    if use_cov:
        # R S^2 R^T of the scene's splats, but 40 symmetric positive-definite matrices A A^T that are not of that form, one
        # of them flat (a zero z row and column)
        Sg = TR._quat_to_R(sp["rotations"]) @ torch.diag_embed(sp["scales"] ** 2) @ TR._quat_to_R(sp["rotations"]).transpose(1, 2)
        A = torch.randn(40, 3, 3, generator=g) * 0.02
        Sg[:40] = A @ A.transpose(1, 2)
        Sg[7, 2, :] = 0.0
        Sg[7, :, 2] = 0.0
        cov = torch.stack([Sg[:, 0, 0], Sg[:, 0, 1], Sg[:, 0, 2], Sg[:, 1, 1], Sg[:, 1, 2], Sg[:, 2, 2]], 1).contiguous()
    opt = Options(sh, degree or 0, aa, mod, cov)
    keep = ~splat_failures(sp, cam, H, W, outside=True, opt=opt).any(1)
    tag = np.array(tags)
    while int(keep.sum()) % 64 == 0:
        keep[np.nonzero(keep & (tag == 0))[0][-1]] = False
    kt = torch.from_numpy(keep)
    sp, opt = {k: v[kt].contiguous() for k, v in sp.items()}, opt.subset(kt)
    assert not splat_failures(sp, cam, H, W, outside=True, opt=opt).any()
    sc = Scene(f"option_{name}", built=(sp, cam, H, W, seed))
    sc.opt, sc.render_geo, sc.tag, sc.isolated = opt, render_geo, tag[keep], isolated[keep]
    sc.custom = (np.arange(P) < 40)[keep] & use_cov                      # the rows whose covariance is an A A^T
    sc.flat = int(np.nonzero(keep)[0].tolist().index(7)) if use_cov and keep[7] else None
    assert sc.P > 256 and sc.P % 64 != 0, sc.P
    return sc


def option_edges(sc, t):
    """Asserts that the scene holds the edges its option set is there for (t: a Truth of it) and returns their counts."""
    o, tag = sc.opt, sc.tag
    vis = t.radii > 0
    drawn = np.zeros(sc.P, bool)
    drawn[t.order[t.blended.any(1)]] = True
    n = dict(P=sc.P, visible=int(vis.sum()), blended=int(drawn.sum()), culled=int((~vis).sum()),
             near=int((~vis & (tag == 4)).sum()), empty_rect=int((~vis & (t.tz > 0.2)).sum()))
    assert n["near"] >= 5 and n["empty_rect"] >= 5 and n["culled"] >= 10, n
    if o.sh is not None:
        n.update(clamped=int((vis & t.clampd).sum()), unclamped=int((vis & ~t.clampd).sum()))
        assert n["clamped"] >= 5 and n["unclamped"] >= 20, n
        assert o.sh.shape[1] == OPTION_SETS[sc.name[7:]][3] >= (o.degree + 1) ** 2
        n["isolated"] = int((drawn & (sc.isolated > 0)).sum())     # every active k >= 1 alone in a drawn, unclamped splat
        assert set(sc.isolated[drawn & ~t.clampd]) >= set(range(1, (o.degree + 1) ** 2)), sorted(set(sc.isolated[drawn]))
    if o.antialiasing:
        below, above = vis & (t.aa_ratio <= 0.000025), vis & (t.aa_ratio > 0.000025)
        faint = vis & (t.opac < 1.0 / 255.0)
        n.update(below_floor=int(below.sum()), above_floor=int(above.sum()), antialiased_away=int(faint.sum()),
                 thin=int((drawn & (tag == 1)).sum()))
        assert n["below_floor"] >= 4 and n["above_floor"] >= 40 and n["antialiased_away"] >= 4 and n["thin"] >= 6, n
        assert (faint & (tag == 3)).any() and not drawn[faint].any()
        # the floor meets a gradient: below-floor splats that are blended, with a non-zero dL_dopacity (t with gradients)
        lit = below & drawn
        n["below_floor_drawn"] = int(lit.sum())
        assert n["below_floor_drawn"] >= 3 and (tag[lit] == 6).all(), n
        if t.g is not None:
            assert (t.g["dL_dopacity"][lit, 0] != 0).all()
    if o.cov3D is not None:
        n.update(not_RSSR=int((vis & sc.custom).sum()), flat=sc.flat)
        assert n["not_RSSR"] >= 20 and sc.flat is not None and vis[sc.flat], n
        c = o.cov3D[sc.flat]
        assert c[2] == 0 and c[4] == 0 and c[5] == 0 and c[0] > 0 and c[3] > 0
    return n


def scene_grads(scene, which=(True, True, True), mask=None):
    """Seeded upstream gradients (dL/dcolour, dL/dinvdepth, dL/dall_map); None where `which` is False.  `mask` [H, W]: the
    undecided pixels, where all three are zero -- every pair of such a pixel then contributes alpha * sum_ch d_ch (...) = 0 to
    every gradient, exactly and in any arithmetic, whichever way a kernel decides there."""
    g = torch.Generator().manual_seed(scene.seed + 7)
    H, W = scene.H, scene.W
    d = (torch.randn(1, H, W, generator=g), torch.randn(1, H, W, generator=g), torch.randn(4, H, W, generator=g))
    if mask is not None and mask.any():
        keep = torch.from_numpy(~mask)
        d = tuple(t * keep for t in d)
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


COV6 = torch.tensor([[0, 1, 2], [1, 3, 4], [2, 4, 5]])    # cov3D_precomp [P, 6] -> the symmetric [P, 3, 3]: cov6[:, COV6]


class Options:
    """The per-splat options of GaussianRasterizer that the compositor scenes leave at their defaults: `sh` [P, M] float32
    spherical-harmonic coefficients evaluated at `degree` (None: colors_precomp), `antialiasing`, `scale_modifier`, `cov3D`
    [P, 6] float32 (None: scales and rotations)."""

    def __init__(self, sh=None, degree=0, antialiasing=False, scale_modifier=1.0, cov3D=None):
        self.sh, self.degree, self.antialiasing, self.scale_modifier, self.cov3D = sh, degree, antialiasing, scale_modifier, cov3D

    def subset(self, keep):
        f = lambda t: None if t is None else t[keep].contiguous()
        return Options(f(self.sh), self.degree, self.antialiasing, self.scale_modifier, f(self.cov3D))


def quirk16(g):
    """A per-coefficient gradient [P, M] as the operator returns it: the kernel writes P * M floats into the
    head of a [P, M, 3] buffer, which autograd sums onto the [P, M, 1] input."""
    P, M = g.shape
    flat = np.zeros(P * M * 3)
    flat[:P * M] = g.reshape(-1)
    return flat.reshape(P, M, 3).sum(-1)


def rows_of(splats, g, name):
    """The elements of gradient tensor `g` that only the splats of the [P] mask `splats` write: their rows -- for dL_dsh,
    whose layout quirk 16 scrambles, the elements no other splat's coefficient is summed into."""
    if name != "dL_dsh":
        return np.broadcast_to(splats.reshape((-1,) + (1,) * (g.ndim - 1)), g.shape)
    return quirk16(np.broadcast_to((~splats)[:, None], g.shape).astype(np.float64)) == 0


def sh_terms(sh, means3D, campos, degree):
    """(result [P], magnitude [P]) in float64: the spherical-harmonic sum + 0.5 before its clamp at 0, and the sum of the
    magnitudes of its terms, |C0 sh_0| + sum_k |c_k basis_k|_mag |sh_k| + 0.5."""
    d = TR.sh_direction(means3D.to(DT), campos.to(DT)).numpy()
    s = sh.to(DT).numpy().reshape(len(d), -1)
    b = TR.sh_basis(d[:, 0], d[:, 1], d[:, 2], degree)
    bm = TR.sh_basis(d[:, 0], d[:, 1], d[:, 2], degree, mag=True)
    res = sum(bk * s[:, k] for k, bk in enumerate(b)) + 0.5
    mag = sum(bk * np.abs(s[:, k]) for k, bk in enumerate(bm)) + 0.5
    return res, mag


def aa_terms(cov2d):
    """(ratio [P], hrel [P]) of the antialiasing factor h = sqrt(max(0.000025, ratio)), ratio = det0 / det with det0 =
    a0 c0 - b0^2 of the undilated and det = a c - b^2 of the dilated 2D covariance: hrel = the relative rounding error of h
    in units of eps, 1/2 ((|a0 c0| + b0^2) / |det0| + (a c + b^2) / det) -- det0 cancels for thin splats."""
    a, b, c = np.asarray(cov2d, np.float64).T
    a0, c0 = a - 0.3, c - 0.3
    det0, det = a0 * c0 - b * b, a * c - b * b
    with np.errstate(divide="ignore", invalid="ignore"):
        hrel = 0.5 * ((np.abs(a0 * c0) + b * b) / np.abs(det0) + (a * c + b * b) / det)
    return det0 / det, hrel


def _jac(P, outs, xs):
    """[P, len(outs), sum of the xs' row sizes]: per-splat Jacobian of per-splat outputs (rows are independent)."""
    rows = []
    for o in outs:
        gs = torch.autograd.grad(o.sum(), xs, retain_graph=True, allow_unused=True)
        rows.append(np.concatenate([(np.zeros(tuple(x.shape)) if g is None else g.numpy()).reshape(P, -1) for g, x in zip(gs, xs)], 1))
    return np.stack(rows, 1)


class Truth:
    """One float64 forward + backward of dense_render on a scene variant with one set of upstream gradients."""

    def __init__(self, scene, sp, grads=None, render_geo=True, opt=None):
        """`opt`: an Options (spherical-harmonic colours, antialiasing, scale_modifier, cov3D_precomp); None = none of them,
        through the call dense_render always had."""
        self.scene, self.render_geo, self.opt = scene, render_geo, opt
        H, W, P = scene.H, scene.W, scene.P
        ins = {k: v.to(DT).requires_grad_(grads is not None) for k, v in sp.items()}
        off = torch.zeros(P, 2, dtype=DT, requires_grad=grads is not None)
        cam = scene.cam
        tr = {}
        kw = {}
        if opt is not None:
            kw = dict(scale_modifier=opt.scale_modifier, antialiasing=opt.antialiasing, reference_backward=True)
            if opt.sh is not None:
                ins["sh"] = opt.sh.to(DT).requires_grad_(grads is not None)
                kw.update(sh=ins["sh"], sh_degree=opt.degree, campos=cam.camera_center.to(DT))
            if opt.cov3D is not None:
                ins["cov3D"] = opt.cov3D.to(DT).requires_grad_(grads is not None)
                kw.update(cov3D=ins["cov3D"][:, COV6])
        col, radii, invd, amap = TR.dense_render(
            ins["means3D"], ins["opacities"], ins["scales"], ins["rotations"], ins["colors"], ins["all_map"],
            cam.world_view_transform.to(DT), cam.full_proj_transform.to(DT), scene.tfx, scene.tfy, H, W, scene.bg.to(DT),
            means2D_ndc_offset=off, trace=tr, **kw)
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
        # what the options add: to a pair's relative alpha error (the antialiasing factor's own rounding, hrel) and, for
        # spherical-harmonic colours (sh_stage), the sum of the magnitudes of a colour's terms (colmag)
        self.hrel, self.colmag, self.sh_stage = np.zeros(P), np.zeros(P), False
        if opt is not None:
            self._option_state(tr)
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
            if "sh" in ins:
                self.g["dL_dsh"] = quirk16(z(ins["sh"]))
            if "cov3D" in ins:
                self.g["dL_dcov3D"] = z(ins["cov3D"])
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
        # (with antialiasing the opacity carries the relative error eps hrel of its factor h into every alpha of the splat)
        self.m_rel = self.m + self.hrel[o][:, None]
        self.X = (bl * self.al / (1 - self.al) * self.m_rel).sum(0)
        self.omega = 1 + self.m_rel + self.X[None, :] + self.n_front
        self.T_final = (self.Tb[-1] * (1 - self.al[-1])) if len(o) else np.ones(self.scene.H * self.scene.W)
        self.n_blended = bl.sum(0)

    def _channels(self):
        """[(name, v [N], |v| [N], |bg|)] of the channels the forward accumulates."""
        o = self.order
        ch = [("color", self.colors[o], np.abs(self.colors[o]), float(self.scene.bg[0])),
              ("invdepth", 1.0 / self.tz[o], np.abs(1.0 / self.tz[o]), 0.0)]
        if self.render_geo:
            ch += [(f"all_map{k}", self.all_map[o, k], np.abs(self.all_map[o, k]), 0.0) for k in range(4)]
        return ch

    def _chanmag(self, vmag, bg):
        """T |v_s| + (sum_{t behind} |v_t| w_t + |bg| T_final) / (1 - alpha_s): the magnitudes of d out / d alpha_s's terms."""
        t = vmag[:, None] * self.w
        behind = np.cumsum(t[::-1], 0)[::-1] - t + abs(bg) * self.T_final[None, :]
        return self.Tb * vmag[:, None] + behind / (1 - self.al)

    def image_bounds(self, K=None):
        K = globals()["K"] if K is None else K
        H, W = self.scene.H, self.scene.W
        out = {}
        for name, v, vmag, bg in self._channels():
            sens = (self.al * self._chanmag(vmag, bg) * (1 + self.m_rel)).sum(0)
            mag = (vmag[:, None] * self.w).sum(0) + abs(bg) * self.T_final
            out[name] = (K * EPS * (sens + (self.n_blended + 2) * mag)).reshape(H, W)
        if self.sh_stage:   # the spherical-harmonic colours' own rounding, K_SH eps colmag per splat, weighted like the colours
            out["color"] = out["color"] + ((K * K_SH / globals()["K"]) * EPS * (self.colmag[self.order][:, None] * self.w).sum(0)).reshape(H, W)
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
        for name, v, vmag, bg in self._channels():
            if ups[name] is not None:
                gmag += np.abs(ups[name])[None, :] * self._chanmag(vmag, bg)
        if self.sh_stage and ups["color"] is not None:   # the colours' own rounding (K_SH eps colmag) in dL/dalpha's two halves
            gmag += (K_SH / globals()["K"]) * np.abs(ups["color"])[None, :] * self._chanmag(self.colmag[o], 0.0)
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
        if self.opt is not None:
            # the float32 pixel-space centre is rounded at eps |px| (not eps |dx|): in the moments of g that is eps |px| times the
            # derivative of the moment's weight by dx.  Sections 4 and 5 leave it to K, which holds while |dx| is not small
            # against eps |px| / eps; the option scenes place drawn splats within 0.08 px of a pixel centre (the C oracle's
            # dL_dmeans2D 44 x outside the bound without this term).
            # px passes four roundings at its own magnitude after the projection (p_hom.x p_w, + 1, W, - 1): 4 eps |px|, taken
            # 4 x as the K rule takes a measured error: 16 eps |px| = K / 4, not K eps |px|
            apx, apy = np.abs(self.px[o])[:, None], np.abs(self.py[o])[:, None]
            B2 = B2 + (K / globals()["K"]) * 16.0 * EPS * np.stack([(gmag * (np.abs(A) * apx + np.abs(B) * apy)).sum(1), (gmag * (np.abs(C) * apy + np.abs(B) * apx)).sum(1),
                                          (gmag * np.abs(dx) * apx).sum(1), (gmag * (np.abs(dx) * apy + np.abs(dy) * apx)).sum(1),
                                          (gmag * np.abs(dy) * apy).sum(1), np.zeros(len(o))], 1)
        G2f, B2f = full(G2, (P, 6)), full(B2, (P, 6))
        half = np.array([0.5 * W, 0.5 * H])
        Gd["dL_dmeans2D"] = np.concatenate([G2f[:, :2] * half, np.zeros((P, 1))], 1)
        Bd["dL_dmeans2D"] = np.concatenate([B2f[:, :2] * half, np.zeros((P, 1))], 1)
        self.G2, self.B2 = G2f, B2f
        if self.opt is not None:
            self._option_bounds(K, Bd, Gd, G2f, B2f, J)
            return Bd, Gd
        J, Jmag = self.jacobian() if J is None else J
        G3 = np.einsum("pij,pi->pj", J, G2f)
        B3 = np.einsum("pij,pi->pj", Jmag, B2f) + K * EPS * np.einsum("pij,pi->pj", Jmag, np.abs(G2f))
        for name, sl in (("dL_dmeans3D", slice(0, 3)), ("dL_dscales", slice(3, 6)), ("dL_drotations", slice(6, 10))):
            Gd[name], Bd[name] = G3[:, sl], B3[:, sl]
        return Bd, Gd

    # ---- the per-splat options (module docstring: "Options")
    def _opt_pre(self, m, op, s, q, cov):
        sc, o = self.scene, self.opt
        return TR.preprocess_2d(m, op, s, q, sc.cam.world_view_transform.to(DT), sc.cam.full_proj_transform.to(DT), sc.tfx, sc.tfy,
                                sc.H, sc.W, o.scale_modifier, None, o.antialiasing, cov, True)

    def _option_state(self, tr):
        """hrel, colmag and the decisions the options add (clampd: the spherical-harmonic result is negative)."""
        sc, o = self.scene, self.opt
        P = sc.P
        self.clampd = np.zeros(P, bool)
        if o.sh is not None:
            res, mag = sh_terms(o.sh, sc.sp["means3D"], sc.cam.camera_center, o.degree)
            self.clampd = res < 0
            self.colors = tr["colors"].numpy()[:, 0]
            self.colmag, self.sh_stage = np.where(self.clampd, 0.0, mag), True
        if o.antialiasing:
            cov = None if o.cov3D is None else o.cov3D.to(DT)[:, COV6]
            d = lambda k: sc.sp[k].to(DT)
            cov2d = self._opt_pre(d("means3D"), d("opacities"), d("scales"), d("rotations"), cov)[5].numpy()
            ratio, hrel = aa_terms(cov2d)
            self.aa_ratio = ratio
            self.hrel = np.where(ratio > 0.000025, hrel, 0.0)

    def jacobian_opt(self):
        """(J, Jmag), both [P, 8, 17 + M]: d (px, py, A, B, C, tz, effective opacity, colour) / d (means3D 3, scales 3,
        rotations 4, cov3D 6, opacity 1, sh M) per splat -- J by float64 autograd with the reference's two departures
        (torch_ref.preprocess_2d(reference_backward=True)), Jmag with the magnitudes of the stages multiplied as in jacobian():
            Jmag[A B C, .]           = |d conic / d Sigma| |d Sigma / d .|
            Jmag[op_eff, .]          = opacity |d h / d cov2D| |d cov2D / d Sigma| |d Sigma / d .|   (h by the reference formula)
            |d Sigma / d scales|     = |d (R (mod S)^2 R^T) / d S| / mod                             (the departure's division)
            |d Sigma / d rotations|  = |d (R (mod S)^2 R^T) / d R| |d R / d q|
            |d Sigma / d cov3D|      = 1 on the diagonal entries, 2 on the others (both symmetric entries read the input)
            Jmag[colour, means3D]    = sum_k |sh_k| |d (c_k basis_k) / d dir| |d dir / d means3D|
            Jmag[colour, sh_k]       = |c_k basis_k| (the sum of the magnitudes of its monomials)
        A clamped colour's row is zero; columns of an input the option set does not have are zero."""
        sc, o = self.scene, self.opt
        P = sc.P
        M = 0 if o.sh is None else o.sh.shape[1]
        has_cov = o.cov3D is not None
        leaf = lambda t: t.detach().to(DT).clone().requires_grad_(True)
        m, op, s, q = (leaf(sc.sp[k]) for k in ("means3D", "opacities", "scales", "rotations"))
        cov6 = leaf(o.cov3D) if has_cov else None
        campos = sc.cam.camera_center.to(DT)
        px, py, conic, opac, tz, cov2d_m = self._opt_pre(m, op, s, q, cov6[:, COV6] if has_cov else None)
        outs = [px, py, conic[:, 0], conic[:, 1], conic[:, 2], tz, opac]
        xs, cols = [m], [slice(0, 3)]
        if has_cov:
            xs, cols = xs + [cov6], cols + [slice(10, 16)]
        else:
            xs, cols = xs + [s, q], cols + [slice(3, 6), slice(6, 10)]
        xs, cols = xs + [op], cols + [slice(16, 17)]
        if M:
            sh = leaf(o.sh)
            outs.append(TR.sh_colour(sh, m, campos, o.degree)[:, 0])
            xs, cols = xs + [sh], cols + [slice(17, 17 + M)]
        Jc = _jac(P, outs, xs)
        J = np.zeros((P, 8, 17 + M))
        at = 0
        for x, c in zip(xs, cols):
            J[:, :len(outs), c] = Jc[:, :, at:at + (c.stop - c.start)]
            at += c.stop - c.start
        a = np.abs
        Jmag = a(J)
        # the covariance path, stage by stage
        if has_cov:
            Sl = leaf(cov6[:, COV6])
        else:
            ql = leaf(q)
            R = TR._quat_to_R(ql)
            J_Rq = _jac(P, [R[:, i, j] for i in range(3) for j in range(3)], [ql])                   # [P, 9, 4]
            Rl, sl = leaf(R), leaf(s)
            Sig = Rl @ torch.diag_embed((o.scale_modifier * sl) ** 2) @ Rl.transpose(1, 2)
            J_SRs = _jac(P, [Sig[:, i, j] for i in range(3) for j in range(3)], [Rl, sl])            # [P, 9, 9 + 3]
            Sl = leaf(Sig)
        pre = self._opt_pre(m.detach(), op.detach(), None, None, Sl)
        con, cov2 = pre[2], pre[5]
        stage = np.zeros((P, 4, 9))                                                                  # rows A, B, C, op_eff
        J_vS = _jac(P, [cov2[:, 0], cov2[:, 1], cov2[:, 2]], [Sl])                                   # [P, 3, 9]
        # |d conic / d cov2D| as the magnitudes of the terms of the formula the kernels evaluate (backward.cu:247-260): its
        # (denom - c_xx c_yy) cancels to -c_xy^2, which leaves eps (denom + c_xx c_yy) |dL_dconic.z| in dL_dc_xx whatever the
        # true derivative is (found on the drawn below-floor splats, 0.025 px: the C oracle 81 x outside |d conic / d Sigma|)
        cx, cxy, cy = (cov2.detach().numpy()[:, i] for i in range(3))
        den = cx * cy - cxy * cxy
        Mv = np.stack([np.stack([cy * cy, 2 * a(cxy) * cy, den + cx * cy], 1),
                       np.stack([2 * a(cxy) * cy, 2 * (den + 2 * cxy * cxy), 2 * cx * a(cxy)], 1),
                       np.stack([den + cx * cy, 2 * cx * a(cxy), cx * cx], 1)], 1) / (den * den)[:, None, None]   # [P, cov2D, conic]
        stage[:, :3] = np.maximum(a(_jac(P, [con[:, 0], con[:, 1], con[:, 2]], [Sl])), np.einsum("pvc,pvk->pck", Mv, a(J_vS)))
        J_vm = _jac(P, [cov2d_m[:, 0], cov2d_m[:, 1], cov2d_m[:, 2]], [m])                           # [P, 3, 3]
        Jmag[:, 2:5, 0:3] = np.maximum(Jmag[:, 2:5, 0:3], np.einsum("pvc,pvk->pck", Mv, a(J_vm)))
        if o.antialiasing:
            c0 = leaf(cov2 - torch.tensor([0.3, 0.0, 0.3], dtype=DT))
            h = TR._AntialiasingScaleRef.apply(c0[:, 0], c0[:, 1], c0[:, 2])
            J_hv = _jac(P, [h], [c0])                                                                # [P, 1, 3]
            stage[:, 3:] = a(op.detach().numpy()).reshape(P, 1, 1) * np.einsum("pij,pjk->pik", a(J_hv), a(J_vS))
        rows = [2, 3, 4, 6]
        if has_cov:
            F = np.zeros((9, 6))
            for i in range(3):
                for j in range(3):
                    F[3 * i + j, int(COV6[i, j])] = 1.0
            Jmag[:, rows, 10:16] = stage @ F
        else:
            Jmag[:, rows, 3:6] = np.einsum("pij,pjk->pik", stage, a(J_SRs[:, :, 9:])) / o.scale_modifier
            Jmag[:, rows, 6:10] = np.einsum("pij,pjk,pkl->pil", stage, a(J_SRs[:, :, :9]), a(J_Rq))
        if M:
            live = (~self.clampd).astype(np.float64)
            ml = leaf(m)
            d = TR.sh_direction(ml, campos)
            J_dm = _jac(P, [d[:, 0], d[:, 1], d[:, 2]], [ml])                                        # [P, 3, 3]
            dl, shd = leaf(d), o.sh.to(DT)
            dcd = np.zeros((P, 3))
            for k, bk in enumerate(TR.sh_basis(dl[:, 0], dl[:, 1], dl[:, 2], o.degree)):
                if k:
                    dcd += a(torch.autograd.grad((bk * shd[:, k]).sum(), dl, retain_graph=True)[0].numpy())
            Jmag[:, 7, 0:3] = live[:, None] * np.einsum("pj,pji->pi", dcd, a(J_dm))
            dn = d.detach().numpy()
            bm = np.stack(TR.sh_basis(dn[:, 0], dn[:, 1], dn[:, 2], o.degree, mag=True), 1)
            Jmag[:, 7, 17:17 + bm.shape[1]] = live[:, None] * bm
        assert (Jmag >= a(J) * (1 - 1e-9)).all()
        return J, Jmag

    def _option_bounds(self, K, Bd, Gd, G2f, B2f, J=None):
        """The per-splat backward with options: the 2D state is (px, py, A, B, C, tz, effective opacity, colour), whose last two
        gradients and bounds are the compositor's dL_dopacity and dL_dcolors (bounds of section 4); each input's gradient is
        J^T G_state with bound |J|^T B_state + K eps |J|^T |G_state| (section 5), the antialiasing factor's own rounding
        (eps hrel of h) added to the effective opacity's row."""
        o = self.opt
        J, Jmag = self.jacobian_opt() if J is None else J
        Gop, Bop = Gd["dL_dopacity"][:, 0], Bd["dL_dopacity"][:, 0]
        G8 = np.concatenate([G2f, Gop[:, None], Gd["dL_dcolors"]], 1)
        B8 = np.concatenate([B2f, (Bop + K * EPS * self.hrel * np.abs(Gop))[:, None], Bd["dL_dcolors"]], 1)
        G = np.einsum("pij,pi->pj", J, G8)
        B = np.einsum("pij,pi->pj", Jmag, B8) + K * EPS * np.einsum("pij,pi->pj", Jmag, np.abs(G8))
        for name, sl in (("dL_dmeans3D", slice(0, 3)), ("dL_dscales", slice(3, 6)), ("dL_drotations", slice(6, 10))):
            Gd[name], Bd[name] = G[:, sl], B[:, sl]
        if o.antialiasing:   # (without it the effective opacity IS the input: the compositor's own gradient and bound)
            Gd["dL_dopacity"], Bd["dL_dopacity"] = G[:, 16:17], B[:, 16:17]
        if o.cov3D is not None:
            Gd["dL_dcov3D"], Bd["dL_dcov3D"] = G[:, 10:16], B[:, 10:16]
        if o.sh is not None:
            # dL_dsh[k] = c_k basis_k dL_dcolour: the compositor's bound of dL_dcolour (at K_DL_DSH) and the basis function's
            # own rounding (the spherical-harmonic stage, K_SH eps), both times |c_k basis_k|_mag
            k0 = globals()["K"]
            per = (K_DL_DSH / k0) * Bd["dL_dcolors"] + (K * K_SH / k0) * EPS * np.abs(Gd["dL_dcolors"])
            Gd["dL_dsh"], Bd["dL_dsh"] = quirk16(G[:, 17:]), quirk16(Jmag[:, 7, 17:] * per)

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
def margins(scene, t=None, K=None, mask=None):
    """Distance of every decision of the float64 forward from its edge; the first two as multiples of the pair's own bound.
    Returns a dict of the smallest margins (check_margins holds each to its minimum).  `mask`: the scene's undecided pixels,
    whose pairs are left out of the per-pair margins (alpha, T, alpha_max)."""
    t = Truth(scene, variant(scene, "base")) if t is None else t
    out = {}
    reached, r_alpha, tested, r_T = _pair_margins(t, K)
    member = t.member
    if mask is not None and mask.any():   # the undecided pixels carry no loss and are not compared: their pairs do not count
        keep = ~mask.reshape(-1)[None, :]
        reached, tested, member = reached & keep, tested & keep, member & keep
    out["alpha"] = float(r_alpha[reached].min()) if reached.any() else np.inf
    out["T"] = float(r_T[tested].min()) if tested.any() else np.inf
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
    if (gaps == 0).any():   # ties must be bit-identical in every arithmetic: rows with bit-identical means3D (_tie_rows)
        min3 = _tie_rows(scene.sp["means3D"], scene.cam)[vis]
        for zv in np.unique(zs[1:][gaps == 0]):
            assert len(np.unique(min3[z32 == zv], axis=0)) == 1, "depth tie between different inputs"
    out["alpha_max"] = float(t.alpha_u[member].max()) if member.any() else 0.0
    m = _view_space(scene.sp["means3D"], scene.cam)
    front = t.tz > 0.2     # (a splat behind the near plane is culled whatever its x / z)
    out["clamp"] = float(min((1.3 * scene.tfx - np.abs(m[front, 0] / m[front, 2])).min() / scene.tfx,
                             (1.3 * scene.tfy - np.abs(m[front, 1] / m[front, 2])).min() / scene.tfy)) if front.any() else 1.0
    out["near"] = float(np.abs(t.tz / 0.2 - 1.0).min())
    return out


def _view_space(means3D, cam):
    """[P, 3] float64 view-space centres (for the camera at the origin with the world's axes: means3D itself, exactly)."""
    V = cam.world_view_transform.double().numpy().T
    return means3D.double().numpy() @ V[:3, :3].T + V[:3, 3]


def _tie_rows(means3D, cam):
    """What two rows must share bit for bit for their depth keys to tie in every arithmetic: means3D -- of which a camera
    whose view depth IS the world's z (the one at the origin with the world's axes) reads the z alone."""
    m = means3D.numpy()
    V = cam.world_view_transform.numpy().T
    return m[:, 2:3] if (V[2] == np.array([0.0, 0.0, 1.0, 0.0], np.float32)).all() else m


def _done_before(t):
    s = np.cumsum(t.stopped, 0)
    return (s - t.stopped) > 0


def _pair_margins(t, K=None):
    """(reached, r_alpha, tested, r_T), all [N, npix]: the pairs whose alpha >= 1/255 decision the float64 forward reached
    and that decision's distance from its edge in bounds of the pair's own alpha; the pairs whose T (1 - alpha) < 1e-4 test it
    ran and that test's distance in bounds of the pair's own T."""
    K = globals()["K"] if K is None else K
    reached = t.member & ~_done_before(t)
    a_err = K * EPS * (1 + t.m_rel)
    r_alpha = np.abs(255.0 * t.alpha_u - 1.0) / a_err
    tested = t.blended | t.stopped
    Tn = t.Tb * (1 - np.minimum(t.alpha_u, 0.99))
    t_err = K * EPS * (t.n_front + 1 + (1 + t.m_rel) * t.alpha_u / (1 - np.minimum(t.alpha_u, 0.99)) + t.X[None, :])
    r_T = np.abs(1e4 * Tn - 1.0) / t_err
    return reached, r_alpha, tested, r_T


def undecided_pixels(scene, t, K=None):
    """[H, W] bool: the pixels at which a pair the float64 forward reached sits within 4 bounds of a per-pair decision
    (alpha >= 1/255, T < 1e-4) or above the 0.97 that keeps the 0.99 clamp out of reach: there a float32 forward may
    legitimately decide the other way.  Such pixels carry no loss (scene_grads) and are left out of the image, `terminated`
    and n_contrib comparisons; check_mask limits how many a scene may have."""
    reached, r_alpha, tested, r_T = _pair_margins(t, K)
    und = (reached & (r_alpha < 4.0)) | (tested & (r_T < 4.0)) | (reached & (t.alpha_u > 0.97))
    return und.any(0).reshape(scene.H, scene.W) if len(t.order) else np.zeros((scene.H, scene.W), bool)


def check_mask(scene, mask):
    """At most 5 % of the scene's pixels and at most 16 of the 64 pixels of any quadrant of any tile are undecided; a scene
    that is not in the masked part of the table has none."""
    if not scene.masked:
        assert not mask.any(), f"{scene.name}: {int(mask.sum())} undecided pixels in a scene that must have none"
    assert mask.sum() <= 0.05 * mask.size, f"{scene.name}: {int(mask.sum())} of {mask.size} pixels undecided"
    H8, W8 = -(-scene.H // 8), -(-scene.W // 8)
    pad = np.zeros((H8 * 8, W8 * 8), bool)
    pad[:scene.H, :scene.W] = mask
    worst = int(pad.reshape(H8, 8, W8, 8).sum((1, 3)).max())
    assert worst <= 16, f"{scene.name}: {worst} undecided pixels in one quadrant"


def splat_failures(sp, cam, H, W, outside=False, opt=None):
    """[P, 6] bool ([P, 8] with `opt`, an Options), per splat, in float64: a per-splat decision inside the margin check_margins asks for -- radius ceil, tile
    rect edge, near cull, the 1.3 tan(fov) clamp, a depth key under 4 ulp from (or tied with) that of a different 3D centre,
    opacity in the slack of the 1/255 cut.  These are cleared where the scene is built (Builder.clear), never masked.
    `outside`: also flag what margins() has no word on because the constructed scenes do not have it -- a rect edge within
    1e-4 of the grid's far side from beyond, and any decision of a splat the float64 forward culls off-screen.
    With `opt` the 2D state is the options' (the opacity of the 1/255 cut is the antialiased one) and two columns follow: the
    spherical-harmonic result within 8 bounds of 0 (the `clamped` flag), the antialiasing ratio within 8 bounds (at least
    1e-3 relative) of its floor 0.000025."""
    tfx, tfy = math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5)
    d = lambda v: v.to(DT)
    kw = {} if opt is None else dict(scale_modifier=opt.scale_modifier, antialiasing=opt.antialiasing,
                                     cov3D=None if opt.cov3D is None else d(opt.cov3D)[:, COV6])
    px, py, _, opac, tz, cov = (v.numpy() for v in TR.preprocess_2d(
        d(sp["means3D"]), d(sp["opacities"]), d(sp["scales"]), d(sp["rotations"]), d(cam.world_view_transform),
        d(cam.full_proj_transform), tfx, tfy, H, W, **kw))
    P = len(tz)
    a, b, c = cov.T
    mid = 0.5 * (a + c)
    rad = 3.0 * np.sqrt(mid + np.sqrt(np.maximum(mid * mid - (a * c - b * b), 0.1)))
    R = np.ceil(rad)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    front = tz > 0.2
    rect = np.stack([np.clip(np.trunc(q), 0, g) for q, g in (((px - R) / 16, gx), ((py - R) / 16, gy), ((px + R + 15) / 16, gx),
                                                              ((py + R + 15) / 16, gy))], 1)
    vis = front & ((rect[:, 2] - rect[:, 0]) * (rect[:, 3] - rect[:, 1]) > 0)
    judged = front if outside else vis
    fail = np.zeros((P, 6 if opt is None else 8), bool)
    if opt is not None and opt.sh is not None:
        res, mag = sh_terms(opt.sh, sp["means3D"], cam.camera_center, opt.degree)
        fail[:, 6] = judged & (np.abs(res) <= 8.0 * K * EPS * mag)
    if opt is not None and opt.antialiasing:
        ratio, hrel = aa_terms(cov)
        with np.errstate(invalid="ignore"):
            fail[:, 7] = judged & ~(np.abs(ratio - 0.000025) > np.maximum(16.0 * K * EPS * hrel * np.abs(ratio), 0.000025 * 1e-3))
    fail[:, 0] = judged & (np.minimum(np.ceil(rad) - rad, rad - np.floor(rad)) / rad < 1e-5)
    for cc, gmax in ((px, gx), (py, gy)):
        for q in ((cc - R) / 16, (cc + R + 15) / 16):
            inside = (q > 0) & (q < gmax + (1e-3 if outside else 0.0))
            fail[:, 1] |= judged & inside & (np.abs(q - np.round(q)) < 1e-4)
    fail[:, 2] = np.abs(tz / 0.2 - 1.0) < 0.01
    m = _view_space(sp["means3D"], cam)
    with np.errstate(divide="ignore", invalid="ignore"):
        fail[:, 3] = front & ~((1.3 * tfx - np.abs(m[:, 0] / m[:, 2]) >= 0.01 * tfx) & (1.3 * tfy - np.abs(m[:, 1] / m[:, 2]) >= 0.01 * tfy))
    ids = np.nonzero(judged)[0]
    z32 = tz[ids].astype(np.float32)
    o = np.argsort(z32, kind="stable")
    key = z32[o].view(np.int32).astype(np.int64)
    m3 = _tie_rows(sp["means3D"], cam)[ids[o]]
    for k in np.nonzero(np.diff(key) < 4)[0]:   # the later row of a close pair (a run of ties flags every row after its first)
        first = k
        while first > 0 and key[first - 1] == key[k]:
            first -= 1
        if key[k + 1] != key[k] or (m3[k + 1] != m3[first]).any():
            fail[ids[o[k + 1]], 4] = True
    with np.errstate(divide="ignore"):   # (quadrant_lists' two assertions on the opacity)
        fail[:, 5] = judged & (((opac < 1.0 / 255.0) & (opac >= 0.5 / 255.0)) |
                               ((opac >= 1.0 / 255.0) & (2.0 * np.log(255.0 * opac) <= 0.05)))
    return fail


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
    the same way (common.h::tile_reach_det drops it).  Where the table names no quadrant lengths the undetermined entries are
    counted instead: `slack` per (splat, quadrant), `tile_slack` per splat that neither reaches a quadrant nor clears the tile
    -- only the latter leave the tile's LIST undetermined."""
    t = Truth(scene, variant(scene, "base")) if t is None else t
    # a scene whose table entry names no lengths (broad splats over many tiles: something always sits between the two cuts)
    # only COUNTS its undetermined entries ("slack"); positions in such a tile's list are then not compared
    strict = scene.expect is not None if strict is None else strict
    gx, gy = (scene.W + 15) // 16, (scene.H + 15) // 16
    out = {}
    yy, xx = np.mgrid[0:8, 0:8]
    for tile in range(gx * gy):
        ty, tx = divmod(tile, gx)
        ids, quads, slack, tile_slack = [], [[], [], [], []], 0, 0
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
                tile_slack += v < 2.0 * tau2
        out[tile] = dict(list=ids, quadrants=quads, slack=int(slack), tile_slack=int(tile_slack))
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
        # (a masked scene's tile list is determinate wherever every splat either reaches a quadrant or clears the whole tile:
        # the list positions do not depend on which quadrant lists a splat in a quadrant's slack joins)
        if d["tile_slack"] if scene.masked else d["slack"]:
            out[pix] = -1   # undetermined list: no position to compare
            continue
        for pos, s in enumerate(d["list"], 1):
            bl = t.blended[rank[s]][pix]
            out[pix[bl]] = pos
    return out.reshape(H, W)
