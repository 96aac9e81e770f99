"""Shared by tests/test_edge_detect_cpu.py and tests/test_edge_detect_gpu.py: seeded photographs, hand-made gradient fields
with their hand-written results, a plain-loop float64 restatement of the gradients, and two tiny scans on disk."""
import math
import os

import numpy as np
import torch

LOW, HIGH, SIGMA = 0.05, 0.15, 1.4
T = np.float32(0.41421357)


# ------------------------------------------------------------------------------------------------ (a) (b) (c) photographs
def photograph(seed, height, width, channels):
    """A smooth random field (a few random sinusoids per channel) with a few filled polygons on it, uint8 [H,W,C] ([H,W] for
    channels == 0).  A fourth channel is random alpha."""
    from PIL import Image, ImageDraw
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:height, 0:width].astype(np.float64)
    planes = []
    for _ in range(3):
        f = np.zeros((height, width))
        for _ in range(4):
            kx, ky, ph = rng.uniform(-0.25, 0.25), rng.uniform(-0.25, 0.25), rng.uniform(0, 2 * math.pi)
            f += rng.uniform(0.1, 0.3) * np.sin(kx * xx + ky * yy + ph)
        planes.append(np.clip(0.5 + 0.5 * f, 0, 1))
    img = Image.fromarray((np.stack(planes, -1) * 255).round().astype(np.uint8), mode="RGB")
    draw = ImageDraw.Draw(img)
    for _ in range(3):
        cx, cy = rng.uniform(0.25, 0.75) * width, rng.uniform(0.25, 0.75) * height
        pts = [(cx + rng.uniform(-0.4, 0.4) * width, cy + rng.uniform(-0.4, 0.4) * height) for _ in range(rng.integers(3, 6))]
        dark = rng.integers(0, 2) == 0      # well off the ground's mid grey either way
        draw.polygon(pts, fill=tuple(int(v) for v in (rng.integers(0, 50, 3) if dark else rng.integers(206, 256, 3))))
    rgb = np.array(img, dtype=np.uint8)
    if channels == 3:
        return rgb
    if channels == 4:
        return np.concatenate([rgb, rng.integers(0, 256, (height, width, 1), dtype=np.uint8)], -1)
    gray = np.array(img.convert("L"), dtype=np.uint8)
    return gray if channels == 0 else gray[:, :, None]


def small_views():
    """(a): 37x29 and 70x45 (width x height) views, C = 1 ([H,W] and [H,W,1]), 3 and 4 in one batch.  70 columns and 29 / 45
    rows cross the 64x16 tiles of the kernels in both directions."""
    return [photograph(1, 29, 37, 3), photograph(2, 45, 70, 0), photograph(3, 45, 70, 4), photograph(4, 29, 37, 1),
            photograph(5, 45, 70, 3)]


DEGENERATE_SIGMA = 2.0   # radius 6: wider than every one of these


def degenerate_views():
    """(b): 1x1, 1x40, 40x1 and 5x4 (height x width)."""
    rng = np.random.default_rng(11)
    return [rng.integers(0, 256, (1, 1, 3), dtype=np.uint8), rng.integers(0, 256, (1, 40), dtype=np.uint8),
            rng.integers(0, 256, (40, 1, 4), dtype=np.uint8), rng.integers(0, 256, (5, 4, 1), dtype=np.uint8)]


def batch_views(n=26):
    """(c): more views than one call's table holds, 9x7 (width x height) each."""
    return [photograph(100 + k, 7, 9, (3, 0, 4)[k % 3]) for k in range(n)]


def disc_image(seed=5):
    """96x80 (width x height): a dark disc of radius 25 about (48, 40) on a light ground, +-2/255 of noise."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:80, 0:96]
    base = np.where(np.hypot(xx - DISC_CX, yy - DISC_CY) <= DISC_R, 25, 230)
    return (base + rng.integers(-2, 3, base.shape)).astype(np.uint8)


DISC_CX, DISC_CY, DISC_R = 48.0, 40.0, 25.0


# ------------------------------------------------------------------------------------------------ gradients, plain loops
def gradients_loop_f64(image, sigma):
    """The rule of the detector's gradients written out pixel by pixel with Python floats (float64): luminance, the taps
    (float64, normalised, rounded to float32), rows then columns with clamped coordinates, Sobel / 4 with clamped
    coordinates, magnitude.  Written for the tests; shares no code with the package."""
    a = np.asarray(image)
    a = a[:, :, None] if a.ndim == 2 else a
    H, W, C = a.shape
    r = min(int(math.ceil(3.0 * sigma)), 12)
    if r == 0:
        taps = [1.0]
    else:
        w = [math.exp(-(o * o) / (2.0 * sigma * sigma)) for o in range(-r, r + 1)]
        taps = [float(np.float32(v / sum(w))) for v in w]
    cl = lambda v, n: 0 if v < 0 else (n - 1 if v > n - 1 else v)
    lum = [[(float(a[y, x, 0]) if C == 1 else 0.299 * float(a[y, x, 0]) + 0.587 * float(a[y, x, 1]) + 0.114 * float(a[y, x, 2]))
            / 255.0 for x in range(W)] for y in range(H)]
    rows = [[sum(taps[o + r] * lum[y][cl(x + o, W)] for o in range(-r, r + 1)) for x in range(W)] for y in range(H)]
    sm = [[sum(taps[o + r] * rows[cl(y + o, H)][x] for o in range(-r, r + 1)) for x in range(W)] for y in range(H)]
    S = lambda x, y: sm[cl(y, H)][cl(x, W)]
    gx, gy = np.zeros((H, W)), np.zeros((H, W))
    for y in range(H):
        for x in range(W):
            gx[y, x] = ((S(x + 1, y - 1) + 2 * S(x + 1, y) + S(x + 1, y + 1)) - (S(x - 1, y - 1) + 2 * S(x - 1, y) + S(x - 1, y + 1))) / 4
            gy[y, x] = ((S(x - 1, y + 1) + 2 * S(x, y + 1) + S(x + 1, y + 1)) - (S(x - 1, y - 1) + 2 * S(x, y - 1) + S(x + 1, y - 1))) / 4
    return gx, gy, np.sqrt(gx * gx + gy * gy)


# ------------------------------------------------------------------------------------------------ (d) hysteresis by hand
class TraceCase:
    """gx = m, gy = 0, thin = False: `kept` is the hand-written set of pixels with a non-zero response."""

    def __init__(self, name, m, kept):
        self.name, self.m, self.kept = name, np.ascontiguousarray(m, np.float32), np.asarray(kept, bool)
        assert self.m.shape == self.kept.shape


WEAK, STRONG = np.float32(0.1), np.float32(0.2)   # LOW <= WEAK < HIGH <= STRONG


def serpentine(strong=True):
    """130x70 (width x height): rows 2, 6, ..., 66 from column 2 to 127, joined alternately at their right and left ends: one
    chain of 2200-odd pixels through ten of the fifteen tiles (64x16) of the image, a strong pixel at its start only."""
    H, W = 70, 130
    chain = np.zeros((H, W), bool)
    ys = list(range(2, 67, 4))
    for k, y in enumerate(ys):
        chain[y, 2:128] = True
        if k + 1 < len(ys):
            chain[y:y + 5, 127 if k % 2 == 0 else 2] = True
    m = np.where(chain, WEAK, np.float32(0))
    if strong:
        m[2, 2] = STRONG
    return TraceCase("serpentine" if strong else "serpentine_without_a_strong_pixel", m, chain if strong else np.zeros_like(chain))


def diagonal_touch():
    """20x8: the run (2..10, 3) with a strong start, the run (11..18, 4) that touches its end only diagonally -- kept -- and
    the run (2..10, 6), two rows below the first -- never reached."""
    m = np.zeros((8, 20), np.float32)
    m[3, 2:11] = WEAK
    m[3, 2] = STRONG
    m[4, 11:19] = WEAK
    m[6, 2:11] = WEAK
    kept = np.zeros((8, 20), bool)
    kept[3, 2:11] = True
    kept[4, 11:19] = True
    return TraceCase("diagonal_touch", m, kept)


def corners_and_borders():
    """20x12: a strong pixel in every corner (kept alone); on each border a weak pixel with a strong one diagonally inside
    (both kept); one weak border pixel on its own (dropped)."""
    H, W = 12, 20
    m = np.zeros((H, W), np.float32)
    kept = np.zeros((H, W), bool)
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        m[y, x] = STRONG
        kept[y, x] = True
    for (by, bx), (sy, sx) in (((0, 9), (1, 10)), ((H - 1, 9), (H - 2, 8)), ((5, 0), (6, 1)), ((5, W - 1), (4, W - 2))):
        m[by, bx], m[sy, sx] = WEAK, STRONG
        kept[by, bx] = kept[sy, sx] = True
    m[0, 4] = WEAK
    return TraceCase("corners_and_borders", m, kept)


def inclusive_thresholds():
    """12x5, row 1: exactly `low` beside exactly `high` -- both kept; row 3: one ulp under `low` beside `high` -- only the
    strong one; columns 8..9 of row 1: exactly `low` beside one ulp under `high` -- a component without a strong pixel."""
    low, high = np.float32(LOW), np.float32(HIGH)
    m = np.zeros((5, 12), np.float32)
    kept = np.zeros((5, 12), bool)
    m[1, 2], m[1, 3] = low, high
    kept[1, 2] = kept[1, 3] = True
    m[3, 2], m[3, 3] = np.nextafter(low, np.float32(0)), high
    kept[3, 3] = True
    m[1, 8], m[1, 9] = low, np.nextafter(high, np.float32(0))
    return TraceCase("inclusive_thresholds", m, kept)


def trace_cases():
    return [serpentine(True), serpentine(False), diagonal_touch(), corners_and_borders(), inclusive_thresholds()]


# ------------------------------------------------------------------------------------------------ (e) thinning by hand
class ThinCase:
    """A 7x7 field with one gradient (gx, gy) everywhere; `values` {(x, y): m}, zero elsewhere; `survivors` the hand-derived
    set of (x, y) whose m' is not 0.  Every value is >= HIGH, so the survivors are exactly the pixels with response 1."""

    def __init__(self, name, gx, gy, values, survivors):
        self.name = name
        self.gx = np.full((7, 7), gx, np.float32)
        self.gy = np.full((7, 7), gy, np.float32)
        self.m = np.zeros((7, 7), np.float32)
        for (x, y), v in values.items():
            self.m[y, x] = v
        self.kept = np.zeros((7, 7), bool)
        for x, y in survivors:
            self.kept[y, x] = True


def _sector(first, second, decoys):
    """The centre (3, 3) = 0.3 between its `first` = 0.2 and `second` = 0.25 neighbour, which it beats and which lose to
    it, and two decoys of 0.9 beside the centre, off the pair's line, that would beat it if the wrong pair were
    compared; the decoys' own pairs are zeros."""
    return {(3, 3): 0.3, first: 0.2, second: 0.25, decoys[0]: 0.9, decoys[1]: 0.9}, {(3, 3), decoys[0], decoys[1]}


def thin_cases():
    up = np.nextafter(T, np.float32(1))
    cases = []
    # the four sectors, tested in the rule's order: |gy| <= T |gx|; |gx| <= T |gy|; gx gy > 0; the rest
    cases.append(ThinCase("horizontal", 1.0, 0.0, *_sector((2, 3), (4, 3), ((3, 2), (3, 4)))))
    cases.append(ThinCase("vertical", 0.0, 1.0, *_sector((3, 2), (3, 4), ((2, 3), (4, 3)))))
    cases.append(ThinCase("diagonal_down", 1.0, 1.0, *_sector((2, 2), (4, 4), ((2, 4), (4, 2)))))
    cases.append(ThinCase("diagonal_down_negative", -1.0, -1.0, *_sector((2, 2), (4, 4), ((2, 4), (4, 2)))))
    cases.append(ThinCase("diagonal_up", 1.0, -1.0, *_sector((4, 2), (2, 4), ((2, 2), (4, 4)))))
    cases.append(ThinCase("diagonal_up_mirrored", -1.0, 1.0, *_sector((4, 2), (2, 4), ((2, 2), (4, 4)))))
    # an exact tie of two pixels along the pair's line: the one that is `first` of the other survives
    cases.append(ThinCase("tie_horizontal", 1.0, 0.0, {(3, 3): 0.3, (4, 3): 0.3}, {(3, 3)}))
    cases.append(ThinCase("tie_vertical", 0.0, 1.0, {(3, 3): 0.3, (3, 4): 0.3}, {(3, 3)}))
    cases.append(ThinCase("tie_diagonal_down", 1.0, 1.0, {(3, 3): 0.3, (4, 4): 0.3}, {(3, 3)}))
    cases.append(ThinCase("tie_diagonal_up", 1.0, -1.0, {(3, 3): 0.3, (2, 4): 0.3}, {(3, 3)}))
    # exactly on a sector boundary: |gy| = T |gx| with |gx| = 1 or 2, so T |gx| is exact in float32 -- still horizontal; the
    # decoys sit on the diagonal that the next sector would compare
    cases.append(ThinCase("boundary_horizontal", 1.0, T, *_sector((2, 3), (4, 3), ((2, 2), (4, 4)))))
    cases.append(ThinCase("boundary_horizontal_twice", 2.0, np.float32(2) * T, *_sector((2, 3), (4, 3), ((2, 2), (4, 4)))))
    # one ulp past it the pair is the diagonal (2, 2), (4, 4): the centre loses to a decoy; (2, 3) and (4, 3) have zeros on
    # their own diagonals and survive, and so do the decoys ((4, 4): first (3, 3) = 0.3 < 0.9)
    cases.append(ThinCase("past_boundary_horizontal", 1.0, up,
                          {(3, 3): 0.3, (2, 3): 0.2, (4, 3): 0.25, (2, 2): 0.9, (4, 4): 0.9}, {(2, 3), (4, 3), (2, 2), (4, 4)}))
    # |gx| = T |gy|: the first test fails (1 > T T), the second holds -- vertical
    cases.append(ThinCase("boundary_vertical", T, 1.0, *_sector((3, 2), (3, 4), ((2, 2), (4, 4)))))
    cases.append(ThinCase("past_boundary_vertical", up, 1.0,
                          {(3, 3): 0.3, (3, 2): 0.2, (3, 4): 0.25, (2, 2): 0.9, (4, 4): 0.9}, {(3, 2), (3, 4), (2, 2), (4, 4)}))
    return cases


# ------------------------------------------------------------------------------------------------ tiny scans
SCAN_H, SCAN_W, SCAN_VIEWS = 40, 56, 3


def _cameras():
    from curve_gaussian_amd import synthetic as S
    return S.room_cameras(SCAN_VIEWS, SCAN_H, SCAN_W, 4)


def scan_photographs():
    return [photograph(50 + k, SCAN_H, SCAN_W, 3) for k in range(SCAN_VIEWS)]


def write_emap_scan(path):
    """An EMAP scan that holds photographs and poses only: meta_data.json and color/<i>_colors.png."""
    from PIL import Image
    from curve_gaussian_amd.scene import dataset_io as IO
    import shutil
    IO.write_emap(path, _cameras(), [torch.zeros(1, SCAN_H, SCAN_W)] * SCAN_VIEWS)
    shutil.rmtree(os.path.join(path, "edge_DexiNed"))
    os.makedirs(os.path.join(path, "color"))
    for k, img in enumerate(scan_photographs()):
        Image.fromarray(img, mode="RGB").save(os.path.join(path, "color", f"{k}_colors.png"))
    return path


def write_colmap_scan(path):
    """A COLMAP scan that holds photographs and poses only: sparse/0 and images/<i:05d>.png."""
    from PIL import Image
    from curve_gaussian_amd.scene import colmap_io as CIO
    import shutil
    pts = np.random.default_rng(0).uniform(0.2, 0.8, (30, 3))
    CIO.write_colmap(path, _cameras(), [torch.zeros(1, SCAN_H, SCAN_W)] * SCAN_VIEWS, pts)
    shutil.rmtree(os.path.join(path, "edge_DexiNed"))
    os.makedirs(os.path.join(path, "images"))
    for k, img in enumerate(scan_photographs()):
        Image.fromarray(img, mode="RGB").save(os.path.join(path, "images", f"{k:05d}.png"))
    return path
