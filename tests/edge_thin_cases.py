"""Shared inputs of the thinning tests (test_edge_thin_cpu.py, test_edge_thin_gpu.py): a brute-force Guo-Hall thinning in
Python integers, small masks, strokes, and the twelve-view drawn scan of edge_dir_cases with its detected masks dilated to
the width of a learned detector's response."""
import functools

import numpy as np

import edge_dir_cases as DC
from curve_gaussian_amd.ops.view_chunks import detected_lut


# ------------------------------------------------------------------------------------------------ brute force
def thin_brute(mask, max_iterations=0):
    """(uint8 [H,W] of 0 / 1, iterations): pixel by pixel in Python integers, from the definition.  The
    count includes the iteration that changed nothing."""
    state = [[1 if int(v) != 0 else 0 for v in row] for row in np.asarray(mask)]
    H, W = len(state), len(state[0])

    def at(s, y, x):
        return s[y][x] if 0 <= y < H and 0 <= x < W else 0

    done = 0
    while True:
        changed = False
        for sub in (0, 1):
            before = state
            state = [row[:] for row in before]
            for y in range(H):
                for x in range(W):
                    if not before[y][x]:
                        continue
                    P2, P3, P4, P5 = at(before, y - 1, x), at(before, y - 1, x + 1), at(before, y, x + 1), at(before, y + 1, x + 1)
                    P6, P7, P8, P9 = at(before, y + 1, x), at(before, y + 1, x - 1), at(before, y, x - 1), at(before, y - 1, x - 1)
                    C = (int(not P2 and (P3 or P4)) + int(not P4 and (P5 or P6)) + int(not P6 and (P7 or P8))
                         + int(not P8 and (P9 or P2)))
                    N1 = int(P9 or P2) + int(P3 or P4) + int(P5 or P6) + int(P7 or P8)
                    N2 = int(P2 or P3) + int(P4 or P5) + int(P6 or P7) + int(P8 or P9)
                    m = ((P6 or P7 or not P9) and P8) if sub == 0 else ((P2 or P3 or not P5) and P4)
                    if C == 1 and 2 <= min(N1, N2) <= 3 and not m:
                        state[y][x] = 0
                        changed = True
        done += 1
        if not changed or done == max_iterations:
            return np.array(state, np.uint8).reshape(H, W), done


# ------------------------------------------------------------------------------------------------ small masks
SMALL_SHAPES = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 3), (1, 5), (5, 1), (2, 3), (3, 17), (17, 5), (5, 5), (17, 17), (33, 2),
                (2, 33), (17, 33), (33, 17), (33, 33)]
DENSITIES = [0.3, 0.6, 0.9]


def random_mask(shape, density, seed=0):
    rng = np.random.default_rng(1000 * shape[0] + 10 * shape[1] + int(100 * density) + seed)
    return (rng.random(shape) < density).astype(np.uint8)


def draw_stroke(img, p0, p1, width):
    """Sets, in place, the pixels of a stroke from p0 = (y, x) to p1: a ``width`` x ``width`` square stamped at every
    half-pixel step (clipped to the image)."""
    H, W = img.shape
    (y0, x0), (y1, x1) = p0, p1
    n = 2 * int(max(abs(y1 - y0), abs(x1 - x0))) + 1
    lo = (width - 1) // 2
    for t in np.linspace(0.0, 1.0, n):
        y, x = int(round(y0 + t * (y1 - y0))) - lo, int(round(x0 + t * (x1 - x0))) - lo
        img[max(y, 0):max(y + width, 0), max(x, 0):max(x + width, 0)] = 1
    return img


def special_masks():
    """(name, uint8 [H,W]) of the hand cases: all ones, all zeros, one pixel, blocks, border lines and strokes 1 to 3 wide."""
    out = []
    for shape in [(1, 1), (2, 2), (3, 3), (5, 17), (17, 17), (33, 33)]:
        out.append((f"ones{shape}", np.ones(shape, np.uint8)))
        out.append((f"zeros{shape}", np.zeros(shape, np.uint8)))
    for shape, at in [((1, 1), (0, 0)), ((5, 5), (2, 2)), ((5, 5), (0, 0)), ((17, 33), (16, 32))]:
        m = np.zeros(shape, np.uint8)
        m[at] = 1
        out.append((f"pixel{shape}{at}", m))
    for b in (2, 3):
        for at in ((0, 0), (6, 7), (17 - b, 17 - b)):
            m = np.zeros((17, 17), np.uint8)
            m[at[0]:at[0] + b, at[1]:at[1] + b] = 1
            out.append((f"block{b}{at}", m))
    for side in ("top", "bottom", "left", "right"):
        m = np.zeros((17, 33), np.uint8)
        if side in ("top", "bottom"):
            m[0 if side == "top" else -1, :] = 1
        else:
            m[:, 0 if side == "left" else -1] = 1
        out.append((f"border_{side}", m))
    frame = np.zeros((17, 33), np.uint8)
    frame[0, :] = frame[-1, :] = frame[:, 0] = frame[:, -1] = 1
    out.append(("border_frame", frame))
    for width in (1, 2, 3):
        for name, p0, p1 in (("horizontal", (16, 3), (16, 29)), ("vertical", (3, 16), (29, 16)), ("diagonal", (4, 4), (28, 28)),
                             ("antidiagonal", (28, 4), (4, 28))):
            out.append((f"{name}{width}", draw_stroke(np.zeros((33, 33), np.uint8), p0, p1, width)))
    return out


def disc(shape, centre, radius):
    yy, xx = np.mgrid[:shape[0], :shape[1]]
    return ((yy - centre[0]) ** 2 + (xx - centre[1]) ** 2 <= radius * radius).astype(np.uint8)


def stroke_field(shape, n, seed=0, widths=(1, 9)):
    """uint8 [H,W]: n random strokes of the given widths (inclusive range)."""
    rng = np.random.default_rng(seed)
    img = np.zeros(shape, np.uint8)
    for _ in range(n):
        p0 = (int(rng.integers(shape[0])), int(rng.integers(shape[1])))
        length, angle = rng.uniform(5, 80), rng.uniform(0, 2 * np.pi)
        p1 = (p0[0] + length * np.sin(angle), p0[1] + length * np.cos(angle))
        draw_stroke(img, p0, p1, int(rng.integers(widths[0], widths[1] + 1)))
    return img


# ------------------------------------------------------------------------------------------------ the drawn scan, dilated
def dilate(masks, r):
    """The masks ([..., H, W], 0 / 1) dilated by a (2r+1) x (2r+1) square: the width of a detector's response."""
    m = np.asarray(masks) != 0
    out = m.copy()
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            src = m[..., max(-dy, 0):m.shape[-2] - max(dy, 0), max(-dx, 0):m.shape[-1] - max(dx, 0)]
            out[..., max(dy, 0):m.shape[-2] - max(-dy, 0), max(dx, 0):m.shape[-1] - max(-dx, 0)] |= src
    return out.astype(np.uint8)


@functools.lru_cache(maxsize=None)
def scan_masks(r=0):
    """uint8 [12,96,128]: the detected masks of the drawn scan (edge_dir_cases.dir_novel_cameras), dilated by r.  Shared: callers leave it
    unchanged."""
    maps = np.stack(DC.dir_novel_cameras()[1])
    return dilate(detected_lut("PidiNet", 0.5)[maps].astype(np.uint8), r)


@functools.lru_cache(maxsize=None)
def thick_scan(r):
    """(cameras, maps): the drawn scan with masks dilated by r, stored as PidiNet bytes (255 = detected)."""
    return DC.dir_novel_cameras()[0], [np.ascontiguousarray(m * np.uint8(255)) for m in scan_masks(r)]

