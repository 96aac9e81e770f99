"""float64 numpy restatement of the three curve-fit kernels' definitions (include/curvegs.h: cgs_curve_straightness,
cgs_segment_merge_labels, cgs_pair_consensus_fit), written from the host code they stand in for (scene/topology.py:
is_curve_straight, _pairwise_segment_distances / _pairwise_cosine_similarity / connected_components, the per-pair block of
merge_curves), not from the kernels.  Inputs are the float32 arrays the kernels read; everything after the conversion is
float64.  Also the margins of an input: how far each thresholded quantity is from its threshold."""
import numpy as np


def bernstein(t):
    t = np.asarray(t, np.float64)
    s = 1.0 - t
    return np.stack([s ** 3, 3 * s ** 2 * t, 3 * s * t ** 2, t ** 3], axis=-1)       # [n,4]


def sample_curves(cp, sample_num):
    """cp [B,4,3] float32 -> [B,sample_num,3] float64 at t = i / (sample_num - 1)."""
    A = bernstein(np.arange(sample_num, dtype=np.float64) / (sample_num - 1))
    return np.einsum("nk,bkc->bnc", A, np.asarray(cp, np.float32).astype(np.float64))


def principal_direction(centered):
    """Unit eigenvector of the largest eigenvalue of centered^T centered, and the relative gap to the next eigenvalue."""
    w, v = np.linalg.eigh(centered.T @ centered)
    d = v[:, 2]
    n = np.linalg.norm(d)
    d = d / n if n > 0 else np.array([1.0, 0.0, 0.0])
    gap = (w[2] - w[1]) / w[2] if w[2] > 0 else 0.0
    return d, gap


# ------------------------------------------------------------------------------------------------ straightness
def curve_straightness(cp, is_bezier, threshold, threshold_max, sample_num=100):
    """-> mean_dist [B], max_dist [B], straight [B] bool, eigengap [B] (relative; 0 for coincident samples)."""
    pts = sample_curves(cp, sample_num)
    B = pts.shape[0]
    mean_d, max_d, gap = np.zeros(B), np.zeros(B), np.zeros(B)
    for b in range(B):
        p = pts[b]
        m = p.mean(axis=0)
        if np.all(p == p[0]):
            continue                                     # every distance is 0
        d, gap[b] = principal_direction(p - m)
        t = (p - m) @ d
        foot = m + np.clip(t, t.min(), t.max())[:, None] * d
        dist = np.linalg.norm(p - foot, axis=1)
        mean_d[b], max_d[b] = dist.mean(), dist.max()
    straight = np.asarray(is_bezier).astype(bool) & (mean_d < threshold) & (max_d < threshold_max)
    return mean_d, max_d, straight, gap


# ------------------------------------------------------------------------------------------------ segment labels
def segment_pair_quantities(seg):
    """seg [n,6] float32 -> (dist [n,n], cos [n,n], valid [n,n]) in float64, symmetric: for a < b the smaller distance of b's
    end points to segment a (foot clipped) and |cos| of the directions; pairs with a zero-length segment are not valid."""
    s = np.asarray(seg, np.float32).astype(np.float64)
    n = len(s)
    p, q = s[:, :3], s[:, 3:]
    d = q - p
    dd = np.einsum("ij,ij->i", d, d)
    nz = dd > 0
    dn = np.where(nz[:, None], d / np.sqrt(np.where(nz, dd, 1.0))[:, None], 0.0)
    cos = np.abs(dn @ dn.T)
    safe = np.where(nz, dd, 1.0)

    def to_seg(pts):                                     # [a, b]: distance of pts[b] to segment a
        r = pts[None, :, :] - p[:, None, :]
        u = np.clip(np.einsum("abc,ac->ab", r, d) / safe[:, None], 0.0, 1.0)
        return np.linalg.norm(p[:, None, :] + u[:, :, None] * d[:, None, :] - pts[None, :, :], axis=2)
    upper = np.triu(np.minimum(to_seg(p), to_seg(q)), 1)
    dist = upper + upper.T
    valid = nz[:, None] & nz[None, :] & ~np.eye(n, dtype=bool)
    return dist, cos, valid


def segment_merge_labels(seg, distance_threshold, similarity_threshold):
    """-> labels [n] (smallest index of the component), n_components."""
    n = len(seg)
    if n == 0:
        return np.zeros(0, np.int64), 0
    dist, cos, valid = segment_pair_quantities(seg)
    adj = valid & (cos >= similarity_threshold) & (dist <= distance_threshold)
    labels = np.full(n, -1, np.int64)
    for i in range(n):                                   # flood fill from the smallest unlabelled index
        if labels[i] >= 0:
            continue
        labels[i] = i
        stack = [i]
        while stack:
            a = stack.pop()
            for b in np.nonzero(adj[a] & (labels < 0))[0]:
                labels[b] = i
                stack.append(int(b))
    return labels, int((labels == np.arange(n)).sum())


def segment_margins(seg, distance_threshold, similarity_threshold):
    """Smallest |dist - distance_threshold| and |cos - similarity_threshold| over the valid pairs (inf without one)."""
    dist, cos, valid = segment_pair_quantities(seg)
    if not valid.any():
        return np.inf, np.inf
    return float(np.abs(dist[valid] - distance_threshold).min()), float(np.abs(cos[valid] - similarity_threshold).min())


# ------------------------------------------------------------------------------------------------ pair consensus fit
def line_residuals(pts, i, j):
    d = pts[j] - pts[i]
    nd = np.linalg.norm(d)
    if not nd > 0:
        return None
    d = d / nd
    r = pts - pts[i]
    return np.linalg.norm(r - np.outer(r @ d, d), axis=1)


def consensus(pts, ransac_thresh):
    """All two-point lines (i < j, non-zero distance): -> (counts [M], residual sums [M], (i, j) [M,2]), row-major order."""
    n = len(pts)
    iu, ju = np.triu_indices(n, 1)
    counts = np.zeros(len(iu), np.int64)
    sums = np.full(len(iu), np.inf)
    for i in range(n - 1):
        sel = slice(i * (2 * n - i - 1) // 2, (i + 1) * (2 * n - i - 2) // 2)
        d = pts[i + 1:] - pts[i]
        nd = np.linalg.norm(d, axis=1)
        okd = nd > 0
        d = d / np.where(okd, nd, 1.0)[:, None]
        r = pts - pts[i]                                               # [n,3]
        t = d @ r.T                                                    # [m,n]
        e = r[None, :, :] - t[:, :, None] * d[:, None, :]
        res = np.linalg.norm(e, axis=2)
        c = (res < ransac_thresh).sum(axis=1)
        s = (res ** 2).sum(axis=1)
        counts[sel] = np.where(okd, c, 0)
        sums[sel] = np.where(okd, s, np.inf)
    return counts, sums, np.stack([iu, ju], axis=1)


def best_candidate(counts, sums):
    """Index of the winner: largest count, then smallest residual sum, then first."""
    order = np.lexsort((np.arange(len(counts)), sums, -counts))
    return int(order[0]), order


def pair_consensus_fit_one(pts, ransac_thresh, error_threshold):
    """pts [N,3] float64 -> dict(ctrl [4,3] float64, rmse, inliers, ok, winner (i, j), runner_up gap info)."""
    n = len(pts)
    counts, sums, ij = consensus(pts, ransac_thresh)
    fail = dict(ctrl=np.zeros((4, 3)), rmse=0.0, inliers=0, ok=False, winner=None, count_gap=None, sum_gap=None, eigengap=None)
    if len(counts) == 0 or counts.max() < 2:
        fail["inliers"] = int(counts.max()) if len(counts) else 0
        return fail
    w, order = best_candidate(counts, sums)
    second = int(order[1]) if len(order) > 1 else None
    i, j = ij[w]
    inl = line_residuals(pts, i, j) < ransac_thresh
    center = pts[inl].mean(axis=0)
    c = pts[inl] - center
    main, gap = principal_direction(c)
    proj = c @ main
    start, end = center + main * proj.min(), center + main * proj.max()
    main = end - start
    main = main / np.linalg.norm(main)
    mid = (end + start) / 2
    ordered = pts[np.argsort((pts - mid) @ main, kind="stable")]
    A = bernstein(np.linspace(0, 1, n))
    P = np.linalg.solve(A.T @ A, A.T @ ordered)
    rmse = float(np.sqrt(np.mean(np.sum((ordered - A @ P) ** 2, axis=1))))
    return dict(ctrl=P, rmse=rmse, inliers=int(counts[w]), ok=bool(rmse <= error_threshold), winner=(int(i), int(j)),
                count_gap=None if second is None else int(counts[w] - counts[second]),
                sum_gap=None if second is None else float((sums[second] - sums[w]) / max(sums[second], 1e-300)),
                eigengap=float(gap), residual_margin=float(np.abs(line_residuals(pts, i, j) - ransac_thresh).min()))


def pair_consensus_fit(cp, pairs, sample_num=100, ransac_thresh=0.005, error_threshold=0.02):
    """-> list of pair_consensus_fit_one results, one per row of pairs."""
    pts = sample_curves(cp, sample_num)
    return [pair_consensus_fit_one(np.concatenate([pts[i], pts[j]]), ransac_thresh, error_threshold) for i, j in np.asarray(pairs)]


def winner_is_unique(r, rel=1e-9):
    """The margin condition on a consensus result: the winner leads by count, or by a relative residual-sum gap."""
    return r["winner"] is None or r["count_gap"] is None or r["count_gap"] >= 1 or r["sum_gap"] >= rel


# ------------------------------------------------------------------------------------------------ seeded test inputs
def chain_segments(seed, n_lines=40, pieces=5, noise=0.003):
    """n_lines random lines in the unit cube, each cut into `pieces` collinear pieces with small gaps, end points jittered,
    randomly oriented and shuffled -> float32 [n_lines * pieces, 6]."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_lines):
        a = rng.uniform(0.1, 0.9, 3)
        d = rng.normal(size=3)
        d = d / np.linalg.norm(d) * rng.uniform(0.3, 0.6)
        cuts = np.linspace(0, 1, pieces + 1)
        for k in range(pieces):
            p = a + d * (cuts[k] + 0.01) + rng.normal(size=3) * noise
            q = a + d * (cuts[k + 1] - 0.01) + rng.normal(size=3) * noise
            out.append(np.concatenate([q, p] if rng.random() < 0.5 else [p, q]))
    out = np.asarray(out)
    return out[rng.permutation(len(out))].astype(np.float32)


def bent_curve(p0, p3, bend):
    """A cubic from p0 to p3 whose inner control points leave the chord by the vector `bend`."""
    p0, p3, bend = (np.asarray(v, np.float64) for v in (p0, p3, bend))
    return np.stack([p0, p0 + (p3 - p0) / 3 + bend, p0 + (p3 - p0) * 2 / 3 + bend, p3])


def straightness_curves(seed=0):
    """float32 [B,4,3]: random bent and nearly straight curves, an exactly straight one, coincident control points, and four
    arcs around the thresholds of fit_curve_to_line.  The samples of an arc bent by b leave the fitted segment by 0.495 b at
    most and 0.196 b on average, so the maximum (0.004) binds first: bends 0.00806 / 0.00811 sit on either side of it, and
    bends 0.0101 / 0.0103 on either side of the mean threshold 0.002 (to be tested with a maximum threshold out of the way)."""
    rng = np.random.default_rng(seed)
    rows = []
    for k in range(24):
        a = rng.uniform(0.1, 0.9, 3)
        d = rng.normal(size=3)
        d = d / np.linalg.norm(d) * rng.uniform(0.1, 0.3)
        b = np.cross(d, rng.normal(size=3))
        b = b / np.linalg.norm(b) * (rng.uniform(0.02, 0.05) if k % 2 else rng.uniform(0.0, 0.002))
        rows.append(bent_curve(a, a + d, b))
    rows.append(bent_curve([0.2, 0.2, 0.2], [0.5, 0.6, 0.7], [0, 0, 0]))                 # exactly straight
    rows.append(np.tile(np.array([0.3, 0.4, 0.5]), (4, 1)))                              # coincident control points
    for bend in (0.00806, 0.00811, 0.0101, 0.0103):
        rows.append(bent_curve([0.1, 0.1, 0.1], [0.4, 0.1, 0.1], [0, bend, 0]))
    return np.asarray(rows).astype(np.float32)


def noisy_bent_pair():
    """float32 [2,4,3]: two end-to-end curves, gently bent and wobbling, whose 200 samples are NOT all within 0.005 of one line."""
    a = bent_curve([0.20, 0.30, 0.50], [0.45, 0.31, 0.50], [0.0, 0.013, 0.004])
    b = bent_curve([0.45, 0.31, 0.50], [0.70, 0.30, 0.51], [0.0, -0.009, 0.011])
    a[1] += [0.0, 0.004, -0.003]
    b[2] += [0.0, 0.006, 0.002]
    return np.stack([a, b]).astype(np.float32)


def cut_cubic(whole=((0.2, 0.2, 0.5), (0.3, 0.32, 0.5), (0.45, 0.36, 0.5), (0.6, 0.3, 0.5))):
    """One cubic and its two de Casteljau halves at 0.5 (exact in float32 for these halvings up to rounding) ->
    (whole [4,3] float64, halves float32 [2,4,3])."""
    p0, p1, p2, p3 = (np.asarray(v, np.float32) for v in whole)
    half = lambda p, q: np.float32(0.5) * (p + q)
    a0, a1, a2 = half(p0, p1), half(p1, p2), half(p2, p3)
    b0, b1 = half(a0, a1), half(a1, a2)
    mid = half(b0, b1)
    return np.asarray(whole, np.float64), np.stack([np.stack([p0, a0, b0, mid]), np.stack([mid, b1, a2, p3])])


def large_model(seed=0, n_lines=200, pieces=5, n_cubics=100):
    """float32 [B,4,3] and is_bezier [B]: n_lines * pieces straight segments (chains of collinear pieces whose directions stay
    within ~3 degrees of a coordinate axis, so that no pair of directions comes near a similarity threshold of 0.97) followed
    by n_cubics bent cubics, each cut in two at 0.5 (rows 2k, 2k + 1), on a grid of pitch 0.4 that keeps different cubics' ends apart (the model spans [0, 2], not the unit cube)."""
    rng = np.random.default_rng(seed)
    segs = []
    for k in range(n_lines):
        axis = np.zeros(3)
        axis[k % 3] = 1.0
        d = axis + rng.normal(size=3) * 0.02
        d = d / np.linalg.norm(d) * rng.uniform(0.3, 0.5)
        a = rng.uniform(0.05, 0.5, 3)
        cuts = np.linspace(0, 1, pieces + 1)
        for j in range(pieces):
            p = a + d * (cuts[j] + 0.01) + rng.normal(size=3) * 0.002
            q = a + d * (cuts[j + 1] - 0.01) + rng.normal(size=3) * 0.002
            p, q = (q, p) if rng.random() < 0.5 else (p, q)
            segs.append(np.stack([p, p + (q - p) / 3, p + (q - p) * 2 / 3, q]))
    segs = np.asarray(segs)[rng.permutation(n_lines * pieces)]
    halves = []
    for k in range(n_cubics):
        o = np.array([0.3 + 0.4 * (k % 5), 0.3 + 0.4 * ((k // 5) % 5), 0.1 + 0.4 * (k // 25)])
        ang = rng.uniform(0, 2 * np.pi)
        u, v = np.array([np.cos(ang), np.sin(ang), 0.0]), np.array([-np.sin(ang), np.cos(ang), 0.0])
        whole = [o, o + 0.055 * u + rng.uniform(0.06, 0.08) * v, o + 0.115 * u + rng.uniform(0.06, 0.08) * v, o + 0.17 * u]
        halves.append(cut_cubic(whole)[1])
    cp = np.concatenate([segs, np.concatenate(halves)]).astype(np.float32)
    isb = np.concatenate([np.zeros(len(segs), bool), np.ones(2 * n_cubics, bool)])
    return cp, isb
