"""Vectorised numpy restatement of the boundary metric's rules (include/dp_mi355x.h, "Scale-invariant boundary metric").

Everything the device computes, on the host: inverse depth, the four ratio maps, plain / thinned / mask edges, the
per-threshold counts and the scores made from them.  `width` says how a ratio meets a threshold: "f64" is
(double)ratio > t (the reference's boundary_f1, and what the kernels do), "f32" is ratio > float32(t) (the reference's
edge_recall_matting).  tests/golden/golden_boundary.npz pins all of it to the reference's own functions.
`scene` is the synthetic test picture, also used by tools/boundary_bench.py at full size.
"""

import numpy as np

DIRS = ("left", "top", "right", "bottom")
EPS = np.float32(1e-6)


def invert_depth(depth):
    d = np.asarray(depth)
    assert d.dtype == np.float32
    with np.errstate(all="ignore"):
        return np.float32(1.0) / np.where(d < EPS, EPS, d)                 # a NaN stays (numpy's clip)


def ratios(inv):
    """(left, top, right, bottom) float32 ratio maps of a float32 inverse depth."""
    with np.errstate(all="ignore"):
        return (inv[:, :-1] / inv[:, 1:], inv[:-1, :] / inv[1:, :], inv[:, 1:] / inv[:, :-1], inv[1:, :] / inv[:-1, :])


def above(ratio, t, width="f64"):
    with np.errstate(invalid="ignore"):
        return ratio.astype(np.float64) > float(t) if width == "f64" else ratio > np.float32(t)


def thin_rows(ratio, edge):
    """Of every maximal run of edge cells in a row, the first of the largest ratios."""
    out = np.zeros(edge.shape, bool)
    if not edge.any():
        return out
    prev = np.zeros_like(edge)
    prev[:, 1:] = edge[:, :-1]
    run = np.cumsum((edge & ~prev).ravel()) - 1                             # the run a cell belongs to, where it is an edge
    at = np.flatnonzero(edge.ravel())
    rid, val = run[at], ratio.ravel()[at]
    top = np.full(rid.max() + 1, -np.inf, np.float32)
    np.maximum.at(top, rid, val)
    best = val == top[rid]
    first = np.full(len(top), ratio.size, np.int64)
    np.minimum.at(first, rid[best], at[best])
    out.ravel()[first] = True
    return out


def plain_edges(inv, t, width="f64"):
    return tuple(above(r, t, width) for r in ratios(inv))


def thinned_edges(inv, t, width="f64"):
    l, tp, r, b = ratios(inv)
    return (thin_rows(l, above(l, t, width)), thin_rows(tp.T, above(tp.T, t, width)).T,
            thin_rows(r, above(r, t, width)), thin_rows(b.T, above(b.T, t, width)).T)


def mask_edges(m):
    m = np.asarray(m, bool)
    return (m[:, :-1] & ~m[:, 1:], m[:-1, :] & ~m[1:, :], m[:, 1:] & ~m[:, :-1], m[1:, :] & ~m[:-1, :])


def counts(pred_inv, target, thresholds, kind, width="f64"):
    """uint64 [n, 4, 3] of (both, target, predicted).  kind "depth": target is an inverse depth, plain edges on both
    sides; kind "mask": target is a bool mask, the prediction is thinned."""
    out = np.zeros((len(thresholds), 4, 3), np.uint64)
    for k, t in enumerate(thresholds):
        if kind == "depth":
            p, g = plain_edges(pred_inv, t, width), plain_edges(target, t, width)
        else:
            p, g = thinned_edges(pred_inv, t, width), mask_edges(target)
        for d in range(4):
            out[k, d] = (np.count_nonzero(p[d] & g[d]), np.count_nonzero(g[d]), np.count_nonzero(p[d]))
    return out


def padded(maps, shape):
    """Four edge maps as one uint8 [4, H, W], 0 outside each map's extent."""
    out = np.zeros((4,) + tuple(shape), np.uint8)
    for d, m in enumerate(maps):
        out[d, :m.shape[0], :m.shape[1]] = m
    return out


def recall_of(c):
    c = [[int(v) for v in row] for row in c]
    return 0.25 * (c[0][0] / max(c[0][1], 1) + c[1][0] / max(c[1][1], 1) + c[2][0] / max(c[2][1], 1) + c[3][0] / max(c[3][1], 1))


def precision_of(c):
    c = [[int(v) for v in row] for row in c]
    return 0.25 * (c[0][0] / max(c[0][2], 1) + c[1][0] / max(c[1][2], 1) + c[2][0] / max(c[2][2], 1) + c[3][0] / max(c[3][2], 1))


def f1_of(c):
    r, p = recall_of(c), precision_of(c)
    if r + p == 0:
        return 0.0
    return 2 * (r * p) / (r + p)


def thresholds_and_weights(t_min=1.05, t_max=1.25, n=10):
    th = np.linspace(t_min, t_max, n)
    return th, th / th.sum()


def si_boundary_f1(pred, target, t_min=1.05, t_max=1.25, n=10):
    th, w = thresholds_and_weights(t_min, t_max, n)
    c = counts(invert_depth(pred), invert_depth(target), th, "depth", "f64")
    return np.sum(np.array([f1_of(c[k]) for k in range(n)]) * w)


def si_boundary_recall(pred, alpha, t_min=1.05, t_max=1.25, n=10, alpha_threshold=0.1):
    th, w = thresholds_and_weights(t_min, t_max, n)
    c = counts(invert_depth(pred), np.asarray(alpha) > alpha_threshold, th, "mask", "f32")
    return np.sum(np.array([recall_of(c[k]) for k in range(n)]) * w)


def scene(h, w, seed=0):
    """Boxes at several depths over a sloped floor with multiplicative noise.  Returns (pred, target, alpha): the
    target depth, the prediction (the target with every third row shifted by one pixel, re-noised) and a boxes mask whose borders
    carry the alphas 0.05, float32(0.1), 0.15 and 1 -- all float32."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    clean = 2.0 + 6.0 * (1.0 - y / h) + 0.5 * x / w
    alpha = np.zeros((h, w), np.float32)
    levels = (np.float32(0.05), np.float32(0.1), np.float32(0.15), np.float32(1.0))
    n_box = max(6, (h * w) // 2000)
    for i in range(n_box):
        bh, bw = int(rng.integers(max(3, h // 12), max(5, h // 3))), int(rng.integers(max(3, w // 12), max(5, w // 3)))
        y0, x0 = int(rng.integers(0, max(1, h - bh))), int(rng.integers(0, max(1, w - bw)))
        clean[y0:y0 + bh, x0:x0 + bw] = clean[y0:y0 + bh, x0:x0 + bw].min() / float(rng.uniform(1.1, 1.8))
        if i % 2 == 0:
            a = alpha[y0:y0 + bh, x0:x0 + bw]
            a[:] = 1.0
            a[0, :], a[-1, :], a[:, 0], a[:, -1] = levels[i % 4], levels[(i + 1) % 4], levels[(i + 2) % 4], levels[(i + 3) % 4]
    target = (clean * rng.uniform(0.985, 1.015, (h, w))).astype(np.float32)
    moved = np.where((np.arange(h) % 3 == 0)[:, None], np.roll(clean, 1, axis=1), clean)
    pred = (moved * rng.uniform(0.97, 1.03, (h, w))).astype(np.float32)
    return pred, target, alpha
