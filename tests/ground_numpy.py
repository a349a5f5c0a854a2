"""Vectorised numpy restatement of the ground stages (fit trace, normalise, grid adjustment).

Ours, written from the reference's rules (img_to_normalized_pointcloud.py:601-816, :880-981,
:983-1118) with sort-and-group instead of one full-length mask per cell, so it runs at 1080p in
well under a second.  tests/test_ground.py pins it to the reference's own functions through
tests/golden/golden_ground.npz, then uses it as the expected value at sizes the fixture lacks.

Each stage also returns `margin`: the smallest distance of any point from a *discontinuous*
decision (|dist| = 0.05 / 0.1, y = 0.2, percentile = 0.01, an interior bin edge); the fit reports
`pushdown_safe` for its count-based decision.  The clamps at
0 / -0.1 and the 0.1 / 1.5 grading knees are continuous and need none.  A test that compares with
a tolerance asserts margin > 1e-6 first, so a flipped classification cannot hide in it.

Points with a non-finite coordinate take no part and pass through unchanged (the project's rule).
"""

import numpy as np

from depth_pro.pointcloud import fit_trace_plane, ground_rotation


def _finite(points):
    return np.isfinite(points).all(axis=1)


def _edge_margin(v, edges):
    """min |v - interior edge| (the outer edges are the min / max themselves: exact on both sides)."""
    inner = edges[1:-1]
    if len(inner) == 0 or len(v) == 0:
        return np.inf
    i = np.searchsorted(inner, v)
    lo, hi = inner[np.clip(i - 1, 0, len(inner) - 1)], inner[np.clip(i, 0, len(inner) - 1)]
    return float(np.minimum(np.abs(v - lo), np.abs(v - hi)).min())


def plane_dist(points, normal, d):
    return ((points[:, 0] * normal[0] + points[:, 1] * normal[1]) + points[:, 2] * normal[2]) + d


def ground_trace(points, grid_size=20):
    """(trace points (k, 3) in bin order, dict(margin, tie_free, counts, valid))."""
    p = points[_finite(points)]
    z, y = p[:, 2], p[:, 1]
    edges = np.linspace(z.min(), z.max(), grid_size + 1)
    bins = np.digitize(z, edges) - 1
    order = np.lexsort((np.arange(len(p)), y, bins))        # by bin, then y, ties in index order
    sb = bins[order]
    starts = np.searchsorted(sb, np.arange(grid_size))
    ends = np.searchsorted(sb, np.arange(grid_size), side="right")
    trace, valid, tie_free = [], [], True
    for s, e in zip(starts, ends):
        c = e - s
        valid.append(c > 10)
        if c > 10:
            k = max(1, int(0.05 * c))
            sel = order[s:s + k]
            trace.append(p[np.sort(sel)].mean(axis=0))
            if k < c and y[order[s + k]] == y[order[s + k - 1]]:
                tie_free = False
    info = dict(margin=_edge_margin(z, edges), tie_free=tie_free, counts=ends - starts, valid=np.array(valid))
    return np.array(trace).reshape(-1, 3), info


def fit(points, grid_size=20):
    """The deterministic fit: (model dict, info)."""
    p = points[_finite(points)]
    trace, info = ground_trace(points, grid_size)
    info["fallback"] = len(trace) < 10
    if len(trace) < 10:
        k = max(10, int(0.05 * len(p)))
        order = np.lexsort((np.arange(len(p)), p[:, 1]))
        if k < len(p) and p[order[k], 1] == p[order[k - 1], 1]:
            info["tie_free"] = False
        trace = p[np.sort(order[:k])]
    normal, d = fit_trace_plane(trace)
    if normal[1] < 0:
        normal, d = -normal, -d
    dist = plane_dist(p, normal, d)
    below = int((dist < 0).sum())
    # the push-down decision is a count against 0.001 n: safe if more points would have to change
    # sides than lie within 1e-6 of the plane
    unsure = int((np.abs(dist) < 1e-6).sum())
    info["pushdown_safe"] = abs(below - 0.001 * len(p)) > unsure and (below > unsure or below + unsure == 0)
    if below > 0 and below > 0.001 * len(p):
        d -= np.percentile(dist, 0.1) + 0.05
    model = {"normal": normal, "d": float(d), "origin": np.array([0.0, -d / normal[1] if normal[1] != 0 else 0.0, 0.0])}
    return model, info


def normalize(points, model):
    """(levelled points, stats (8,) in depth_pro.pointcloud.NORMALIZE_STATS order, margin)."""
    out = np.array(points, dtype=np.float64, copy=True)
    fin = _finite(points)
    p = points[fin]
    m = ground_rotation(model)
    unit, d, R, const, rotate = m[:3], m[3], m[4:13].reshape(3, 3), m[13], m[14]
    dist = plane_dist(p, unit, d)
    q = p.copy()
    if rotate:
        q = np.stack([(R[r, 0] * p[:, 0] + R[r, 1] * p[:, 1]) + R[r, 2] * p[:, 2] for r in range(3)], axis=1)
        q[:, 1] = q[:, 1] - const
    near = np.abs(dist) < 0.1
    level, taken = 0.0, near.sum() > 10
    if taken:
        level = np.percentile(q[near, 1], 2)
        q[:, 1] -= level
    ground = np.abs(dist) < 0.05
    zero = (q[:, 1] < 0) & ground
    q[zero, 1] = 0.0
    lim = (q[:, 1] < -0.1) & ~ground
    q[lim, 1] = -0.1
    out[fin] = q
    stats = np.array([fin.sum(), (~fin).sum(), near.sum(), level, float(taken), ground.sum(), zero.sum(), lim.sum()],
                     dtype=np.float64)
    ad = np.abs(dist)
    margin = float(min(np.abs(ad - 0.05).min(), np.abs(ad - 0.1).min())) if len(p) else np.inf
    return out, stats, margin


def adjust(points, grid_size=20, percentile=5):
    """(adjusted points, stats (8,) in depth_pro.pointcloud.ADJUST_STATS order, margin)."""
    out = np.array(points, dtype=np.float64, copy=True)
    fin = _finite(points)
    p = points[fin]
    if len(p) == 0:
        return out, np.array([0, (~fin).sum(), 0, 0, 0, 0, 0, 0], dtype=np.float64), np.inf
    x, y, z = p[:, 0], p[:, 1].copy(), p[:, 2]
    g = grid_size
    xe, ze = np.linspace(x.min(), x.max(), g + 1), np.linspace(z.min(), z.max(), g + 1)
    cell = np.clip(np.digitize(x, xe) - 1, 0, g - 1) * g + np.clip(np.digitize(z, ze) - 1, 0, g - 1)
    n_all = np.bincount(cell, minlength=g * g)
    low = y < 0.2
    n_low = np.bincount(cell[low], minlength=g * g)
    order = np.lexsort((y[low], cell[low]))
    ys, cs = y[low][order], cell[low][order]
    starts = np.searchsorted(cs, np.arange(g * g))
    pct = np.full(g * g, np.nan)
    for c in np.flatnonzero(n_low):
        pct[c] = np.percentile(ys[starts[c]:starts[c] + n_low[c]], percentile)
    ok = (n_all >= 10) & (n_low >= 5) & (pct > 0.01)
    pp = np.where(ok, pct, 0.0)[cell]
    adj = np.zeros(len(p))
    near = y < 0.1
    adj[near] = pp[near]
    mid = (y >= 0.1) & (y < 1.5)
    adj[mid] = pp[mid] * (1.0 - (y[mid] - 0.1) / 1.4)
    ynew = y - adj
    inok = ok[cell]
    ynew[inok & (ynew < 0)] = 0.0
    p2 = p.copy()
    p2[:, 1] = np.where(inok, ynew, y)
    out[fin] = p2
    stats = np.array([fin.sum(), (~fin).sum(), (n_all > 0).sum(), (n_all >= 10).sum(), ok.sum(), (adj > 0).sum(), 0, 0],
                     dtype=np.float64)
    cand = (n_all >= 10) & (n_low >= 5)
    margin = min(_edge_margin(x, xe), _edge_margin(z, ze), float(np.abs(y - 0.2).min()),
                 float(np.abs(pct[cand] - 0.01).min()) if cand.any() else np.inf)
    return out, stats, margin


def terrain(h, w, seed):
    """Random rolling terrain seen from 1.6 m, a far wall, fp32 depth with a few invalid pixels."""
    g = np.random.default_rng(seed)
    f = 0.9 * w
    v, u = np.indices((h, w)).astype(np.float64)
    ry = -(v - h / 2) / f
    bumps = sum(a * np.sin(u / w * fr + ph) * np.cos(v / h * fr * 0.7 + ph)
                for a, fr, ph in zip((0.05, 0.03, 0.02), (9.0, 23.0, 51.0), g.random(3) * 6))
    t = np.radians(5.0)
    nr = np.cos(t) * ry + np.sin(t)
    z = np.where(nr < -1e-3, -(1.6 + bumps) / np.minimum(nr, -1e-3), np.inf)
    depth = np.minimum(z, 30.0) * (1 + 1e-3 * g.standard_normal((h, w)))
    depth = depth.astype(np.float32)
    depth[g.random((h, w)) < 0.002] = np.nan
    depth[g.random((h, w)) < 0.002] = 0.0
    return depth, float(np.float32(f))
