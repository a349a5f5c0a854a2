"""numpy / scipy restatement of the cleaning stage (include/dp_mi355x.h, "Cleaned point clouds"), in the
role tests/ground_numpy.py has for the ground stages: the GPU tests compare with it exactly, and
tests/golden/make_golden_clean.py checks it against the reference's own functions.

Stray points: scipy's cKDTree only proposes candidates (a slightly larger radius); the formula of the
header, (dx*dx + dy*dy) + dz*dz < radius*radius in fp64, decides.  Shadows: numpy's own arange,
digitize and median on a stable (column, y, index) order.
"""

import numpy as np


def _finite(points):
    return np.isfinite(points).all(axis=1)


def neighbour_counts(points, radius):
    """Number of finite points (itself included) within the strict radius of every finite point;
    0 for the non-finite ones."""
    from scipy.spatial import cKDTree

    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    fin = _finite(points)
    P = points[fin]
    counts = np.zeros(len(points), dtype=np.int64)
    if len(P) == 0:
        return counts
    r2 = radius * radius
    cand = cKDTree(P).query_ball_point(P, radius * (1 + 1e-9) + 1e-300)
    c = np.empty(len(P), dtype=np.int64)
    for j, idx in enumerate(cand):
        d = P[idx] - P[j]
        c[j] = int((((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) < r2).sum())
    counts[fin] = c
    return counts


def stray_mask(points, nb_points=20, radius=0.1):
    """(keep (n,) bool, stats (8,)): dp_clean_stray without its overflow flag (tests stay below it)."""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    fin = _finite(points)
    keep = neighbour_counts(points, radius) >= nb_points
    keep &= fin
    stats = np.array([fin.sum(), (~fin).sum(), keep.sum(), len(points) - keep.sum(), 0, 0, 0, 0], dtype=np.float64)
    return keep, stats


def shadow_cell_size(P):
    """The reference's cell size from the finite points P (0.05 for an empty cloud)."""
    if len(P) == 0:
        return 0.05
    x_min, x_max = np.min(P[:, 0]), np.max(P[:, 0])
    z_min, z_max = np.min(P[:, 2]), np.max(P[:, 2])
    with np.errstate(all="ignore"):
        density = np.float64(len(P)) / ((x_max - x_min) * (z_max - z_min))
        v = 1.0 / np.sqrt(density / 10)
    return max(0.05, v)


def shadow_mask(points, shadow_height_threshold=0.1, max_shadow_angle=75, min_points_per_column=3):
    """(keep (n,) bool, stats (8,), info): dp_clean_shadows.  info["columns"] lists, per tested column,
    (member indices in order, angles, median); info["heights"] every occupied column's y range."""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n = len(points)
    fin = _finite(points)
    keep = np.ones(n, dtype=bool)
    P, where = points[fin], np.flatnonzero(fin)
    cell = float(shadow_cell_size(P))
    stats = np.array([fin.sum(), (~fin).sum(), 0, 0, 0, 0, cell, 0], dtype=np.float64)
    info = {"cell": cell, "columns": [], "heights": np.zeros(0), "counts": np.zeros(0, dtype=np.int64)}
    if len(P) == 0:
        return keep, stats, info
    x_min, x_max = np.min(P[:, 0]), np.max(P[:, 0])
    z_min, z_max = np.min(P[:, 2]), np.max(P[:, 2])
    with np.errstate(all="ignore"):
        lx = np.ceil(((x_max + cell) - x_min) / cell)
        lz = np.ceil(((z_max + cell) - z_min) / cell)
    if not (lx >= 1 and lz >= 1 and lx * lz < 2.0 ** 31) or not (x_min + cell) - x_min > 0 \
            or not (z_min + cell) - z_min > 0:
        stats[7] = 1
        return keep, stats, info
    x_bins = np.arange(x_min, x_max + cell, cell)
    z_bins = np.arange(z_min, z_max + cell, cell)
    assert len(x_bins) == lx and len(z_bins) == lz
    col = (np.digitize(P[:, 0], x_bins) - 1).astype(np.int64) * len(z_bins) + (np.digitize(P[:, 2], z_bins) - 1)
    info["column_of"] = np.full(n, -1, dtype=np.int64)               # column id per input row (-1: non-finite)
    info["column_of"][where] = col
    order = np.lexsort((np.arange(len(P)), P[:, 1], col))          # by column, then y, ties in index order
    cs, S = col[order], P[order]
    heads = np.flatnonzero(np.r_[True, cs[1:] != cs[:-1]])
    ends = np.r_[heads[1:], len(cs)]
    counts = ends - heads
    heights = S[ends - 1, 1] - S[heads, 1]
    tested = (counts >= min_points_per_column) & (counts >= 3) & (heights > shadow_height_threshold)
    info["heights"], info["counts"] = heights, counts
    info["x_bins"], info["z_bins"] = x_bins, z_bins
    info["runs"] = (heads, ends, S[:, 1])
    removed_cols = removed_pts = 0
    for a, b in zip(heads[tested], ends[tested]):
        v = np.diff(S[a:b], axis=0)
        with np.errstate(all="ignore"):
            norm = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
            ang = np.arccos(np.clip(v[:, 1] / norm, -1.0, 1.0)) * 180 / np.pi
            med = np.median(ang)
        members = where[order[a:b]]
        info["columns"].append((members, ang, med))
        if med < max_shadow_angle:
            keep[members] = False
            removed_cols += 1
            removed_pts += b - a
    stats[2:6] = [len(heads), tested.sum(), removed_cols, removed_pts]
    return keep, stats, info


def compact(points, colors, keep):
    keep = np.asarray(keep, dtype=bool)
    return points[keep], (None if colors is None else colors[keep])


def clean(points, colors=None, nb_points=20, radius=0.1, shadow_height_threshold=0.1, max_shadow_angle=75,
          min_points_per_column=3):
    """remove_stray_points then clean_shadows: (points, colors, stray keep, shadow keep on the survivors,
    stray stats, shadow stats)."""
    k1, s1 = stray_mask(points, nb_points, radius)
    p1, c1 = compact(points, colors, k1)
    k2, s2, _ = shadow_mask(p1, shadow_height_threshold, max_shadow_angle, min_points_per_column)
    p2, c2 = compact(p1, c1, k2)
    return p2, c2, k1, k2, s1, s2
