"""numpy restatement of the "Triangle mesh" specification in include/dp_mi355x.h (additive to ABI 20):
the exact k nearest other rows with the ring statistic, the mean neighbour distance, the fan of triangles and
the removal of invalid, degenerate and duplicated triangles.

Written from the header's numbered rules, not from the kernels: the search is a brute-force fp64 distance
matrix with the header's expression, ordered by np.lexsort on (row, d2); the clean-up is a dictionary of
canonical forms.  tests/golden/make_golden_mesh.py pins the search to scipy.spatial.cKDTree.query(k + 1).
"""

import numpy as np

CELL_MAX = (1 << 21) - 2
KNN_STATS = ("finite", "non_finite", "few_neighbors", "max_ring", "error", "reserved0", "reserved1", "reserved2")
TRI_STATS = ("input", "invalid", "degenerate", "duplicated", "kept", "error", "reserved0", "reserved1")


def _live(points, count):
    pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    n = len(pts) if count is None else max(0, min(int(count), len(pts)))
    return pts[:n], n


def ring_of(d2, edge, cover):
    """Rule 4's distance part: per entry the smallest r >= 0 with d2 < (r * edge) * (r * edge), capped at cover."""
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.clip(np.nan_to_num(np.floor(np.sqrt(d2) / edge) - 2.0, nan=0.0, posinf=float(CELL_MAX)), 0, cover).astype(np.int64)
    while True:
        lim = r.astype(np.float64) * edge
        open_ = (r < cover) & ~(d2 < lim * lim)
        if not open_.any():
            return r
        r = r + open_


def knn_exact(points, count=None, k=6, cell_edge=0.1, chunk=512):
    """-> (nbr (n, k) int32 padded with -1; nbr_count (n,) int32; d2 (n, k) float64, NaN past the count; stats (8,);
    ties: True if, for some row, the k-th and the (k+1)-th smallest other row have equal d2 -- the cut by row decides)."""
    pts, n = _live(points, count)
    fin = np.isfinite(pts).all(axis=1)
    stats = np.zeros(8)
    stats[0], stats[1] = fin.sum(), n - fin.sum()
    nbr = np.full((n, k), -1, dtype=np.int32)
    cnt = np.zeros(n, dtype=np.int32)
    d2o = np.full((n, k), np.nan)
    rows = np.flatnonzero(fin)
    if not len(rows):
        return nbr, cnt, d2o, stats, False
    P = pts[rows]
    g = cell_edge * (1.0 + 1.0 / 1048576.0)
    origin = P.min(axis=0)
    with np.errstate(over="ignore", invalid="ignore"):
        err = bool(np.any(~((P.max(axis=0) - origin) / g < CELL_MAX)))
    if err:
        stats[2], stats[4] = fin.sum(), 1
        return nbr, cnt, d2o, stats, False
    m = min(k, len(rows) - 1)
    ties = False
    for a in range(0, len(rows), chunk):
        q = P[a:a + chunk]
        dx, dy, dz = (P[None, :, c] - q[:, None, c] for c in range(3))
        d2 = (dx * dx + dy * dy) + dz * dz
        d2[np.arange(len(q)), a + np.arange(len(q))] = np.inf               # the query itself, by identity
        order = np.lexsort((np.broadcast_to(rows, d2.shape), d2), axis=-1)[:, :m + 1]
        srt = np.take_along_axis(d2, order, axis=1)
        if m < len(rows) - 1:
            ties |= bool(np.any(srt[:, m - 1] == srt[:, m])) if m else False
        nbr[rows[a:a + chunk], :m] = rows[order[:, :m]]
        d2o[rows[a:a + chunk], :m] = srt[:, :m]
        cnt[rows[a:a + chunk]] = m
    cells = np.clip(np.floor((P - origin) / g), 0, CELL_MAX).astype(np.int64)
    ext = cells.max(axis=0)
    cover = np.maximum(cells, ext - cells).max(axis=1)
    ring = cover if m < k else ring_of(d2o[rows, k - 1], cell_edge, cover)
    stats[2] = len(rows) if m < k else 0
    stats[3] = ring.max()
    return nbr, cnt, d2o, stats, ties


def mean_neighbor_distance(d2, nbr_count):
    """Rules 1 and 2 of the mean neighbour distance -> (mean, rows with a neighbour)."""
    d2, m = np.asarray(d2, dtype=np.float64), np.asarray(nbr_count)
    n, k = d2.shape
    s = np.zeros(n)
    with np.errstate(invalid="ignore"):
        for j in range(k):
            s = s + np.where(j < m, np.sqrt(np.where(j < m, d2[:, j], 0.0)), 0.0)
        rm = np.where(m > 0, s / np.maximum(m, 1), 0.0)
    has = (m > 0).astype(np.float64)
    pad = (-n) % 256
    rm, has = np.r_[rm, np.zeros(pad)].reshape(-1, 256), np.r_[has, np.zeros(pad)].reshape(-1, 256)
    part, cnt = np.zeros(256), np.zeros(256)
    for j in range(len(rm)):                                    # partial t takes rows t, t + 256, ... in turn
        part, cnt = part + rm[j], cnt + has[j]
    part, cnt = part.reshape(4, 64), cnt.reshape(4, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        part, cnt = part + part[:, lane ^ o], cnt + cnt[:, lane ^ o]
    tot = ((part[0, 0] + part[1, 0]) + part[2, 0]) + part[3, 0]
    rows = ((cnt[0, 0] + cnt[1, 0]) + cnt[2, 0]) + cnt[3, 0]
    return (tot / rows if rows > 0 else 0.0), rows


def fan(nbr, nbr_count, count=None):
    """-> (n * (k - 1), 3) int32: slot i * (k - 1) + j = (i, nbr[i, j], nbr[i, j + 1]) for j < m - 1, else -1."""
    nbr = np.asarray(nbr)
    n = len(nbr) if count is None else max(0, min(int(count), len(nbr)))
    k = nbr.shape[1]
    tri = np.full((n, k - 1, 3), -1, dtype=np.int32)
    m = np.minimum(np.asarray(nbr_count)[:n], k)
    for j in range(k - 1):
        on = j + 1 < m
        tri[on, j, 0] = np.flatnonzero(on)
        tri[on, j, 1] = nbr[:n][on, j]
        tri[on, j, 2] = nbr[:n][on, j + 1]
    return tri.reshape(-1, 3)


def canonical(t):
    a, b, c = (int(v) for v in t)
    return min((a, b, c), (b, c, a), (c, a, b))


def clean_triangles(tri, n_vertices, count=None):
    """-> (kept triangles (t_out, 3) int32 in input order and as they came, stats (8,))."""
    tri = np.asarray(tri, dtype=np.int64).reshape(-1, 3)
    t = len(tri) if count is None else max(0, min(int(count), len(tri)))
    stats = np.zeros(8)
    stats[0] = t
    seen, keep = set(), []
    for i in range(t):
        a, b, c = tri[i]
        if not all(0 <= v < n_vertices for v in (a, b, c)):
            stats[1] += 1
        elif a == b or b == c or a == c:
            stats[2] += 1
        elif canonical(tri[i]) in seen:
            stats[3] += 1
        else:
            seen.add(canonical(tri[i]))
            keep.append(i)
    stats[4] = len(keep)
    return tri[keep].astype(np.int32).reshape(-1, 3), stats


def simple_mesh(points, neighbors=6, cell_edge=0.1, count=None):
    """knn_exact, fan, clean_triangles over points that are already down-sampled -> (triangles, knn stats, triangle stats)."""
    pts, n = _live(points, count)
    nbr, cnt, _, kst, _ = knn_exact(pts, None, neighbors, cell_edge)
    tri, tst = clean_triangles(fan(nbr, cnt), len(np.asarray(points).reshape(-1, 3)))
    return tri, kst, tst
