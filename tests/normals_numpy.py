"""numpy restatement of the "Oriented mesh points" specification in include/dp_mi355x.h (ABI 19):
voxel grid, hybrid (radius + max_nn) neighbour search, two-pass PCA normals, orientation.

Written from the header's sentences, not from the kernels: the search is brute force over all pairs,
the voxel grid is np.unique over the packed keys.  tests/golden/make_golden_normals.py pins it to
scipy.spatial.cKDTree (neighbour sets), numpy.linalg.eigh (eigenvalues) and np.unique of the floor
indices (voxel membership).  The eigen-solver follows the header's method (cyclic Jacobi, rotations
(0,1), (0,2), (1,2), stop when the off-diagonal sum no longer changes the diagonal sum) operation for
operation, and the sums run in list order, so that an eigenvector's arbitrary sign comes out as on the
device and the `flipped` counts can be compared.
"""

import numpy as np

CELL_MAX = (1 << 21) - 2
STATS = ("finite", "non_finite", "voxels_or_few_neighbors", "truncated", "flipped", "error", "reserved0", "reserved1")


def _live(points, count):
    pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    n = len(pts) if count is None else max(0, min(int(count), len(pts)))
    return pts[:n], n


def _cells(pts, fin, origin, edge):
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.floor((pts[fin] - origin) / edge)
    return np.clip(q, 0, CELL_MAX).astype(np.int64)


def _span_error(pts, fin, origin, edge):
    if not fin.any():
        return False
    with np.errstate(over="ignore", invalid="ignore"):
        return bool(np.any(~((pts[fin].max(axis=0) - origin) / edge < CELL_MAX)))


def voxel_downsample(points, colors=None, count=None, voxel_size=0.05):
    """-> dict: points (n_out, 3), colors (n_out, 3) or None, count (n_out,), voxel_of (n,), n_out, keys (n_out,),
    bound (n_out, 3): the summation bound 4 * 2^-53 * m * max |coordinate in the voxel|, stats (8,)."""
    pts, n = _live(points, count)
    fin = np.isfinite(pts).all(axis=1)
    origin = (pts[fin].min(axis=0) if fin.any() else np.zeros(3)) - voxel_size / 2
    stats = np.zeros(8)
    stats[0], stats[1] = fin.sum(), n - fin.sum()
    voxel_of = np.full(n, -1, dtype=np.int32)
    err = _span_error(pts, fin, origin, voxel_size)
    stats[5] = err
    if err or not fin.any():
        return {"points": np.zeros((0, 3)), "colors": None if colors is None else np.zeros((0, 3), np.uint8),
                "count": np.zeros(0, np.int32), "voxel_of": voxel_of, "n_out": 0, "keys": np.zeros(0, np.int64),
                "bound": np.zeros((0, 3)), "stats": stats}
    c = _cells(pts, fin, origin, voxel_size)
    key = (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]
    keys, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    voxel_of[fin] = inv
    k = len(keys)
    out = np.stack([np.bincount(inv, weights=pts[fin][:, a], minlength=k) for a in range(3)], axis=1) / cnt[:, None]
    amax = np.zeros((k, 3))
    np.maximum.at(amax, inv, np.abs(pts[fin]))
    cols = None
    if colors is not None:
        col = np.asarray(colors, dtype=np.uint8).reshape(-1, 3)[:n][fin].astype(np.int64)
        s = np.stack([np.bincount(inv, weights=col[:, a], minlength=k).astype(np.int64) for a in range(3)], axis=1)
        cols = ((2 * s + cnt[:, None]) // (2 * cnt[:, None])).astype(np.uint8)
    stats[2] = k
    return {"points": out, "colors": cols, "count": cnt.astype(np.int32), "voxel_of": voxel_of, "n_out": k, "keys": keys,
            "bound": 4 * 2.0 ** -53 * cnt[:, None] * amax, "stats": stats}


def knn_search(points, count=None, radius=0.1, max_nn=30, chunk=512):
    """-> (nbr (n, max_nn) int32, padded with -1; nbr_count (n,) int32; stats (8,); total (n,): neighbours before
    the cut; ties: True if two neighbours of one row that the cut could tell apart only by the row have equal d2)."""
    pts, n = _live(points, count)
    fin = np.isfinite(pts).all(axis=1)
    stats = np.zeros(8)
    stats[0], stats[1] = fin.sum(), n - fin.sum()
    nbr = np.full((n, max_nn), -1, dtype=np.int32)
    cnt = np.zeros(n, dtype=np.int32)
    total = np.zeros(n, dtype=np.int64)
    edge = radius * (1.0 + 1.0 / 1048576.0)
    err = _span_error(pts, fin, pts[fin].min(axis=0) if fin.any() else np.zeros(3), edge)
    stats[5] = err
    if err:
        stats[2] = fin.sum()
        return nbr, cnt, stats, total, False
    r2 = radius * radius
    rows = np.flatnonzero(fin)
    P = pts[rows]
    ties = False
    for a in range(0, len(rows), chunk):
        q = P[a:a + chunk]
        dx, dy, dz = (P[None, :, k] - q[:, None, k] for k in range(3))
        d2 = (dx * dx + dy * dy) + dz * dz
        hit = d2 < r2
        d2 = np.where(hit, d2, np.inf)
        order = np.argsort(d2, axis=1, kind="stable")[:, :max_nn + 1]          # ties: the smaller row first
        tot = hit.sum(axis=1)
        srt = np.take_along_axis(d2, order, axis=1)
        ties |= bool(np.any((srt[:, 1:] == srt[:, :-1]) & np.isfinite(srt[:, 1:])))
        for i in range(len(q)):
            m = min(int(tot[i]), max_nn)
            nbr[rows[a + i], :m] = rows[order[i, :m]]
            cnt[rows[a + i]] = m
        total[rows[a:a + chunk]] = tot
    stats[2] = np.count_nonzero(total[fin] < 3)
    stats[3] = np.count_nonzero(total > max_nn)
    return nbr, cnt, stats, total, ties


def covariance(points, nbr, nbr_count):
    """Two passes in list order -> (mean (n, 3), C (n, 3, 3)); rows with fewer than 3 neighbours get zeros."""
    pts = np.asarray(points, dtype=np.float64)
    n, max_nn = nbr.shape
    m = np.where(nbr_count >= 3, nbr_count, 0)
    safe = np.where(nbr >= 0, nbr, 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.zeros((n, 3))
        for k in range(max_nn):
            s = s + np.where((k < m)[:, None], pts[safe[:, k]], 0.0)
        mean = np.where((m > 0)[:, None], s / m[:, None], 0.0)
        a = np.zeros((n, 6))
        for k in range(max_nn):
            d = np.where((k < m)[:, None], pts[safe[:, k]] - mean, 0.0)
            a = a + np.stack([d[:, 0] * d[:, 0], d[:, 0] * d[:, 1], d[:, 0] * d[:, 2], d[:, 1] * d[:, 1], d[:, 1] * d[:, 2],
                              d[:, 2] * d[:, 2]], axis=1)
        a = np.where((m > 0)[:, None], a / m[:, None], 0.0)
    C = np.empty((n, 3, 3))
    C[:, 0, 0], C[:, 0, 1], C[:, 0, 2], C[:, 1, 1], C[:, 1, 2], C[:, 2, 2] = a.T
    C[:, 1, 0], C[:, 2, 0], C[:, 2, 1] = C[:, 0, 1], C[:, 0, 2], C[:, 1, 2]
    return mean, C


def jacobi_eigh(C):
    """Cyclic Jacobi on a stack of symmetric 3 x 3 -> (diagonal (n, 3), V (n, 3, 3), columns = vectors), not sorted."""
    A = np.array(C, dtype=np.float64)
    n = len(A)
    V = np.tile(np.eye(3), (n, 1, 1))
    with np.errstate(all="ignore"):
        for _ in range(24):
            off = (np.abs(A[:, 0, 1]) + np.abs(A[:, 0, 2])) + np.abs(A[:, 1, 2])
            dia = (np.abs(A[:, 0, 0]) + np.abs(A[:, 1, 1])) + np.abs(A[:, 2, 2])
            live = (off > 0.0) & ~(dia + off == dia)
            if not live.any():
                break
            for p, q, r in ((0, 1, 2), (0, 2, 1), (1, 2, 0)):
                app, aqq, apq, apr, aqr = A[:, p, p], A[:, q, q], A[:, p, q], A[:, p, r], A[:, q, r]
                act = live & (apq != 0.0)
                theta = (aqq - app) / (2.0 * apq)
                t = np.where(theta < 0.0, -1.0, 1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                new = {(p, p): app - t * apq, (q, q): aqq + t * apq, (p, q): np.zeros(n), (p, r): c * apr - s * aqr,
                       (q, r): s * apr + c * aqr}
                vp, vq = V[:, :, p].copy(), V[:, :, q].copy()
                for (i, j), val in new.items():
                    val = np.where(act, val, A[:, i, j])
                    A[:, i, j] = val
                    A[:, j, i] = val
                V[:, :, p] = np.where(act[:, None], c[:, None] * vp - s[:, None] * vq, vp)
                V[:, :, q] = np.where(act[:, None], s[:, None] * vp + c[:, None] * vq, vq)
    return np.stack([A[:, 0, 0], A[:, 1, 1], A[:, 2, 2]], axis=1), V


def estimate_normals(points, nbr, nbr_count, count=None, camera=(0.0, 0.0, 0.0), orient=True):
    """-> dict: normals (n, 3), stats (8,), C (n, 3, 3), lam (n, 3) ascending eigenvalues (the Jacobi's), dot (n,):
    n . (camera - p) before the flip, dist (n,) = |camera - p|."""
    pts, n = _live(points, count)
    nbr, nbr_count = np.asarray(nbr)[:n], np.asarray(nbr_count)[:n]
    fin = np.isfinite(pts).all(axis=1)
    _, C = covariance(pts, nbr, nbr_count)
    d, V = jacobi_eigh(C)
    s1 = d[:, 1] < d[:, 0]
    e1 = np.where(s1, d[:, 1], d[:, 0])
    s2 = d[:, 2] < e1
    col = np.where(s2, 2, np.where(s1, 1, 0))
    vec = np.take_along_axis(V, col[:, None, None], axis=2)[:, :, 0]
    with np.errstate(all="ignore"):
        ln = np.sqrt((vec[:, 0] * vec[:, 0] + vec[:, 1] * vec[:, 1]) + vec[:, 2] * vec[:, 2])
        ok = (nbr_count >= 3) & (ln > 0) & np.isfinite(ln)
        normals = np.where(ok[:, None], vec / ln[:, None], np.array([0.0, 0.0, 1.0]))
        cam = np.asarray(camera, dtype=np.float64)
        to = cam - pts
        dot = (normals[:, 0] * to[:, 0] + normals[:, 1] * to[:, 1]) + normals[:, 2] * to[:, 2]
        dist = np.sqrt((to * to).sum(axis=1))
    flip = fin & (dot < 0) & bool(orient)
    normals = np.where(flip[:, None], -normals, normals)
    normals[~fin] = 0.0
    stats = np.zeros(8)
    stats[0], stats[1] = fin.sum(), n - fin.sum()
    stats[2] = np.count_nonzero(fin & (nbr_count < 3))
    stats[4] = flip.sum()
    return {"normals": normals, "stats": stats, "C": C, "lam": np.sort(d, axis=1), "dot": dot, "dist": dist, "flip": flip}
