"""numpy restatement of the clustering stage's specification (include/dp_mi355x.h, "Clustered point
clouds"): rules 1-5 and the sampling rule.  Tests compare the device against it; the golden fixture
(tests/golden/golden_cluster.npz, made with sklearn) pins the restatement itself.

The neighbour search is a plain cell grid of edge eps * (1 + 2^-20) with 3 x 3 candidate cells (not
the kernel's grid, and no code shared with the package); every candidate pair is then tested as the
specification words it: dx*dx + dz*dz <= eps*eps, each product and sum rounded on its own in fp64.
"""

import numpy as np


def participants(points, height_threshold=None, max_points=0):
    """Row indices of the participants, ascending."""
    P = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    ok = np.isfinite(P).all(axis=1)
    if height_threshold is not None and not np.isnan(height_threshold):
        ok &= P[:, 1] >= height_threshold
    rows = np.flatnonzero(ok)
    e, m = len(rows), int(max_points)
    if m > 0 and e > m:
        k = np.arange(e, dtype=np.int64)
        take = (k * m) // e != ((k - 1) * m) // e
        take[0] = True
        rows = rows[take]
    return rows


def neighbour_pairs(x, z, eps):
    """All ordered pairs (i, j), i == j included, with dx*dx + dz*dz <= eps*eps."""
    m = len(x)
    if m == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    edge = eps * (1.0 + 2.0 ** -20)
    cx = np.floor((x - x.min()) / edge).astype(np.int64)
    cz = np.floor((z - z.min()) / edge).astype(np.int64)
    W = int(cz.max()) + 3
    cell = (cx + 1) * W + (cz + 1)
    order = np.argsort(cell, kind="stable")
    sc = cell[order]
    out_i, out_j = [], []
    for dxc in (-1, 0, 1):
        # the three z-adjacent cells of one x row are one run of the sorted cell ids
        lo = np.searchsorted(sc, cell + dxc * W - 1, side="left")
        hi = np.searchsorted(sc, cell + dxc * W + 1, side="right")
        cnt = hi - lo
        i = np.repeat(np.arange(m), cnt)
        start = np.repeat(lo - (np.cumsum(cnt) - cnt), cnt)
        j = order[np.arange(cnt.sum()) + start]
        dx, dz = x[j] - x[i], z[j] - z[i]
        near = dx * dx + dz * dz <= eps * eps
        out_i.append(i[near])
        out_j.append(j[near])
    return np.concatenate(out_i), np.concatenate(out_j)


def dbscan(points, eps=0.2, min_samples=5, height_threshold=None, max_points=0):
    """(labels (n,) int32: cluster, -1 noise, -2 not a participant; core rows (ascending); stats (8,)
    in depth_pro.pointcloud.CLUSTER_STATS order, error flag 0)."""
    P = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n = len(P)
    rows = participants(P, height_threshold, max_points)
    x, z = P[rows, 0], P[rows, 2]
    m = len(rows)
    i, j = neighbour_pairs(x, z, eps)
    core = np.bincount(i, minlength=m) >= min_samples                      # rule 2
    # rule 3: components of the core-core neighbour graph; comp[a] = smallest member, by min
    # propagation with pointer jumping (participants are in row order, so smallest index = smallest row)
    cc = core[i] & core[j]
    ei, ej = i[cc], j[cc]
    comp = np.arange(m)
    while True:
        new = comp.copy()
        np.minimum.at(new, ei, comp[ej])
        new = new[new]
        if np.array_equal(new, comp):
            break
        comp = new
    roots = np.flatnonzero(core & (comp == np.arange(m)))
    number = np.full(m, -1, dtype=np.int64)
    number[roots] = np.arange(len(roots))
    lab = np.full(m, -1, dtype=np.int64)
    lab[core] = number[comp[core]]
    bc = ~core[i] & core[j]                                                 # rule 4
    best = np.full(m, np.iinfo(np.int64).max)
    np.minimum.at(best, i[bc], lab[j[bc]])
    border = ~core & (best != np.iinfo(np.int64).max)
    lab[border] = best[border]
    labels = np.full(n, -2, dtype=np.int32)                                 # rule 5
    labels[rows] = lab
    finite = int(np.isfinite(P).all(axis=1).sum())
    stats = np.array([finite, n - finite, m, core.sum(), border.sum(), m - core.sum() - border.sum(), len(roots), 0],
                     dtype=np.float64)
    return labels, rows[core], stats


def table(points, labels, core_rows=None):
    """Per cluster: count, smallest core row (-1 without core_rows), x min, x max, z min, z max, y min,
    y max (exact), then order and offsets; the sums are left to math.fsum in the tests."""
    P = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    labels = np.asarray(labels)
    k = int(labels.max()) + 1 if len(labels) and labels.max() >= 0 else 0
    lab_rows = np.flatnonzero(labels >= 0)
    order = lab_rows[np.argsort(labels[lab_rows], kind="stable")]
    offsets = np.searchsorted(labels[order], np.arange(k + 1), side="left")
    t = np.zeros((k, 8))
    for c in range(k):
        r = order[offsets[c]:offsets[c + 1]]
        mc = -1
        if core_rows is not None:
            cr = np.asarray(core_rows)
            mc = cr[labels[cr] == c].min()
        t[c] = [len(r), mc, P[r, 0].min(), P[r, 0].max(), P[r, 2].min(), P[r, 2].max(), P[r, 1].min(), P[r, 1].max()]
    return t, order.astype(np.int64), offsets.astype(np.int64)
