"""Golden vectors for the clustering stage, from sklearn's DBSCAN -- the reference's own clustering
call (`DBSCAN(eps=..., min_samples=...).fit(points_2d)`, simple_pointcloud_viewer.py:347).

Run where sklearn is installed:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_cluster.py

Per scene golden_cluster.npz holds the points (n, 3), eps, min_samples, the height threshold, and
sklearn's `labels_` and `core_sample_indices_` over the participants (the finite rows with
y >= threshold, in row order; their (x, z) is what sklearn is given).  Every scene has at least 64
participants (below about a dozen sklearn searches by brute force, which rounds differently).

The generator asserts what the tests rely on:
 (a) no pair of participants has |d^2 - eps^2| <= 1e-12 eps^2 unless d^2 == eps^2 exactly in fp64, so
     agreement does not depend on how a kd-tree rounds;
 (b) tests/cluster_numpy.py reproduces sklearn's labels and core set exactly on every scene;
 (c) the bridge scene is one cluster and loses that when the bridge is taken out; the shared-border
     scene is two clusters whose shared point is a border point with core neighbours in both.
"""

import os
import sys

import numpy as np
from sklearn.cluster import DBSCAN

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "tests"))


def blobs(seed):
    """Five Gaussian blobs and uniform clutter, 1 500 points, shuffled; about one row in eight is
    below the 1.3 m threshold."""
    g = np.random.default_rng(seed)
    centres = g.uniform(-2.0, 2.0, (5, 2))
    parts = [c + g.normal(0.0, s, (260, 2)) for c, s in zip(centres, (0.10, 0.15, 0.20, 0.25, 0.30))]
    parts.append(g.uniform(-3.0, 3.0, (200, 2)))
    xz = np.concatenate(parts)
    g.shuffle(xz)
    y = np.where(g.random(len(xz)) < 0.125, g.uniform(0.0, 1.29, len(xz)), g.uniform(1.3, 2.5, len(xz)))
    y[:4] = 1.3                                                   # exactly at the threshold: takes part
    return np.c_[xz[:, 0], y, xz[:, 1]], 0.08, 5, 1.3


def lattice():
    """20 x 20 at spacing exactly 0.25 = eps: dx*dx == eps*eps holds exactly for the four axis neighbours."""
    u, v = np.meshgrid(0.25 * np.arange(20), 0.25 * np.arange(20), indexing="ij")
    return np.c_[u.ravel(), np.full(400, 2.0), v.ravel()], 0.25, 5, 1.3


def levelled():
    """The 'side' scene of golden_ground.npz, levelled, then through the clean restatement."""
    import clean_numpy as C

    pts = np.load(os.path.join(HERE, "golden_ground.npz"))["side_normalized"]
    pts = C.clean(pts)[0]
    return np.ascontiguousarray(pts), 0.05, 5, float(np.median(pts[:, 1]))


def _line(x0, step, k, g):
    return np.c_[x0 + step * np.arange(k), 1e-4 * g.standard_normal(k)]


def bridge(with_bridge=True):
    """Two dense blobs 1 m apart joined by a line of points 0.04 apart: with eps 0.1 and min_samples 5
    each bridge point has itself and two on each side, so the bridge is core and one point wide."""
    g = np.random.default_rng(11)
    a = g.normal(0.0, 0.02, (60, 2))
    b = np.array([1.0, 0.0]) + g.normal(0.0, 0.02, (60, 2))
    parts = [a, b]
    if with_bridge:
        parts.append(_line(0.07, 0.04, 22, g))                   # 0.07 ... 0.91
    parts.append(g.uniform(-0.5, 1.5, (20, 2)) + np.array([0.0, 2.0]))      # clutter away from the blobs
    parts.append(np.c_[g.uniform(0.1, 0.9, 12), g.uniform(-0.03, 0.03, 12)])   # below the threshold, along the bridge
    xz = np.concatenate(parts)
    y = np.full(len(xz), 2.0)
    y[-12:] = 0.5
    perm = g.permutation(len(xz))
    xz, y = xz[perm], y[perm]
    return np.c_[xz[:, 0], y, xz[:, 1]], 0.1, 5, 1.3


def shared_border():
    """Two lines of points 0.0097 apart (min_samples 10: the end points have exactly themselves and 10
    more), their ends 0.17 apart, and one point between them with two points of each line in reach:
    5 neighbours, not core, a border point of both.  It is row 0, in front of every core point."""
    g = np.random.default_rng(12)
    a = _line(-0.0097 * 40, 0.0097, 41, g)                       # ends at x = 0
    b = _line(0.17, 0.0097, 41, g)
    mid = np.array([[0.085, 0.0]])
    far = g.uniform(-0.5, 0.5, (8, 2)) + np.array([0.0, 3.0])
    xz = np.concatenate([mid, b, far, a])
    return np.c_[xz[:, 0], np.full(len(xz), 2.0), xz[:, 1]], 0.1, 10, 1.3


def check_margin(xz, eps, name):
    e2 = eps * eps
    for s in range(0, len(xz), 1024):
        d = xz[s:s + 1024, None, :] - xz[None, :, :]
        d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
        bad = (np.abs(d2 - e2) <= 1e-12 * e2) & (d2 != e2)
        assert not bad.any(), (name, "a pair within 1e-12 of eps^2: change the seed")


def main():
    import cluster_numpy as N

    scenes = {f"blobs{k}": blobs(100 + k) for k in range(5)}
    scenes["lattice"] = lattice()
    scenes["levelled"] = levelled()
    scenes["bridge"] = bridge()
    scenes["border"] = shared_border()
    out = {"scenes": np.array(list(scenes))}
    for name, (pts, eps, ms, thr) in scenes.items():
        rows = np.flatnonzero(np.isfinite(pts).all(axis=1) & (pts[:, 1] >= thr))
        assert len(rows) >= 64, name
        xz = pts[rows][:, [0, 2]]
        check_margin(xz, eps, name)                                                   # (a)
        db = DBSCAN(eps=eps, min_samples=ms).fit(xz)
        labels, core_rows, stats = N.dbscan(pts, eps, ms, thr)
        assert np.array_equal(labels[rows], db.labels_), (name, "labels differ from sklearn")          # (b)
        assert np.array_equal(core_rows, rows[db.core_sample_indices_]), (name, "core set differs")
        assert (labels[np.setdiff1d(np.arange(len(pts)), rows)] == -2).all()
        out[f"{name}_points"] = pts
        out[f"{name}_params"] = np.array([eps, ms, thr], dtype=np.float64)
        out[f"{name}_labels"] = db.labels_.astype(np.int32)
        out[f"{name}_core"] = db.core_sample_indices_.astype(np.int32)
        print(name, "points", len(pts), "participants", len(rows), "clusters", int(db.labels_.max()) + 1, "core",
              len(db.core_sample_indices_), "noise", int((db.labels_ == -1).sum()), "border",
              int((db.labels_ >= 0).sum()) - len(db.core_sample_indices_))
    # (c)
    lb = N.dbscan(*bridge())[0]
    blob_rows = lambda p, c: np.flatnonzero((np.hypot(p[:, 0] - c, p[:, 2]) < 0.06) & (p[:, 1] >= 1.3))   # noqa: E731
    p = bridge()[0]
    assert len(set(lb[blob_rows(p, 0.0)]) | set(lb[blob_rows(p, 1.0)])) == 1
    p2, *par = bridge(False)
    l2 = N.dbscan(p2, *par)[0]
    assert set(l2[blob_rows(p2, 0.0)]) != set(l2[blob_rows(p2, 1.0)])
    pts, eps, ms, thr = shared_border()
    l3, core3, _ = N.dbscan(pts, eps, ms, thr)
    assert l3.max() == 1 and 0 not in core3 and l3[0] == 0
    d2 = (pts[core3, 0] - pts[0, 0]) ** 2 + (pts[core3, 2] - pts[0, 2]) ** 2
    assert set(l3[core3[d2 <= eps * eps]]) == {0, 1}
    path = os.path.join(HERE, "golden_cluster.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
