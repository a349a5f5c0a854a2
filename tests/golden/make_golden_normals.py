"""Makes tests/golden/golden_normals.npz: the three clouds of tests/test_normals.py (ABI 19, oriented mesh
points) with what scipy and numpy say about them, and asserts the properties that make the restatement in
tests/normals_numpy.py a fair yardstick.  CPU only, seeded:

    python tests/golden/make_golden_normals.py

Cloud A (3000 points, seed 7): 1600 on a 1.5 m x 1.5 m plane patch with 2 mm noise, 1100 on a sphere of
radius 0.4 m around (1.5, 0.6, 3.0), 250 on a wall, 50 uniform strays, shuffled; random colours.
Cloud B: a 12 x 12 x 3 integer lattice scaled by 0.04, shuffled: every neighbourhood has distance ties.
Cloud C: cloud A with 5 NaN / inf rows and a live count below its length.

Asserted (a cloud that violates one is changed, never excused):
 (a) cloud A at radius 0.1, max_nn 30: 60 rows with fewer than 3 neighbours, 101 truncated, the largest
     neighbourhood 41, no distance ties, no row with a relative eigen-gap (l1 - l0) / l2 below 1e-6;
     after the 0.05 voxel grid 1664 voxels, 65 of them with fewer than 3 neighbours, again no small gap;
 (b) the restatement's neighbour sets on A and on the down-sampled A equal cKDTree.query(k = 30,
     distance_upper_bound = 0.1);
 (c) its eigenvalues equal numpy.linalg.eigh's within 1e-13 of the largest (two backward-stable solvers on
     one matrix), and its normal is within 1e-9 / gap of eigh's vector;
 (d) its voxel membership equals np.unique(axis = 0) of the floor indices, its voxel points np.add.at's means;
 (e) cloud B at max_nn 8: every row truncated, equal rounded distances in every neighbourhood, and for more
     than half of the rows two of them on either side of the cut, where only the (d2, row) rule decides.
The cKDTree neighbour lists, eigh's eigenvalues and the np.unique inverse of cloud A are stored, so the
non-GPU tests check (b) - (d) again without trusting this run.
"""

import os
import sys

import numpy as np
from scipy.spatial import cKDTree

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import normals_numpy as N  # noqa: E402

RADIUS, MAX_NN, VOXEL = 0.1, 30, 0.05
CENTRE = (1.5, 0.6, 3.0)


def cloud_a():
    rng = np.random.default_rng(7)
    n1 = 1600
    pl = np.c_[rng.uniform(-.75, .75, n1), rng.normal(0, .002, n1), rng.uniform(2, 3.5, n1)]
    v = rng.normal(size=(1100, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    sp = v * 0.4 + CENTRE
    wall = np.c_[rng.uniform(-.75, .75, 250), rng.uniform(0, 1.0, 250), np.full(250, 3.6) + rng.normal(0, .002, 250)]
    st = rng.uniform([-2, 0, 1], [3, 2, 5], (50, 3))
    P = np.r_[pl, sp, wall, st]
    P = P[rng.permutation(len(P))]
    return np.ascontiguousarray(P), rng.integers(0, 256, (len(P), 3), dtype=np.uint8)


def kd_lists(P, radius, k):
    d, i = cKDTree(P).query(P, k=k, distance_upper_bound=radius)
    return np.where(np.isfinite(d), i, -1).astype(np.int32)


def check_search(P, name, few, trunc=None, biggest=None):
    """(a) - (c) on one cloud; returns (kd lists, eigh eigenvalues, largest Rayleigh excess / l2, largest sin * gap)."""
    nbr, cnt, stats, total, ties = N.knn_search(P, None, RADIUS, MAX_NN)
    kd = kd_lists(P, RADIUS, MAX_NN)
    assert not ties, name
    assert np.array_equal(np.sort(nbr, axis=1), np.sort(kd, axis=1)), name                      # (b)
    assert np.array_equal(nbr, kd), name                                                         # no ties: the order too
    assert stats[2] == few == np.count_nonzero(cnt < 3), (name, stats[2])
    if trunc is not None:
        assert stats[3] == trunc and total.max() == biggest, (name, stats[3], total.max())
    out = N.estimate_normals(P, nbr, cnt)
    w, vec = np.linalg.eigh(out["C"])
    rows = np.flatnonzero(cnt >= 3)
    lam = out["lam"]
    assert np.abs(lam[rows] - w[rows]).max(axis=1).max() <= 1e-13 * w[rows, 2].max()
    assert (np.abs(lam[rows] - w[rows]).max(axis=1) <= 1e-13 * w[rows, 2]).all(), name           # (c)
    gap = (w[rows, 1] - w[rows, 0]) / w[rows, 2]
    assert gap.min() >= 1e-6, (name, gap.min())
    n = out["normals"][rows]
    sin = np.linalg.norm(np.cross(n, vec[rows, :, 0]), axis=1)
    assert (sin <= 1e-9 / gap).all(), name
    excess = np.einsum("ni,nij,nj->n", n, out["C"][rows], n) - w[rows, 0]
    print(f"{name}: n={len(P)} few={few} truncated={int(stats[3])} largest={int(total.max())} min gap={gap.min():.3e} "
          f"Rayleigh excess / l2 <= {np.max(excess / w[rows, 2]):.3e}  sin * gap <= {np.max(sin * gap):.3e}")
    return kd, w


def main():
    A, colors = cloud_a()
    kd, w = check_search(A, "A", 60, 101, 41)                                                     # (a)
    vox = N.voxel_downsample(A, colors, None, VOXEL)
    mb = A.min(axis=0) - VOXEL * 0.5                                                              # (d)
    idx = np.floor((A - mb) / VOXEL).astype(np.int64)
    u, inv = np.unique(idx, axis=0, return_inverse=True)
    inv = inv.ravel()
    assert vox["n_out"] == len(u) == 1664 and np.array_equal(vox["voxel_of"], inv)
    assert np.array_equal(vox["keys"], (u[:, 0] << 42) | (u[:, 1] << 21) | u[:, 2]) and (np.diff(vox["keys"]) > 0).all()
    D = np.zeros((len(u), 3))
    np.add.at(D, inv, A)
    D /= np.bincount(inv)[:, None]
    assert (np.abs(vox["points"] - D) <= vox["bound"]).all() and np.array_equal(vox["count"], np.bincount(inv))
    m = np.bincount(inv)
    sums = np.stack([np.bincount(inv, weights=colors[:, a]).astype(np.int64) for a in range(3)], axis=1)
    halves = (2 * sums) % (2 * m[:, None]) == m[:, None]
    assert np.array_equal(vox["colors"][~halves], np.rint(sums / m[:, None])[~halves].astype(np.uint8))   # off a half: plain rounding
    assert np.array_equal(vox["colors"][halves], (sums // m[:, None] + 1)[halves].astype(np.uint8)) and halves.any()
    check_search(vox["points"], "A down-sampled", 65)

    g = np.random.default_rng(8)
    i, j, k = np.meshgrid(np.arange(12), np.arange(12), np.arange(3), indexing="ij")
    B = np.c_[i.ravel(), j.ravel(), k.ravel()].astype(np.float64) * 0.04
    B = np.ascontiguousarray(B[g.permutation(len(B))])
    nbr, cnt, stats, total, ties = N.knn_search(B, None, RADIUS, 8)                               # (e)
    assert ties and (total > 8).all() and stats[3] == len(B) and (cnt == 8).all() and total.max() <= 64

    def d2_of(lists):                       # the specification's expression, so a tie here is a tie there
        d = np.where(lists[:, :, None] >= 0, B[lists] - B[:, None, :], np.nan)
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]

    full = d2_of(N.knn_search(B, None, RADIUS, 64)[0])
    assert (np.diff(full, axis=1) == 0).any(axis=1).all()                  # every neighbourhood has ties (as rounded)
    at_cut = np.count_nonzero(full[:, 7] == full[:, 8])
    assert 2 * at_cut > len(B), at_cut                                     # and for most rows one straddles the cut
    print(f"B: n={len(B)} neighbourhoods {total.min()}..{total.max()}, a tie across the cut in {at_cut} rows")

    C = A.copy()
    bad = g.choice(2900, 5, replace=False)
    C[bad[0], 0] = np.nan
    C[bad[1], 1] = np.inf
    C[bad[2], 2] = -np.inf
    C[bad[3]] = np.nan
    C[bad[4], 1] = np.nan
    count = 2900
    assert N.knn_search(C, count, RADIUS, MAX_NN)[2][1] == 5

    out = os.path.join(HERE, "golden_normals.npz")
    np.savez_compressed(out, A_points=A, A_colors=colors, B_points=B, C_points=C, C_count=np.int32(count),
                        C_bad=np.sort(bad).astype(np.int32), A_kd=kd.astype(np.int16), A_eigh=w,
                        A_unique_inverse=inv.astype(np.int16), sphere_centre=np.array(CENTRE),
                        params=np.array([RADIUS, MAX_NN, VOXEL]))
    print(f"wrote {out} ({os.path.getsize(out)} bytes)")


if __name__ == "__main__":
    main()
