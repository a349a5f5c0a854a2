"""Makes tests/golden/golden_mesh.npz: the random cloud of tests/test_mesh.py (triangle mesh, additive to ABI 20)
with what scipy's cKDTree says about it and about the down-sampled cloud A of golden_normals.npz, and asserts
the properties that make the restatement in tests/mesh_numpy.py a fair yardstick.  CPU only, seeded:

    python tests/golden/make_golden_mesh.py

Cloud R (400 points, seed 11): uniform in a 1 m cube.  Cloud A down-sampled: cloud A of golden_normals.npz
through the restated 0.05 m voxel grid (1664 voxels).

Asserted for R at k = 6 and k = 20 and for the down-sampled A at k = 6 (a cloud that violates one is changed,
never excused):
 (a) no row has two candidates that tie at the cut (k-th against (k+1)-th smallest d2), so the neighbour
     sets do not depend on the order among equal distances, which Open3D and scipy leave open;
 (b) cKDTree.query(k + 1) lists the query itself first, and the k entries behind it are the restatement's
     list, in its order;
 (c) the square roots of the restatement's d2 equal cKDTree's distances to 1 ulp.
The cKDTree lists are stored, so the non-GPU tests check (b) again without trusting this run.
"""

import os
import sys

import numpy as np
from scipy.spatial import cKDTree

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import mesh_numpy as M  # noqa: E402
import normals_numpy as N  # noqa: E402


def pin(P, k, edge, name):
    nbr, cnt, d2, stats, ties = M.knn_exact(P, None, k, edge)
    assert not ties and (cnt == k).all(), name                                                # (a)
    dist, idx = cKDTree(P).query(P, k=k + 1)
    assert np.array_equal(idx[:, 0], np.arange(len(P))), name                                 # (b)
    assert np.array_equal(np.sort(idx[:, 1:], axis=1), np.sort(nbr, axis=1)), name
    assert np.array_equal(idx[:, 1:], nbr), name
    root = np.sqrt(d2)
    assert (np.abs(root - dist[:, 1:]) <= np.spacing(root)).all(), name                       # (c)
    print(f"{name}: n={len(P)} k={k} max ring {int(stats[3])}, largest |sqrt(d2) - kd| / ulp "
          f"{np.max(np.abs(root - dist[:, 1:]) / np.spacing(root)):.2f}")
    return idx[:, 1:].astype(np.int16)


def main():
    R = np.ascontiguousarray(np.random.default_rng(11).uniform(0.0, 1.0, (400, 3)))
    g = np.load(os.path.join(HERE, "golden_normals.npz"))
    down = N.voxel_downsample(g["A_points"], None, None, 0.05)["points"]
    assert len(down) == 1664
    out = os.path.join(HERE, "golden_mesh.npz")
    np.savez_compressed(out, R_points=R, R_kd6=pin(R, 6, 0.1, "R"), R_kd20=pin(R, 20, 0.1, "R"),
                        A_down_kd6=pin(down, 6, 0.1, "A down-sampled"))
    print(f"wrote {out} ({os.path.getsize(out)} bytes)")


if __name__ == "__main__":
    main()
