"""Makes tests/golden/golden_shapes.npz: hand-built 2-D clusters for the shape stage (ABI 18) with the
results of the reference's own calls on them -- scipy.spatial.ConvexHull and scipy.optimize.leastsq
(simple_pointcloud_viewer.py:12-77) -- and asserts the conditions that make those results a fair
yardstick for any implementation of the header's specification.  CPU only:

    python tests/golden/make_golden_shapes.py

Conditions (a scene that violates one is changed, never excused):
 (a) in every cluster every member triple's rounded orientation o(a, b, c) has the exact sign: the
     fp64 value is outside its forward error bound, or (lattice coordinates) equal to the exact value
     computed in integers.  Then every correct algorithm on the predicate gives the same vertex list.
 (b) the restatement's vertex set equals qhull's and its area is within 1e-12 relative of hull.volume.
 (c) each of the three decision criteria has the same truth value under scipy's circle and under the
     restatement's, and every criterion that decides the outcome (all three for a circle, one false one
     for a rectangle) is at least 5 % of its threshold away from it.
 (d) for the clusters the reference calls circles, d_ref = max |restatement - leastsq| over
     (xc, yc, r); the largest is stored as circle_tol.
"""

import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import cluster_numpy as CN  # noqa: E402
import shapes_numpy as S  # noqa: E402

EPS_DBL = 2.0 ** -53
THRESHOLDS = (0.85, 0.15, 0.3)


def ring(g, n, r, noise):
    t = g.uniform(0, 2 * np.pi, n)
    rr = r + g.normal(0, noise, n)
    return np.c_[rr * np.cos(t), rr * np.sin(t)]


def disc(g, n, r):
    t, rr = g.uniform(0, 2 * np.pi, n), r * np.sqrt(g.uniform(0, 1, n))
    return np.c_[rr * np.cos(t), rr * np.sin(t)]


def box(g, n, w, h, deg):
    p = np.c_[g.uniform(-w / 2, w / 2, n), g.uniform(-h / 2, h / 2, n)]
    a = np.radians(deg)
    return np.c_[p[:, 0] * np.cos(a) - p[:, 1] * np.sin(a), p[:, 0] * np.sin(a) + p[:, 1] * np.cos(a)]


def scenes():
    """name -> (list of 2-D clusters, eps, min_samples); clusters are laid out 4 m apart."""
    g = np.random.default_rng(18)
    out = {}
    out["rings"] = ([ring(g, 300, 0.5, 0.01), ring(g, 400, 0.5, 0.01), ring(g, 200, 0.2, 0.004), ring(g, 350, 0.8, 0.01)],
                    0.2, 5)
    out["noisy_ring"] = ([ring(g, 400, 0.5, 0.1)], 0.2, 5)
    out["filled"] = ([disc(g, 400, 0.5), box(g, 400, 1.0, 1.0, 0.0), disc(g, 300, 0.3)], 0.2, 5)
    sq = np.array([[x, y] for x in (-0.5, 0.5) for y in (-0.5, 0.5)])
    tie = np.concatenate([sq, box(g, 300, 0.98, 0.98, 0.0)])                # a square: every edge gives the same area
    out["boxes"] = ([box(g, 300, 1.2, 0.5, d) for d in (0.0, 30.0, 45.0, 60.0, 90.0, 120.0)] + [tie], 0.2, 5)
    t = g.uniform(0.0, np.pi / 2, 250)
    arc = np.c_[0.8 * np.cos(t), 0.8 * np.sin(t)] + g.normal(0, 0.005, (250, 2))
    near = np.c_[np.linspace(0, 2, 200), 0.3 * np.linspace(0, 2, 200) + g.normal(0, 0.003, 200)]
    k = np.arange(64) / 32.0
    out["thin"] = ([arc, near, np.c_[k, k], np.c_[k, np.zeros(64)]], 0.2, 5)   # arc, near-line, two exact lines
    u, v = np.meshgrid(0.25 * np.arange(20), 0.25 * np.arange(20), indexing="ij")
    out["lattice"] = ([np.c_[u.ravel(), v.ravel()]], 0.3, 3)                 # 3: a corner has itself and two neighbours
    return out


def lift(clusters, g):
    """(x, y, z) rows, y = 2.0, shuffled; cluster k is centred 4 m * k along u (a multiple of 4: lattice stays exact)."""
    uv = np.concatenate([c + [4.0 * k, 8.0] for k, c in enumerate(clusters)])
    uv = uv[g.permutation(len(uv))]
    return np.c_[-uv[:, 0], np.full(len(uv), 2.0), uv[:, 1]]


def exact_signs(uv):
    """Condition (a) for one cluster."""
    n = len(uv)
    scale = 2.0 ** 20
    ints = np.round(uv * scale)
    lattice = bool((ints / scale == uv).all() and np.abs(ints).max() < 2 ** 30)
    ints = ints.astype(np.int64)
    bu, bv = uv[:, 0][:, None], uv[:, 1][:, None]
    cu, cv = uv[:, 0][None, :], uv[:, 1][None, :]
    for a in range(n):
        l, r = (bu - uv[a, 0]) * (cv - uv[a, 1]), (bv - uv[a, 1]) * (cu - uv[a, 0])
        o = l - r
        bound = (3.0 + 16.0 * EPS_DBL) * 2 * EPS_DBL * (np.abs(l) + np.abs(r))    # Shewchuk's A bound (eps = 2^-53 there)
        doubt = np.abs(o) <= bound
        doubt[a, :] = doubt[:, a] = False                                 # b == a, c == a or b == c: 0, exactly
        doubt[np.arange(n), np.arange(n)] = False
        assert (o[a, :] == 0).all() and (o[:, a] == 0).all() and (np.diag(o) == 0).all()
        if doubt.any():
            assert lattice, "a triple inside the error bound in a cluster that is not on the lattice"
            ib, ic = np.nonzero(doubt)
            ex = (ints[ib, 0] - ints[a, 0]) * (ints[ic, 1] - ints[a, 1]) - (ints[ib, 1] - ints[a, 1]) * (ints[ic, 0] - ints[a, 0])
            assert np.array_equal(np.sign(ex), np.sign(o[ib, ic]).astype(np.int64))


def reference_circle(uv):
    """The reference's fit_circle, verbatim in its calls (scipy.optimize.leastsq from the mean)."""
    from scipy import optimize

    def f_2(c):
        Ri = np.sqrt((uv[:, 0] - c[0]) ** 2 + (uv[:, 1] - c[1]) ** 2)
        return Ri - Ri.mean()

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        c, _ = optimize.leastsq(f_2, (np.mean(uv[:, 0]), np.mean(uv[:, 1])))
    Ri = np.sqrt((uv[:, 0] - c[0]) ** 2 + (uv[:, 1] - c[1]) ** 2)
    r = Ri.mean()
    return float(c[0]), float(c[1]), float(r), float(np.mean((Ri - r) ** 2) / r ** 2)


def main():
    from scipy.spatial import ConvexHull, QhullError

    g = np.random.default_rng(7)
    out = {"scenes": np.array(list(scenes()))}
    circle_tol = 0.0
    for name, (clusters, eps, ms) in scenes().items():
        pts = lift(clusters, g)
        labels, _, st = CN.dbscan(pts, eps, ms)
        assert st[6] == len(clusters) and st[5] == 0, (name, st)          # the clusters as built, no noise
        shapes, hrows, hoffs = S.fit_shapes(pts, labels)
        hv, hvo, vol, circ, kinds = [], [0], [], [], []
        for c in range(len(clusters)):
            rows = np.flatnonzero(labels == c)
            uv = np.c_[-pts[rows, 0], pts[rows, 2]]
            assert 5 <= len(uv) <= 400 + 4
            exact_signs(uv)                                               # (a)
            mine = hrows[hoffs[c]:hoffs[c + 1]]
            try:
                hull = ConvexHull(uv)
                qv, qvol = np.sort(rows[hull.vertices]), float(hull.volume)
                assert np.array_equal(np.sort(mine), qv), (name, c)       # (b)
                assert abs(shapes[c, 12] - qvol) <= 1e-12 * qvol, (name, c, shapes[c, 12], qvol)
            except QhullError:
                qv, qvol = np.zeros(0, np.int64), 0.0
                assert len(mine) < 3 and shapes[c, 12] == 0.0 and shapes[c, 0] == 1.0, (name, c)
            rc = reference_circle(uv)
            _, ref_crit, ref_val = S.criteria(qvol, len(qv), rc[2], rc[3], shapes[c, 7])
            _, my_crit, my_val = S.criteria(shapes[c, 12], shapes[c, 13], shapes[c, 10], shapes[c, 11], shapes[c, 7])
            assert ref_crit == my_crit, (name, c, ref_val, my_val)        # (c)
            far = [abs(a - t) >= 0.05 * t and abs(b - t) >= 0.05 * t for a, b, t in zip(ref_val, my_val, THRESHOLDS)]
            kind = 2 if all(ref_crit) else 1
            if len(qv) >= 3:
                if kind == 2:
                    assert all(far), (name, c, ref_val, my_val)
                else:
                    assert any(f and not t for f, t in zip(far, ref_crit)), (name, c, ref_val, my_val)
            assert kind == shapes[c, 0]
            if kind == 2:                                                 # (d)
                d = max(abs(shapes[c, 8] - rc[0]), abs(shapes[c, 9] - rc[1]), abs(shapes[c, 10] - rc[2]))
                circle_tol = max(circle_tol, d)
            print(f"{name}[{c}] n={len(uv)} hull={len(mine)} kind={kind} circ/err/ratio ref={ref_val} mine={my_val} "
                  f"evals={S.fit_circle(uv)[4]}")
            hv.append(qv)
            hvo.append(hvo[-1] + len(qv))
            vol.append(qvol)
            circ.append(rc)
            kinds.append(kind)
        out[f"{name}_points"] = pts
        out[f"{name}_params"] = np.array([eps, ms], dtype=np.float64)
        out[f"{name}_qhull_rows"] = np.concatenate(hv).astype(np.int64)
        out[f"{name}_qhull_offsets"] = np.array(hvo, dtype=np.int64)
        out[f"{name}_qhull_volume"] = np.array(vol)
        out[f"{name}_leastsq"] = np.array(circ)
        out[f"{name}_kind"] = np.array(kinds, dtype=np.int64)
    assert circle_tol > 0.0
    out["circle_tol"] = np.float64(circle_tol)
    print("circle_tol", circle_tol)
    np.savez_compressed(os.path.join(HERE, "golden_shapes.npz"), **out)


if __name__ == "__main__":
    main()
