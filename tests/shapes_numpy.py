"""numpy restatement of the shape stage's specification (include/dp_mi355x.h, "Cluster shapes"): the
monotone chain with the stated predicate, the calipers, the stated circle iteration and the decision.
Tests compare the device against it; the golden fixture (tests/golden/golden_shapes.npz, made with
scipy's ConvexHull and leastsq) pins the restatement itself.  No code shared with the package.

Every fp64 operation is written out one at a time, so numpy rounds each on its own as the header
asks; only sums over a cluster (np.sum: pairwise) are in an order of their own.
"""

import math

import numpy as np

H_MAX = 2048
COLUMNS = ("kind", "count", "rect_cu", "rect_cv", "width", "height", "angle", "area", "xc", "yc", "r", "fit_error",
           "hull_area", "hull_vertices", "circ", "error")
DEG = 57.29577951308232


def orient(a, b, c):
    """o(a, b, c) of rule 2."""
    return (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])


def hull(uv):
    """Rule 2: indices (into uv) of the hull's vertices, counter-clockwise from the smallest (u, v)."""
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    idx = np.lexsort((np.arange(len(uv)), uv[:, 1], uv[:, 0]))            # by (u, v, row)
    first = [i for k, i in enumerate(idx) if k == 0 or tuple(uv[i]) != tuple(uv[idx[k - 1]])]

    def chain(seq):
        st = []
        for i in seq:
            while len(st) >= 2 and not orient(uv[st[-2]], uv[st[-1]], uv[i]) > 0:
                st.pop()
            st.append(i)
        return st

    if len(first) == 1:
        return np.array(first, dtype=np.int64)
    lo, up = chain(first), chain(first[::-1])
    return np.array(lo[:-1] + up[:-1], dtype=np.int64)


def hull_area(p):
    """Rule 2: the shoelace sum from the first vertex."""
    if len(p) < 3:
        return 0.0
    t = (p[1:-1, 0] - p[0, 0]) * (p[2:, 1] - p[0, 1]) - (p[1:-1, 1] - p[0, 1]) * (p[2:, 0] - p[0, 0])
    return float(np.sum(t)) / 2.0


def edge_rect(p, i):
    """Rule 3 for edge i of the vertex list p: (area, width, height, e_u, e_v, centre u, centre v)."""
    d = p[(i + 1) % len(p)] - p[i]
    ln = np.sqrt(d[0] * d[0] + d[1] * d[1])
    eu, ev = d[0] / ln, d[1] / ln
    pp = p[:, 0] * eu + p[:, 1] * ev
    qq = p[:, 1] * eu - p[:, 0] * ev
    w, h = pp.max() - pp.min(), qq.max() - qq.min()
    pc, qc = (pp.min() + pp.max()) / 2.0, (qq.min() + qq.max()) / 2.0
    return w * h, w, h, eu, ev, eu * pc - ev * qc, ev * pc + eu * qc


def min_area_rect(p):
    """Rule 3: (centre u, centre v, width, height, angle, area) of the hull vertices p."""
    p = np.asarray(p, dtype=np.float64).reshape(-1, 2)
    if len(p) < 2:
        return float(p[0, 0]), float(p[0, 1]), 0.0, 0.0, 0.0, 0.0
    best = None
    for i in range(len(p)):
        r = edge_rect(p, i)
        if best is None or r[0] < best[0]:
            best = r
    area, w, h, eu, ev, cu, cv = best
    ang = math.atan2(ev, eu) * DEG
    k = math.floor(ang / 90.0)
    ang = ang - 90.0 * k
    if ang >= 90.0:
        ang, k = 0.0, k + 1
    if k % 2:
        w, h = h, w
    return float(cu), float(cv), float(w), float(h), float(ang), float(area)


def _sums(uv, x, y):
    du, dv = uv[:, 0] - x, uv[:, 1] - y
    R = np.sqrt(du * du + dv * dv)
    with np.errstate(invalid="ignore", divide="ignore"):
        a = np.where(R == 0.0, 0.0, du / R)
        b = np.where(R == 0.0, 0.0, dv / R)
    return [float(np.sum(v)) for v in (R, a, b, a * a, a * b, b * b, a * R, b * R, R * R)]


def fit_circle(uv):
    """Rule 4: (xc, yc, r, fit_error, evaluations)."""
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    N = float(len(uv))
    x, y = float(np.sum(uv[:, 0])) / N, float(np.sum(uv[:, 1])) / N
    e = _sums(uv, x, y)
    lam, evals = 1e-3, 0
    for _ in range(50):
        SR, Sa, Sb, Saa, Sab, Sbb, SaR, SbR, SRR = e
        Rm = SR / N
        A11, A12, A22 = Saa - Sa * Sa / N, Sab - Sa * Sb / N, Sbb - Sb * Sb / N
        g1, g2 = SaR - Sa * Rm, SbR - Sb * Rm
        cost = SRR - SR * Rm
        M11, M22 = A11 * (1.0 + lam), A22 * (1.0 + lam)
        det = M11 * M22 - A12 * A12
        if not det > 0.0:
            break
        dx, dy = (M22 * g1 - A12 * g2) / det, (M11 * g2 - A12 * g1) / det
        t = _sums(uv, x + dx, y + dy)
        evals += 1
        if t[8] - t[0] * (t[0] / N) <= cost:
            x, y, e = x + dx, y + dy, t
            lam = lam / 10.0
            if math.sqrt(dx * dx + dy * dy) <= 1e-13 * (t[0] / N):
                break
        else:
            lam = lam * 10.0
            if lam > 1e10:
                break
    r = e[0] / N
    du, dv = uv[:, 0] - x, uv[:, 1] - y
    d = np.sqrt(du * du + dv * dv) - r
    with np.errstate(invalid="ignore", divide="ignore"):
        err = float(np.float64(np.sum(d * d)) / N / np.float64(r * r))
    return x, y, r, err, evals


def criteria(harea, hn, r, err, rect_area, thr=0.85):
    """Rule 5: (circ, [circ > thr, err < 0.15, area ratio < 0.3], the three compared values)."""
    ca = math.pi * (r * r)
    if hn < 3 or not harea > 0.0:
        return 0.0, [False, False, False], (0.0, err, float("nan"))
    with np.errstate(invalid="ignore", divide="ignore"):
        circ = np.float64(harea) / np.float64(ca)
        inv = np.float64(1.0) / circ
        circ = float(inv if inv < circ else circ)
        big = rect_area if rect_area > ca else ca
        ratio = float(np.float64(abs(ca - rect_area)) / np.float64(big))
    return circ, [bool(circ > thr), bool(err < 0.15), bool(ratio < 0.3)], (circ, err, ratio)


def fit_cluster(uv, thr=0.85):
    """One cluster's row (16,) and its hull (indices into uv)."""
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    row = np.zeros(16)
    row[1] = len(uv)
    if len(uv) < 5:
        return row, np.zeros(0, np.int64)
    hi = hull(uv)
    if len(hi) > H_MAX:
        row[15] = 1.0
        return row, np.zeros(0, np.int64)
    p = uv[hi]
    row[12], row[13] = hull_area(p), len(hi)
    row[2:8] = min_area_rect(p)
    row[8:12] = fit_circle(uv)[:4]
    circ, crit, _ = criteria(row[12], len(hi), row[10], row[11], row[7], thr)
    row[14] = circ
    row[0] = 2.0 if all(crit) else 1.0
    return row, hi


def decide(row, thr=0.85):
    """The kind that rule 5 gives a row's own columns."""
    if row[0] == 0:
        return 0
    return 2 if all(criteria(row[12], row[13], row[10], row[11], row[7], thr)[1]) else 1


def fit_shapes(points, labels, max_clusters=4096, thr=0.85):
    """(shapes (K, 16), hull_rows, hull_offsets (K + 1,)) for the clusters of `labels` (-1 / -2: none)."""
    P = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    labels = np.asarray(labels)
    k = min(int(labels.max()) + 1 if len(labels) and labels.max() >= 0 else 0, max_clusters)
    shapes, rows, offs = np.zeros((k, 16)), [], [0]
    for c in range(k):
        r = np.flatnonzero(labels == c)
        shapes[c], hi = fit_cluster(np.c_[-P[r, 0], P[r, 2]], thr)
        rows.append(r[hi])
        offs.append(offs[-1] + len(hi))
    return shapes, (np.concatenate(rows) if rows else np.zeros(0, np.int64)).astype(np.int64), np.array(offs, np.int64)


def inside_rect(uv, row):
    """Largest distance by which a point of uv lies outside the row's rectangle (<= 0: all inside)."""
    a = row[6] / DEG
    eu, ev = math.cos(a), math.sin(a)
    du, dv = uv[:, 0] - row[2], uv[:, 1] - row[3]
    p, q = du * eu + dv * ev, dv * eu - du * ev
    return float(max(np.abs(p).max() - row[4] / 2.0, np.abs(q).max() - row[5] / 2.0))
