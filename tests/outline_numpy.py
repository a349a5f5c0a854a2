"""Sequential numpy restatement of "Floor-plan polygons" (include/dp_mi355x.h, rules O1-O5 and S1-S7): the border
following, CHAIN_APPROX_SIMPLE, contourArea and arcLength, the closed Douglas-Peucker, the exact validity test,
the rectangle snap, the mean height and the polygons file.  Tests compare the device against it; the non-GPU
tests pin it to scipy.ndimage (the set of border cells) and scipy.spatial (the hull).  No code shared with the
package; the hull and the calipers are the shapes stage's restatement (tests/shapes_numpy.py).
"""

import math

import numpy as np

import shapes_numpy as SN

INT_COLUMNS, REAL_COLUMNS, POLYGON_COLUMNS = 4, 2, 8
DROP_NONE, DROP_SMALL, DROP_FEW, DROP_INVALID, DROP_OVERFLOW = range(5)
# rule O2: 0 = E, counter-clockwise on the screen with z down
DX = (1, 1, 0, -1, -1, -1, 0, 1)
DZ = (0, -1, -1, -1, 0, 1, 1, 1)


def trace(labels, label):
    """Rules O1-O3 for one region: (emitted cells [(x, z)], vertices [(x, z)])."""
    h, w = labels.shape
    cells = np.flatnonzero(labels.reshape(-1) == label)
    if not len(cells):
        return [], []
    sz, sx = divmod(int(cells[0]), w)

    def member(x, z):
        return 0 <= x < w and 0 <= z < h and labels[z, x] == label

    s0 = next((d for d in (4, 3, 2, 1, 0, 7, 6, 5) if member(sx + DX[d], sz + DZ[d])), None)
    if s0 is None:
        return [(sx, sz)], [(sx, sz)]
    i1 = (sx + DX[s0], sz + DZ[s0])
    x, z, din = sx, sz, s0
    emitted, vertices = [], []
    for _ in range(8 * len(cells)):
        dout = next(d & 7 for d in range(din + 1, din + 9) if member(x + DX[d & 7], z + DZ[d & 7]))
        emitted.append((x, z))
        if dout != din ^ 4:
            vertices.append((x, z))
        nx, nz = x + DX[dout], z + DZ[dout]
        if (nx, nz) == (sx, sz) and (x, z) == i1:
            break
        x, z, din = nx, nz, dout ^ 4
    return emitted, vertices


def shoelace(v):
    """The signed sum of rule O4 over a vertex list, exact."""
    n = len(v)
    return sum(int(v[i][0]) * int(v[(i + 1) % n][1]) - int(v[(i + 1) % n][0]) * int(v[i][1]) for i in range(n))


def perimeter(v):
    """arcLength(closed) of rule O4: float32 lengths, fp64 sum in vertex order."""
    n, total = len(v), 0.0
    for i in range(n):
        dx = np.float32(v[(i + 1) % n][0] - v[i][0])
        dy = np.float32(v[(i + 1) % n][1] - v[i][1])
        total += float(np.sqrt(np.float32(np.float32(dx * dx) + np.float32(dy * dy))))
    return total


def region_outlines(labels, n_regions=None, max_regions=4096, max_vertices=1 << 20):
    """dp_region_outlines: {"offsets", "vertices", "columns", "measures", "stats", "emitted"}."""
    labels = np.asarray(labels)
    h, w = labels.shape
    n = int(labels.max()) if n_regions is None and labels.size else int(n_regions or 0)
    rows = min(n, max_regions)
    cols = np.zeros((rows, INT_COLUMNS), np.int64)
    real = np.zeros((rows, REAL_COLUMNS))
    offsets = np.zeros(rows + 1, np.int32)
    verts, emitted_all = [], []
    total = written = 0
    for r in range(rows):
        emitted, v = trace(labels, r + 1)
        emitted_all.append(emitted)
        s = shoelace(v) if v else 0
        cols[r] = (len(v), len(emitted), s, v[0][1] * w + v[0][0] if v else -1)
        real[r] = (abs(s) / 2.0, perimeter(v))
        total += len(v)
        if total <= max_vertices:
            verts.extend(v)
            written = total
        offsets[r + 1] = written
    stats = np.array([n, rows, total, written, float(total > written), float(n > max_regions), h, w], np.float64)
    return {"offsets": offsets, "vertices": np.array(verts, np.int32).reshape(-1, 2), "columns": cols, "measures": real,
            "stats": stats, "emitted": emitted_all}


def anchors(v):
    """S3: (A, B, the last largest squared distance)."""
    n = len(v)
    cur, far, best = 0, 0, 0
    for _ in range(3):
        cur = (cur + far) % n
        best = 0
        for j in range(1, n):
            p = v[(cur + j) % n]
            d = (int(p[0]) - int(v[cur][0])) ** 2 + (int(p[1]) - int(v[cur][1])) ** 2
            if d > best:
                best, far = d, j
    return cur, (cur + far) % n, best


def douglas_peucker(v, eps):
    """S3: the indices (into v) of the kept vertices, in ring order from the anchor A."""
    n = len(v)
    a, b, best = anchors(v)
    eps2 = eps * eps
    if float(best) <= eps2 or a == b:
        return [a]
    jb = (b - a) % n
    keep = {0, jb}
    stack = [(0, jb), (jb, n)]
    while stack:
        s, e = stack.pop()
        ps, pe = v[(a + s) % n], v[(a + e) % n]
        dx, dy = int(pe[0]) - int(ps[0]), int(pe[1]) - int(ps[1])
        c_best, at = 0, -1
        for j in range(s + 1, e):
            p = v[(a + j) % n]
            c = abs((int(p[1]) - int(ps[1])) * dx - (int(p[0]) - int(ps[0])) * dy)
            if at < 0 or c > c_best:
                c_best, at = c, j
        if at >= 0 and float(c_best) * float(c_best) > eps2 * float(dx * dx + dy * dy):
            keep.add(at)
            stack += [(s, at), (at, e)]
    return [(a + j) % n for j in sorted(keep)]


def _orient(a, b, c):
    return (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])


def _on_segment(a, b, c):
    return min(a[0], b[0]) <= c[0] <= max(a[0], b[0]) and min(a[1], b[1]) <= c[1] <= max(a[1], b[1])


def segments_meet(a, b, c, d):
    d1, d2, d3, d4 = _orient(c, d, a), _orient(c, d, b), _orient(a, b, c), _orient(a, b, d)
    if d1 * d2 < 0 and d3 * d4 < 0:
        return True
    return (d1 == 0 and _on_segment(c, d, a)) or (d2 == 0 and _on_segment(c, d, b)) or \
        (d3 == 0 and _on_segment(a, b, c)) or (d4 == 0 and _on_segment(a, b, d))


def ring_valid(p):
    """S5 on a ring of integer vertices."""
    p = [(int(x), int(y)) for x, y in p]
    m = len(p)
    if m < 3 or shoelace(p) == 0 or len(set(p)) < m:
        return False
    for i in range(m):
        a, b, c = p[i], p[(i + 1) % m], p[(i + 2) % m]
        if _orient(a, b, c) == 0 and (b[0] - a[0]) * (c[0] - b[0]) + (b[1] - a[1]) * (c[1] - b[1]) < 0:
            return False
        for j in range(i + 2, m):
            if i == 0 and j == m - 1:
                continue
            if segments_meet(a, b, p[j], p[(j + 1) % m]):
                return False
    return True


def box_points(cx, cy, w, h, angle):
    """cv2.boxPoints of ((cx, cy), (w, h), angle in degrees)."""
    ang = angle / SN.DEG
    b, a = math.cos(ang) * 0.5, math.sin(ang) * 0.5
    p0 = (cx - a * h - b * w, cy + b * h - a * w)
    p1 = (cx + a * h - b * w, cy - b * h - a * w)
    return np.array([p0, p1, (2.0 * cx - p0[0], 2.0 * cy - p0[1]), (2.0 * cx - p1[0], 2.0 * cy - p1[1])])


def snap(ring):
    """S6: (corners (4, 2), rect_area) when the ring snaps, else None."""
    ring = np.asarray(ring, np.float64)
    if not 4 <= len(ring) <= 6:
        return None
    hull = ring[SN.hull(ring)]
    cx, cy, w, h, ang, area = SN.min_area_rect(hull)
    ring_area = abs(shoelace(ring.astype(np.int64))) / 2.0
    if abs(area - ring_area) / ring_area < 0.2:
        return box_points(cx, cy, w, h, ang), area, (cx, cy, w, h, ang)
    return None


def simplify_one(v, area, per, resolution, min_area):
    """S1-S6 for one outline: (reason, ring or corners as float64 (n, 2), snapped, area in cells, epsilon, ring indices)."""
    eps = 0.005 * per
    if area * (resolution * resolution) < min_area / 4.0:
        return DROP_SMALL, None, 0, 0.0, eps, []
    if v is None:
        return DROP_OVERFLOW, None, 0, 0.0, eps, []
    idx = douglas_peucker(v, eps)
    if len(idx) < 3:
        return DROP_FEW, None, 0, 0.0, eps, idx
    ring = [tuple(int(c) for c in v[i]) for i in idx]
    if not ring_valid(ring):
        return DROP_INVALID, None, 0, 0.0, eps, idx
    s = snap(ring)
    if s is not None:
        return DROP_NONE, s[0], 1, s[1], eps, idx
    return DROP_NONE, np.array(ring, np.float64), 0, abs(shoelace(ring)) / 2.0, eps, idx


def simplify_outlines(out, resolution=0.1, min_area=0.025, max_polygon_vertices=1 << 20):
    """dp_simplify_outlines on a region_outlines result: {"offsets", "vertices", "polygons", "stats"}."""
    rows = len(out["columns"])
    pol = np.zeros((rows, POLYGON_COLUMNS))
    offsets = np.zeros(rows + 1, np.int32)
    verts, counts = [], np.zeros(5, np.int64)
    total = written = 0
    for r in range(rows):
        nv = int(out["columns"][r, 0])
        lo, hi = int(out["offsets"][r]), int(out["offsets"][r + 1])
        v = out["vertices"][lo:hi] if nv > 0 and hi - lo == nv else None
        reason, p, snapped, area, eps, _ = simplify_one(v, out["measures"][r, 0], out["measures"][r, 1], resolution, min_area)
        n = 0 if reason else len(p)
        total += n
        if n and total > max_polygon_vertices:
            reason, n = DROP_OVERFLOW, 0                                   # flags and areas stay: the polygon exists
        elif n:
            verts.extend(p.tolist())
            written = total
        offsets[r + 1] = written
        counts[reason] += 1
        pol[r] = (r + 1, n, snapped, area, area * (resolution * resolution), eps, reason, nv)
    stats = np.array([rows, counts[0], total, written, counts[4], counts[1], counts[2], counts[3]], np.float64)
    return {"offsets": offsets, "vertices": np.array(verts, np.float64).reshape(-1, 2), "polygons": pol, "stats": stats}


def mean_height(points, count=None, height_threshold=1.3):
    """The file's height label: (mean y of the raster's participants, their number)."""
    pts = np.asarray(points, np.float64).reshape(-1, 3)[:count]
    ok = np.isfinite(pts).all(axis=1)
    if not math.isnan(height_threshold):
        ok &= ~(pts[:, 1] < height_threshold)
    n = int(ok.sum())
    return (float(np.mean(pts[ok, 1])) if n else float(height_threshold)), n


def world_reference(p, origin, resolution):
    """shapely.affinity.scale about the bounding-box centre, then the translation by the grid origin."""
    p = np.asarray(p, np.float64)
    cx = (p[:, 0].min() + p[:, 0].max()) / 2.0
    cy = (p[:, 1].min() + p[:, 1].max()) / 2.0
    return np.c_[cx + (p[:, 0] - cx) * resolution + origin[0], cy + (p[:, 1] - cy) * resolution + origin[1]]


def floorplan_text(polys, height, origin, resolution):
    """save_floorplan_data: `polys` is the list of kept polygons (grid units) in label order; the file lists them
    last-found first."""
    lines = ["# Floor Plan Data\n", "# Units: meters\n\n", "# Shapes by height\n",
             "# Format: height, num_points, x1, z1, x2, z2, ...\n"]
    for p in polys[::-1]:
        wxy = world_reference(p, origin, resolution)
        lines.append(f"{height:.3f}, {len(wxy)}" + "".join(f", {x:.3f}, {z:.3f}" for x, z in wxy) + "\n")
    return "".join(lines)
