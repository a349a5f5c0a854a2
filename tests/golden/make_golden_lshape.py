"""Makes tests/golden/golden_lshape.npz: hand-built rectangles and point sets for the L-shape split (additive to ABI 20)
with the outcome of the header's rules computed a second, independent way, and asserts the conditions
that make the fixture a fair yardstick.  CPU only:

    python tests/golden/make_golden_lshape.py

cv2 and shapely are not installed here, so the reference's detect_and_split_l_shapes itself cannot be
run: the 2 x 2 dilation anchor and the strict interior rule are taken from OpenCV's and shapely's
documentation, and nothing here verifies them against those libraries.  This file imports nothing from
the reference.  What it does is compute the header's rules without the restatement's own means:
  - membership by matplotlib.path.Path.contains_points on the rectangle's fp64 corners, and the points' places
    in the grid from their distances to the low corner along the two edges (a rotation written here, not the
    restatement's);
  - the dilation by an explicit shifted OR;
  - both labellings, their sizes and their numbering by scipy.ndimage.label (cross structure) and
    ndimage.sum;
  - the parts by shapes_numpy's hull and calipers (rule 3 of "Cluster shapes").

Conditions (a scene that violates one is changed, never excused):
 (a) every point's |x'| - w/2 and |y'| - h/2 is at least 1e-9 m from 0 in every rectangle that reaches rule 2;
 (b) every (x' + w/2) / 0.2 and (y' + h/2) / 0.2 of an inside point, and every w / 0.2 and h / 0.2, is at
     least 1e-9 from an integer;
 (c) every threshold that decides a status (10, 50, 0.2, 0.6, 1.0, 0.4, 1.3, and the 6 cells of a
     component) is missed by at least 5 % of its value -- except in the scene `holes`, which puts
     components of 5 and 6 cells on the integer threshold on purpose (an integer comparison);
 (d) this computation and the restatement (tests/lshape_numpy.py) agree on every status, count and cell;
 (e) every status 0..9 occurs.
"""

import math
import os
import sys

import numpy as np
from matplotlib.path import Path
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import lshape_numpy as LN  # noqa: E402
import shapes_numpy as SN  # noqa: E402

CELL = 0.2
CROSS = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])


# ---- scenes -------------------------------------------------------------------------------------------

def cells_to_points(g, rect, cells, per=1):
    """World (x, y, z) rows for `per` points in each (gy, gx) cell of the rectangle's own grid."""
    cu, cv, w, h, ang = rect[:5]
    a = -ang * math.pi / 180.0
    c, s = math.cos(a), math.sin(a)
    cells = np.repeat(np.asarray(cells, dtype=np.float64).reshape(-1, 2), per, axis=0)
    xr = -w / 2.0 + (cells[:, 1] + 0.5 + g.uniform(-0.3, 0.3, len(cells))) * CELL
    yr = -h / 2.0 + (cells[:, 0] + 0.5 + g.uniform(-0.3, 0.3, len(cells))) * CELL
    u, v = cu + (xr * c + yr * s), cv + (-xr * s + yr * c)
    return np.c_[-u, np.full(len(u), 1.5), v]


def box(y0, y1, x0, x1):
    """The cells of rows y0..y1 and columns x0..x1, inclusive."""
    return [(y, x) for y in range(y0, y1 + 1) for x in range(x0, x1 + 1)]


def rect(cu, cv, w, h, ang, cluster=0, flags=0):
    return np.array([cu, cv, w, h, ang, cluster, flags, 0.0])


def scenes():
    g = np.random.default_rng(21)
    S = {}

    def add(name, rects, pts, labels=None, max_cells=1 << 20, **extra):
        pts = np.concatenate(pts)
        S[name] = dict(rects=np.array(rects).reshape(-1, 8), points=pts, max_cells=max_cells,
                       labels=np.zeros(len(pts), np.int32) if labels is None else np.concatenate(labels).astype(np.int32),
                       **extra)

    slab = box(0, 5, 0, 29) + box(14, 19, 0, 29)                  # two 6 x 1.2 slabs, a 1.6 m gap
    rs = [rect(0, 5, 6.1, 4.1, 0.0, 0), rect(20, 5, 6.1, 4.1, 30.0, 1), rect(40, 5, 6.1, 4.1, 120.0, 2)]
    add("slabs", rs, [cells_to_points(g, r, slab, 2) for r in rs])

    r = rect(3, -2, 8.1, 6.1, 15.0)
    ring = [c for c in box(0, 29, 0, 39) if c[0] in (0, 29) or c[1] in (0, 39)]
    add("room", [r], [cells_to_points(g, r, ring + box(8, 22, 10, 29))], ring=len(ring))

    r = rect(-4, 7, 6.1, 4.1, 75.0)
    add("true_L", [r], [cells_to_points(g, r, box(0, 5, 0, 29) + box(6, 19, 0, 7))])

    r = rect(1, 1, 3.05, 3.05, 10.0)
    add("small", [r], [cells_to_points(g, r, box(0, 13, 0, 13))])
    r = rect(1, 1, 6.1, 4.1, 100.0)
    add("few", [r], [cells_to_points(g, r, box(3, 3, 0, 29))])                       # 30 points
    r = rect(2, 3, 0.3, 40.1, 40.0)
    add("thin", [r], [cells_to_points(g, r, box(0, 59, 0, 0))])                      # gw = 2
    r = rect(-2, 3, 6.1, 4.1, 160.0)
    add("full", [r], [cells_to_points(g, r, box(0, 19, 0, 29))])
    r = rect(-2, 3, 6.1, 4.1, 50.0)
    add("sparse", [r], [cells_to_points(g, r, box(0, 1, 0, 29))])
    r = rect(5, 5, 6.1, 4.1, 20.0)
    add("few_parts", [r], [cells_to_points(g, r, box(0, 9, 0, 29) + box(15, 16, 10, 11))])
    r = rect(5, -5, 6.1, 4.1, 65.0)
    add("thin_parts", [r], [cells_to_points(g, r, sum((box(y, y, 0, 29) for y in (0, 4, 8, 12, 16)), []))])
    r = rect(0, 0, 6.1, 4.1, 35.0)
    hole5, hole6 = box(5, 6, 4, 9), box(5, 6, 14, 20)             # 2 x 6 and 2 x 7 bare cells: 1 x 5 and 1 x 6 after dilation
    add("holes", [r], [cells_to_points(g, r, [c for c in box(0, 19, 0, 29) if c not in hole5 + hole6])])

    # a cluster of 1200 points over 12.1 x 9.1 through the rectangle list: both halves go in
    big = rect(2, 2, 12.1, 9.1, 20.0)
    shapes = np.zeros((2, 16))
    shapes[0, :8] = [1.0, 1200.0, 2.0, 2.0, 12.1, 9.1, 20.0, 12.1 * 9.1]
    shapes[1, :8] = [2.0, 40.0, 9.0, 9.0, 1.0, 1.0, 0.0, 1.0]     # a circle: no rectangle
    halves = LN.rectangle_list(shapes)
    add("halves", halves, [cells_to_points(g, big, box(0, 29, 0, 39))], shapes=shapes)

    r = rect(0, 0, 60.1, 2.1, 25.0)
    add("long", [r], [cells_to_points(g, r, box(0, 2, 0, 299) + box(6, 8, 0, 299))])

    rs = [rect(0, 0, 6.1, 4.1, 30.0, 0), rect(20, 0, 6.1, 4.1, 60.0, 1), rect(0, 40, 210.1, 1.1, 5.0, 2)]
    add("cap", rs, [cells_to_points(g, rs[0], slab), cells_to_points(g, rs[1], slab),
                    cells_to_points(g, rs[2], box(2, 2, 0, 59))], max_cells=700)

    # the second slab is noise and another cluster's members; rows with label -2 fill the gap but take no part
    r = rect(0, 0, 6.1, 4.1, 45.0)
    p0 = cells_to_points(g, r, box(0, 5, 0, 29))
    p1 = cells_to_points(g, r, box(14, 19, 0, 29))
    p2 = cells_to_points(g, r, box(7, 12, 0, 29))
    l1 = np.where(np.arange(len(p1)) % 2 == 0, -1, 1)
    add("strangers", [r], [p0, p1, p2], [np.zeros(len(p0)), l1, np.full(len(p2), -2)])
    return S


# ---- the second computation ---------------------------------------------------------------------------

def corners(r):
    cu, cv, w, h, ang = r[:5]
    a = -ang * math.pi / 180.0
    c, s = math.cos(a), math.sin(a)
    out = []
    for xr, yr in ((-w / 2, -h / 2), (w / 2, -h / 2), (w / 2, h / 2), (-w / 2, h / 2)):
        out.append((cu + (xr * c + yr * s), cv + (-xr * s + yr * c)))
    return np.array(out)


def margin(x, thr):
    return abs(x - thr) / thr


def second(r, uv, grid_ok, loose6):
    """(info (8,), parts, cells dict) by the means of this file; asserts (a), (b), (c) on the way."""
    cu, cv, w, h, ang = (float(v) for v in r[:5])
    info = np.zeros(8)
    assert margin(w * h, 10.0) >= 0.05
    if w * h < 10.0:
        info[0] = 1
        return info, [], {}
    # coordinates in the rectangle's frame from its corners (not from the restatement's rotation): the distance from
    # the low corner along the width and the height edge
    k = corners(r)
    ex, ey = (k[1] - k[0]) / w, (k[3] - k[0]) / h
    px, py = (uv - k[0]) @ ex, (uv - k[0]) @ ey
    xr, yr = px - w / 2, py - h / 2
    c, s = math.cos(-ang * math.pi / 180.0), math.sin(-ang * math.pi / 180.0)
    assert min(np.abs(np.abs(xr) - w / 2).min(), np.abs(np.abs(yr) - h / 2).min()) >= 1e-9            # (a)
    inside = Path(corners(r)).contains_points(uv)
    n_in = int(inside.sum())
    gw, gh = int(math.floor(w / CELL)) + 1, int(math.floor(h / CELL)) + 1
    for q in (w / CELL, h / CELL):
        assert abs(q - round(q)) >= 1e-9                                                              # (b)
    info[1:4] = n_in, gw, gh
    assert margin(n_in, 50.0) >= 0.05
    if n_in < 50:
        info[0] = 2
        return info, [], {}
    if gw <= 2 or gh <= 2:
        info[0] = 3
        return info, [], {}
    if gw > 1024 or gh > 1024 or not grid_ok:
        info[0], info[7] = 9, 1
        return info, [], {}
    fx, fy = px[inside] / CELL, py[inside] / CELL
    assert min(np.abs(fx - np.round(fx)).min(), np.abs(fy - np.round(fy)).min()) >= 1e-9              # (b)
    b = np.zeros((gh, gw), bool)
    b[np.floor(fy).astype(int), np.floor(fx).astype(int)] = True
    d = np.zeros_like(b)
    for dy in (0, 1):
        for dx in (0, 1):
            d[dy:, dx:] |= b[:gh - dy, :gw - dx]
    lab, n = ndimage.label(~d, structure=CROSS)
    sizes = ndimage.sum(~d, lab, index=np.arange(1, n + 1)).astype(int) if n else np.zeros(0, int)
    if not loose6:
        assert all(margin(v, 6.0) >= 0.05 for v in sizes)
    empty_mask = np.isin(lab, 1 + np.flatnonzero(sizes >= 6))
    cells = dict(b=b, d=d, empty_mask=empty_mask)
    info[4] = empty_mask.sum()
    if not (sizes >= 6).any():
        info[0] = 4
        return info, [], cells
    ratio = empty_mask.sum() / (gw * gh)
    assert margin(ratio, 0.2) >= 0.05 and margin(ratio, 0.6) >= 0.05
    if ratio < 0.2 or ratio > 0.6:
        info[0] = 5
        return info, [], cells
    olab, m = ndimage.label(~empty_mask, structure=CROSS)
    osz = ndimage.sum(~empty_mask, olab, index=np.arange(1, m + 1)).astype(int)
    assert all(margin(v, 6.0) >= 0.05 for v in osz)
    cells["olab"] = olab
    info[5] = m
    if m < 2:
        info[0] = 6
        return info, [], cells
    parts, area = [], 0.0
    for k in 1 + np.flatnonzero(osz >= 6):
        ys, xs = np.nonzero(olab == k)
        p = np.c_[xs * CELL - w / 2, ys * CELL - h / 2]
        sx, sy, sw, sh, sa, _ = SN.min_area_rect(p[SN.hull(p)])
        assert margin(sw * sh, 1.0) >= 0.05
        if sw * sh > 1.0:
            parts.append(np.array([(sx * c - sy * s) + cu, (sx * s + sy * c) + cv, sw, sh, math.fmod(sa + ang, 180.0),
                                   r[5], r[6] + 2.0, 0.0]))
            area += sw * sh
    info[6] = len(parts)
    if len(parts) < 2:
        info[0] = 7
        return info, [], cells
    q = area / (w * h)
    assert margin(q, 0.4) >= 0.05 and margin(q, 1.3) >= 0.05
    if not 0.4 < q < 1.3:
        info[0] = 8
        return info, [], cells
    return info, parts, cells


def main():
    out, seen = {}, set()
    for name, sc in scenes().items():
        uv = LN.participants(sc["points"], sc["labels"])
        trace = []
        rows, n_out, info = LN.split_l_shapes(sc["points"], sc["labels"], sc["rects"], sc["max_cells"], trace=trace)
        used, rows2 = 0, []
        for i, r in enumerate(sc["rects"]):
            ok = True
            if not r[2] * r[3] < 10.0:
                gw, gh = int(r[2] / CELL) + 1, int(r[3] / CELL) + 1
                if 2 < gw <= 1024 and 2 < gh <= 1024:
                    used += gw * gh
                    ok = used <= sc["max_cells"]
            inf2, parts, cells = second(r, uv, ok, name == "holes")
            assert np.array_equal(inf2, info[i]), (name, i, inf2, info[i])                            # (d)
            for key, val in cells.items():
                assert np.array_equal(val, trace[i][key]), (name, i, key)
            rows2.extend(parts if inf2[0] == 0 else [r])
            seen.add(int(inf2[0]))
        rows2 = np.array(rows2).reshape(-1, 8)
        assert rows2.shape == rows.shape and np.array_equal(rows2, rows), name
        print(f"{name:11s} points {len(sc['points']):5d}  status {info[:, 0].astype(int).tolist()}  rows {n_out[0]}")
        for key in ("points", "labels", "rects"):
            out[f"{name}.{key}"] = sc[key]
        out[f"{name}.max_cells"] = np.int64(sc["max_cells"])
        out[f"{name}.out"], out[f"{name}.info"] = rows, info
        if "shapes" in sc:
            out[f"{name}.shapes"] = sc["shapes"]
    assert seen == set(range(10)), sorted(seen)                                                       # (e)
    # what the scenes are there to show
    st = lambda n: out[f"{n}.info"][:, 0].astype(int).tolist()  # noqa: E731
    assert st("slabs") == [0, 0, 0] and len(out["slabs.out"]) == 6
    assert st("room") == [0] and out["room.out"][0, 2] * out["room.out"][0, 3] > 0.95 * 8.1 * 6.1
    assert st("true_L") == [6] and st("small") == [1] and st("few") == [2] and st("thin") == [3] and st("full") == [4]
    assert st("sparse") == [5] and st("few_parts") == [7] and st("thin_parts") == [8]
    assert st("holes") == [5] and out["holes.info"][0, 4] == 6
    assert len(out["halves.rects"]) == 2 and st("long") == [0] and out["long.info"][0, 2] == 301
    assert st("cap") == [0, 9, 9]
    sc = scenes()["strangers"]
    own = np.where(sc["labels"] == 0, 0, -2)
    assert st("strangers") == [0] and LN.split_l_shapes(sc["points"], own, sc["rects"])[2][0, 0] == 5
    out["names"] = np.array(sorted({k.split(".")[0] for k in out}))
    path = os.path.join(HERE, "golden_lshape.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
